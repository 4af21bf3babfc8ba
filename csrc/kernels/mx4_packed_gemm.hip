// MXFP4 (W4A16) above the decode row counts: y[M, N] = x[M, K] . dequant(W)[N, K]^T for
// any M (the model uses it for M > 64: prefill chunks, mixed steps, large decode batches)
// on the SAME image the decode kernel streams (mx4a16.hip documents it; ops.quant.pack_mx4:
// wq [N/16][K/128][lane][16 B], sc [N/16][K/128][64] scale bytes), so an MXFP4 model
// keeps no bf16 copy of its projections.
//
// w4_packed_gemm.hip minus everything int4 (no zero-point pairs, no per-group fold, no
// ones-MFMAs), with its K-stage of one 128-wide k-step:
//   * W: one (16-column tile, k-step) block is 1 KiB contiguous in the image, so one
//     global_load_lds_dwordx4 per tile brings the stage; lane l reads back its 16 B at
//     l * 16 and its scale byte, and 16 v_cvt_scalef32_pk_bf16_fp4 widen AND scale them
//     to the four bf16 B fragments of the k-step (dword j = MFMA j, k = 32 g + 8 j + e),
//     once per stage for the wave's MT row tiles;
//   * scale bytes come THROUGH THE STAGE'S DMA: 64 B per column tile and k-step, one
//     instruction covers 16 column tiles (lane l brings bytes 16 (l & 3) .. of tile
//     l >> 2), read back as one ds_read_u8 per column tile.  Every wave issues it (the
//     same bytes to the same place), so the counted vmcnt waits stay uniform;
//   * x: the stage is two 64-k images [BM][64] with packed_gemm.hip's swizzle (16-B
//     chunk c of local row r at slot c ^ ((r >> 1) & 5), applied on the per-lane
//     SOURCE address), 8 rows x 128 B per DMA instruction; the x fragment of MFMA j is
//     piece 4 g + j of the 128 k: image g >> 1, chunk 4 (g & 1) + j;
//   * an S-slot ring, S - 2 stages in flight across the one raw s_barrier per stage,
//     counted vmcnt, no __syncthreads in the loop;
//   * tile order, XCD remap and split-K over gridDim.y are packed_gemm.hip's.
// Numerics are the decode kernel's: sums of the same exact bf16 products fp4 * 2^e into
// fp32, the accumulator is the result; rows above and below 64 see the same weights.
// Rows and column tiles past the end are clamped on load (nothing outside x, the image
// or the scale bytes is read) and masked on store.
// Plain vector stores only; fixed waits and barriers only.
#include "ft_common.h"
#include "ft_lds.h"

namespace ft {

typedef __bf16 mx4pg_bf16x8 __attribute__((ext_vector_type(8)));
typedef float mx4pg_floatx4 __attribute__((ext_vector_type(4)));

enum Mx4pgEpi { kMx4pgStore = 0, kMx4pgSlab = 1, kMx4pgSilu = 2 };

__device__ __forceinline__ mx4pg_bf16x8 mx4pg_frag(const uint4& v) {
  return __builtin_bit_cast(mx4pg_bf16x8, v);
}

__device__ __forceinline__ uint32_t mx4pg_read_u8(uint32_t a) {
  uint32_t v;
  asm volatile("ds_read_u8 %0, %1" : "=v"(v) : "v"(a));
  return v;
}
__device__ __forceinline__ void mx4pg_dep(uint32_t& v) { asm volatile("" : "+v"(v)); }

// one dword (8 e2m1 nibbles, low nibble of byte 0 first) times 2^(byte - 127)
__device__ __forceinline__ uint4 mx4pg_widen(uint32_t w, float scale) {
  const ft_bf16x2_t a = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 0);
  const ft_bf16x2_t b = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 1);
  const ft_bf16x2_t c = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 2);
  const ft_bf16x2_t d = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 3);
  return make_uint4(__builtin_bit_cast(uint32_t, a), __builtin_bit_cast(uint32_t, b),
                    __builtin_bit_cast(uint32_t, c), __builtin_bit_cast(uint32_t, d));
}

template <int PW, int S>
__device__ __forceinline__ void mx4pg_wait_ahead(int ahead) {
  // this wave's DMA groups are issued one stage at a time: leave `ahead` stages
  // (PW instructions each) in flight, retire everything older
  if (S >= 4 && ahead >= 2) {
    vm_wait<(S >= 4 ? 2 * PW : 0)>();
  } else if (S >= 3 && ahead >= 1) {
    vm_wait<(S >= 3 ? PW : 0)>();
  } else {
    vm_wait<0>();
  }
}

template <int WM, int WN, int MT, int NT, int S, int EPI>
__global__ __launch_bounds__(512, 1) void mx4_packed_gemm_kernel(
    const uint16_t* __restrict__ x, int x_stride, int M, const uint8_t* __restrict__ wq,
    const uint8_t* __restrict__ sc, int N, int K, int k_slice, uint16_t* __restrict__ out,
    int out_stride, float* __restrict__ ws) {
  constexpr int NW = WM * WN;
  static_assert(NW == 8, "8 waves");
  constexpr int BM = WM * MT * 16, BN = WN * NT * 16;
  static_assert(BN == 256, "one scale DMA instruction covers 16 column tiles");
  constexpr int A_HALF = BM * 128;            // one 64-k image of the stage
  constexpr int A_BYTES = 2 * A_HALF;
  constexpr int B_BYTES = BN * 64;            // BN / 16 KiB
  constexpr int Z_BYTES = BN * 4;             // 64 scale bytes per column tile
  constexpr int STAGE = A_BYTES + B_BYTES + Z_BYTES;
  constexpr int A_PW = 2 * BM / (8 * NW);     // x DMA instructions per wave per stage
  constexpr int B_INST = BN / 16;             // one per column tile
  static_assert(B_INST % NW == 0 && (2 * BM / 8) % NW == 0, "uniform DMA counts");
  constexpr int B_PW = B_INST / NW;
  constexpr int PW = A_PW + B_PW + 1;         // + one scale instruction
  static_assert(2 * PW < 64, "vmcnt field");
  static_assert(S >= 2 && S <= 4 && S * STAGE <= 160 * 1024, "LDS");
  static_assert(EPI != kMx4pgSilu || NT % 2 == 0, "SiLU pairs need an even NT");
  __shared__ __attribute__((aligned(16))) uint8_t smem[S * STAGE];

  const int lane = lane_id(), w = wave_id();
  const int wm = w / WN, wn = w % WN;
  const int l15 = lane & 15, g = lane >> 4;

  // tile id: XCD-aware bijective remap, m fastest inside an n-block
  const int mt_tiles = (M + BM - 1) / BM;
  const int total = gridDim.x;
  const int orig = blockIdx.x;
  const int q8 = total / 8, r8 = total % 8, xcd = orig % 8;
  const int wgid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + orig / 8;
  const int tn = wgid / mt_tiles, tm = wgid % mt_tiles;
  const int m0 = tm * BM, n0 = tn * BN;
  const int s = blockIdx.y;
  const int kbeg = s * k_slice;
  const int nk = k_slice >> 7;                // k-steps of this split
  const int steps_total = K >> 7;
  const int step0 = kbeg >> 7;
  const int ntiles_all = N >> 4;

  const uint32_t lds0 = lds_off(smem);

  // per-lane DMA sources (k-step 0 of this split); a stage advances x by 128 elements, W
  // by one 1 KiB block, the scale bytes by one 64-B record.  Rows and column tiles past
  // the end are clamped to the last one: nothing outside x or the image is read.
  const uint16_t* a_src[A_PW];
#pragma unroll
  for (int i = 0; i < A_PW; ++i) {
    const int inst = i * NW + w;              // LDS destination inst * 1024
    const int step = inst / (BM / 8), rb = inst % (BM / 8);
    const int rl = rb * 8 + (lane >> 3);
    const int c = (lane & 7) ^ ((rl >> 1) & 5);
    const int row = min(m0 + rl, M - 1);
    a_src[i] = x + (size_t)row * x_stride + kbeg + step * 64 + c * 8;
  }
  const uint8_t* b_src[B_PW];
#pragma unroll
  for (int i = 0; i < B_PW; ++i) {
    const int nt = min((n0 >> 4) + i * NW + w, ntiles_all - 1);
    b_src[i] = wq + ((size_t)nt * steps_total + step0) * 1024 + lane * 16;
  }
  const uint8_t* z_src;
  {
    const int nt = min((n0 >> 4) + (lane >> 2), ntiles_all - 1);
    z_src = sc + ((size_t)nt * steps_total + step0) * 64 + (lane & 3) * 16;
  }

  auto issue = [&](int t) {
    const uint32_t base = lds0 + (t % S) * STAGE;
#pragma unroll
    for (int i = 0; i < A_PW; ++i) glds16(a_src[i] + t * 128, base + (i * NW + w) * 1024);
#pragma unroll
    for (int i = 0; i < B_PW; ++i)
      glds16(b_src[i] + (size_t)t * 1024, base + A_BYTES + (i * NW + w) * 1024);
    glds16(z_src + (size_t)t * 64, base + A_BYTES + B_BYTES);
  };

  mx4pg_floatx4 acc[MT][NT];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[i][j] = mx4pg_floatx4{0.f, 0.f, 0.f, 0.f};

  // fragment read offsets inside a stage: MFMA q of the k-step reads piece 4 g + q
  uint32_t a_off[MT][4];
#pragma unroll
  for (int i = 0; i < MT; ++i) {
    const int rl = wm * MT * 16 + i * 16 + l15;
#pragma unroll
    for (int q = 0; q < 4; ++q)
      a_off[i][q] = (g >> 1) * A_HALF + rl * 128 + (((4 * (g & 1) + q) ^ ((rl >> 1) & 5)) * 16);
  }
  const uint32_t b_off = A_BYTES + (wn * NT) * 1024 + lane * 16;
  const uint32_t z_off = A_BYTES + B_BYTES + (wn * NT) * 64 + lane;

#pragma unroll
  for (int t = 0; t < S - 1; ++t)
    if (t < nk) issue(t);

  for (int t = 0; t < nk; ++t) {
    // stage t landed (own DMAs), and every wave is done reading stage t-1's slot
    mx4pg_wait_ahead<PW, S>(min(S - 2, nk - 1 - t));
    lgkm_wait<0>();
    __builtin_amdgcn_s_barrier();
    if (t + S - 1 < nk) issue(t + S - 1);
    const uint32_t base = lds0 + (t % S) * STAGE;
    uint4 bw[NT];
    uint32_t zb[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      bw[j] = ds_read16(base + b_off + j * 1024);
      zb[j] = mx4pg_read_u8(base + z_off + j * 64);
    }
    uint4 af[2][4];
#pragma unroll
    for (int q = 0; q < 4; ++q) af[0][q] = ds_read16(base + a_off[0][q]);
    lgkm_wait<4>();   // the weight words and scale bytes (LDS returns in order)
    uint4 bf[NT][4];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      dep(bw[j]);
      mx4pg_dep(zb[j]);
      const float scale = __builtin_bit_cast(float, zb[j] << 23);
      bf[j][0] = mx4pg_widen(bw[j].x, scale);
      bf[j][1] = mx4pg_widen(bw[j].y, scale);
      bf[j][2] = mx4pg_widen(bw[j].z, scale);
      bf[j][3] = mx4pg_widen(bw[j].w, scale);
    }
#pragma unroll
    for (int i = 0; i < MT; ++i) {
      const int cur = i & 1;
      if (i + 1 < MT) {
#pragma unroll
        for (int q = 0; q < 4; ++q) af[cur ^ 1][q] = ds_read16(base + a_off[i + 1][q]);
        lgkm_wait<4>();
      } else {
        lgkm_wait<0>();
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) dep(af[cur][q]);
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int j = 0; j < NT; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(mx4pg_frag(af[cur][q]),
                                                              mx4pg_frag(bf[j][q]), acc[i][j], 0, 0, 0);
      __builtin_amdgcn_s_setprio(0);
    }
  }

  // epilogue: C layout, lane (g, l15) holds rows 4g..4g+3 of column l15
  const int mw = m0 + wm * MT * 16;
  const int nw = n0 + wn * NT * 16;
  if (EPI == kMx4pgSilu) {
    const int half_n = N >> 1;
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int j = 0; j < NT; j += 2) {
        const int col = ((nw + 16 * j) >> 1) + l15;  // pair (gate tile, up tile) -> 16 outputs
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          const int m = mw + 16 * i + 4 * g + rr;
          if (m < M && col < half_n) {
            const float gv = acc[i][j][rr], uv = acc[i][j + 1][rr];
            out[(size_t)m * out_stride + col] = f32_to_bf16(gv / (1.f + __expf(-gv)) * uv);
          }
        }
      }
  } else {
    float* slab = ws + (size_t)s * M * N;
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const int n = nw + 16 * j + l15;
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          const int m = mw + 16 * i + 4 * g + rr;
          if (m < M && n < N) {
            if (EPI == kMx4pgSlab)
              slab[(size_t)m * N + n] = acc[i][j][rr];
            else
              out[(size_t)m * out_stride + n] = f32_to_bf16(acc[i][j][rr]);
          }
        }
      }
  }
}

}  // namespace ft

// cfg: 0 = 128 x 256 tile (2 x 4 waves of 64 x 64, 3 LDS slots of 49 KiB = 147 KiB).
// epi: 0 bf16 out (one split), 1 fp32 slabs ws[splits][M][N] (any split count,
// ws_floats elements), 2 SiLU-mul of the 16-row interleaved gate/up image (one split,
// out [M, N / 2]).  Requirements (checked before any launch): N % 16 == 0 (N % 32 for
// SiLU), K % (128 * splits) == 0.
extern "C" int ft_mx4_packed_gemm(const void* x, int x_stride, int M, const uint8_t* wq,
                                  const uint8_t* sc, int N, int K, int splits, int epi, int cfg,
                                  void* out, int out_stride, float* ws, long ws_floats,
                                  hipStream_t stream) {
  if (M <= 0) return 0;
  if (N <= 0 || N % 16 != 0 || (epi == 2 && N % 32 != 0)) return -2;
  if (splits < 1 || K <= 0 || K % (128 * splits) != 0) return -3;
  if (epi < 0 || epi > 2) return -4;
  if (epi == 1 ? ws == nullptr : (splits != 1 || out == nullptr)) return -4;
  if (cfg != 0) return -5;
  if (epi == 1 && ws_floats < (long)splits * M * N) return -8;
  const int k_slice = K / splits;
  const int bm = 128, bn = 256;
  const int tiles = ((M + bm - 1) / bm) * ((N + bn - 1) / bn);
  dim3 grid(tiles, splits), block(512);
#define FT_MX4PG(E_)                                                                            \
  hipLaunchKernelGGL((ft::mx4_packed_gemm_kernel<2, 4, 4, 4, 3, E_>), grid, block, 0, stream,   \
                     (const uint16_t*)x, x_stride, M, wq, sc, N, K, k_slice, (uint16_t*)out,    \
                     out_stride, ws)
  if (epi == 0)
    FT_MX4PG(ft::kMx4pgStore);
  else if (epi == 1)
    FT_MX4PG(ft::kMx4pgSlab);
  else
    FT_MX4PG(ft::kMx4pgSilu);
#undef FT_MX4PG
  return static_cast<int>(hipGetLastError());
}
