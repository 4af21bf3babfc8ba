// W8A16 above the decode row counts: y[M, N] = s[n] * (x[M, K] . q[N, K]^T) for any M
// (the model uses it for M > 64: prefill chunks, mixed steps, large decode batches) on
// the SAME fp8 image the decode kernel streams (w8a16.hip, ops.quant.pack_w8:
// wq [N/16][K/64][lane][16 B], scale fp32 [N]), so an fp8 model keeps no bf16 copy of
// its projections.
//
// w4_packed_gemm.hip without everything int4 (no zero points, no per-group fold, no
// ones-MFMAs), with a K-stage of one 64-wide k-step:
//   * W: one (16-column tile, k-step) block is 1 KiB contiguous in the image, so one
//     global_load_lds_dwordx4 per tile brings the stage; lane l reads back its 16 B at
//     l * 16 and fp8x8_to_bf16 (v_cvt_scalef32_pk_bf16_fp8, scale 1; every e4m3 value is
//     exact in bf16) widens them to the two bf16 B fragments of the k-step, once per
//     stage for the wave's MT row tiles;
//   * x: the stage is one 64-k image [BM][64] with packed_gemm.hip's swizzle (16-B
//     chunk c of local row r at slot c ^ ((r >> 1) & 5), applied on the per-lane
//     SOURCE address), 8 rows x 128 B per DMA instruction;
//   * an S-slot ring, S - 2 stages in flight across the one raw s_barrier per stage,
//     counted vmcnt (every wave issues the same number of DMA instructions per
//     stage), no __syncthreads in the loop;
//   * tile order, XCD remap and split-K over gridDim.y are packed_gemm.hip's.
// Numerics are the decode kernel's: bf16 MFMAs on the exact q into fp32, the channel
// scale applied once to the fp32 accumulator in the epilogue (to every slab under
// split-K), then one rounding; rows above and below 64 see the same weights.
// Rows and column tiles past the end are clamped on load (nothing outside x or the
// image is read) and masked on store; the scale vector is read under the same mask.
// Plain vector stores only; fixed waits and barriers only.
#include "ft_common.h"
#include "ft_lds.h"

namespace ft {

typedef __bf16 w8pg_bf16x8 __attribute__((ext_vector_type(8)));
typedef float w8pg_floatx4 __attribute__((ext_vector_type(4)));

enum W8pgEpi { kW8pgStore = 0, kW8pgSlab = 1, kW8pgSilu = 2 };

__device__ __forceinline__ w8pg_bf16x8 w8pg_frag(const uint4& v) {
  return __builtin_bit_cast(w8pg_bf16x8, v);
}

template <int PW, int S>
__device__ __forceinline__ void w8pg_wait_ahead(int ahead) {
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
__global__ __launch_bounds__(512, 1) void w8_packed_gemm_kernel(
    const uint16_t* __restrict__ x, int x_stride, int M, const uint8_t* __restrict__ wq,
    const float* __restrict__ scale, int N, int K, int k_slice, uint16_t* __restrict__ out,
    int out_stride, float* __restrict__ ws) {
  constexpr int NW = WM * WN;
  static_assert(NW == 8, "8 waves");
  constexpr int BM = WM * MT * 16, BN = WN * NT * 16;
  constexpr int A_BYTES = BM * 128;           // [BM][64] bf16
  constexpr int B_BYTES = BN * 64;            // BN / 16 KiB
  constexpr int STAGE = A_BYTES + B_BYTES;
  constexpr int A_INST = BM / 8;              // 8 rows per DMA instruction
  constexpr int B_INST = BN / 16;             // one per column tile
  static_assert(A_INST % NW == 0 && B_INST % NW == 0, "uniform DMA counts");
  constexpr int A_PW = A_INST / NW, B_PW = B_INST / NW;
  constexpr int PW = A_PW + B_PW;
  static_assert(2 * PW < 64, "vmcnt field");
  static_assert(S >= 2 && S <= 4 && S * STAGE <= 160 * 1024, "LDS");
  static_assert(EPI != kW8pgSilu || NT % 2 == 0, "SiLU pairs need an even NT");
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
  const int nk = k_slice >> 6;                // k-steps of this split
  const int steps_total = K >> 6;
  const int step0 = kbeg >> 6;
  const int ntiles_all = N >> 4;

  const uint32_t lds0 = lds_off(smem);

  // per-lane DMA sources (k-step 0 of this split); a stage advances x by 64 elements and
  // W by one 1 KiB block.  Rows and column tiles past the end are clamped to the last one.
  const uint16_t* a_src[A_PW];
#pragma unroll
  for (int i = 0; i < A_PW; ++i) {
    const int rb = i * NW + w;                // LDS destination rb * 1024
    const int rl = rb * 8 + (lane >> 3);
    const int c = (lane & 7) ^ ((rl >> 1) & 5);
    const int row = min(m0 + rl, M - 1);
    a_src[i] = x + (size_t)row * x_stride + kbeg + c * 8;
  }
  const uint8_t* b_src[B_PW];
#pragma unroll
  for (int i = 0; i < B_PW; ++i) {
    const int nt = min((n0 >> 4) + i * NW + w, ntiles_all - 1);
    b_src[i] = wq + ((size_t)nt * steps_total + step0) * 1024 + lane * 16;
  }

  auto issue = [&](int t) {
    const uint32_t base = lds0 + (t % S) * STAGE;
#pragma unroll
    for (int i = 0; i < A_PW; ++i) glds16(a_src[i] + t * 64, base + (i * NW + w) * 1024);
#pragma unroll
    for (int i = 0; i < B_PW; ++i)
      glds16(b_src[i] + (size_t)t * 1024, base + A_BYTES + (i * NW + w) * 1024);
  };

  w8pg_floatx4 acc[MT][NT];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[i][j] = w8pg_floatx4{0.f, 0.f, 0.f, 0.f};

  // fragment read offsets inside a stage
  uint32_t a_off[MT][2];
#pragma unroll
  for (int i = 0; i < MT; ++i) {
    const int rl = wm * MT * 16 + i * 16 + l15;
#pragma unroll
    for (int h = 0; h < 2; ++h) a_off[i][h] = rl * 128 + (((2 * g + h) ^ ((rl >> 1) & 5)) * 16);
  }
  const uint32_t b_off = A_BYTES + (wn * NT) * 1024 + lane * 16;

#pragma unroll
  for (int t = 0; t < S - 1; ++t)
    if (t < nk) issue(t);

  for (int t = 0; t < nk; ++t) {
    // stage t landed (own DMAs), and every wave is done reading stage t-1's slot
    w8pg_wait_ahead<PW, S>(min(S - 2, nk - 1 - t));
    lgkm_wait<0>();
    __builtin_amdgcn_s_barrier();
    if (t + S - 1 < nk) issue(t + S - 1);
    const uint32_t base = lds0 + (t % S) * STAGE;
    uint4 bw[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) bw[j] = ds_read16(base + b_off + j * 1024);
    uint4 af[2][2];
#pragma unroll
    for (int h = 0; h < 2; ++h) af[0][h] = ds_read16(base + a_off[0][h]);
    lgkm_wait<2>();   // the weight bytes (LDS returns in order)
    uint4 bf[NT][2];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      dep(bw[j]);
      bf[j][0] = fp8x8_to_bf16(bw[j].x, bw[j].y);
      bf[j][1] = fp8x8_to_bf16(bw[j].z, bw[j].w);
    }
#pragma unroll
    for (int i = 0; i < MT; ++i) {
      const int cur = i & 1;
      if (i + 1 < MT) {
#pragma unroll
        for (int h = 0; h < 2; ++h) af[cur ^ 1][h] = ds_read16(base + a_off[i + 1][h]);
        lgkm_wait<2>();
      } else {
        lgkm_wait<0>();
      }
#pragma unroll
      for (int h = 0; h < 2; ++h) dep(af[cur][h]);
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int j = 0; j < NT; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w8pg_frag(af[cur][h]),
                                                              w8pg_frag(bf[j][h]), acc[i][j], 0, 0, 0);
      __builtin_amdgcn_s_setprio(0);
    }
  }

  // epilogue: C layout, lane (g, l15) holds rows 4g..4g+3 of column l15
  const int mw = m0 + wm * MT * 16;
  const int nw = n0 + wn * NT * 16;
  float sc[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int n = nw + 16 * j + l15;
    sc[j] = n < N ? scale[n] : 0.f;
  }
  if (EPI == kW8pgSilu) {
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
            const float gv = acc[i][j][rr] * sc[j], uv = acc[i][j + 1][rr] * sc[j + 1];
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
            const float v = acc[i][j][rr] * sc[j];
            if (EPI == kW8pgSlab)
              slab[(size_t)m * N + n] = v;
            else
              out[(size_t)m * out_stride + n] = f32_to_bf16(v);
          }
        }
      }
  }
}

}  // namespace ft

// cfg: 0 = 128 x 256 tile (2 x 4 waves of 64 x 64, 4 LDS slots of 32 KiB).
// epi: 0 bf16 out (one split), 1 fp32 slabs ws[splits][M][N] (any split count,
// ws_floats elements), 2 SiLU-mul of the 16-row interleaved gate/up image (one split,
// out [M, N / 2]).  Requirements (checked before any launch): N % 16 == 0 (N % 32 for
// SiLU), K % (64 * splits) == 0.
extern "C" int ft_w8_packed_gemm(const void* x, int x_stride, int M, const uint8_t* wq,
                                 const float* scale, int N, int K, int splits, int epi, int cfg,
                                 void* out, int out_stride, float* ws, long ws_floats,
                                 hipStream_t stream) {
  if (M <= 0) return 0;
  if (N <= 0 || N % 16 != 0 || (epi == 2 && N % 32 != 0)) return -2;
  if (splits < 1 || K <= 0 || K % (64 * splits) != 0) return -3;
  if (epi < 0 || epi > 2) return -4;
  if (epi == 1 ? ws == nullptr : (splits != 1 || out == nullptr)) return -4;
  if (cfg != 0) return -5;
  if (epi == 1 && ws_floats < (long)splits * M * N) return -8;
  const int k_slice = K / splits;
  const int bm = 128, bn = 256;
  const int tiles = ((M + bm - 1) / bm) * ((N + bn - 1) / bn);
  dim3 grid(tiles, splits), block(512);
#define FT_W8PG(E_)                                                                            \
  hipLaunchKernelGGL((ft::w8_packed_gemm_kernel<2, 4, 4, 4, 4, E_>), grid, block, 0, stream,   \
                     (const uint16_t*)x, x_stride, M, wq, scale, N, K, k_slice, (uint16_t*)out, \
                     out_stride, ws)
  if (epi == 0)
    FT_W8PG(ft::kW8pgStore);
  else if (epi == 1)
    FT_W8PG(ft::kW8pgSlab);
  else
    FT_W8PG(ft::kW8pgSilu);
#undef FT_W8PG
  return static_cast<int>(hipGetLastError());
}
