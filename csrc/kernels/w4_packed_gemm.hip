// W4A16 above the decode row counts: y[M, N] = x[M, K] . dequant(W)[N, K]^T for any
// M (the model uses it for M > 64: prefill chunks, mixed steps, large decode
// batches) on the SAME int4 image the decode kernels stream (w4a16.hip,
// ops.quant.pack_w4: wq [N/16][K/128][lane][4 x u32], sz [N/16][K/128][16][2] fp32),
// so a W4 model needs no dequantized bf16 copy of its projections for prefill.
//
// Tiling: packed_gemm.hip's workgroup tile (8 waves as WM x WN, each MT x NT 16x16
// tiles, v_mfma_f32_16x16x32_bf16) with a K-stage of one 128-wide quantization group:
//   * W: one (16-column tile, group) block is 1 KiB contiguous in the image, so one
//     global_load_lds_dwordx4 per tile brings the whole group; lane l reads its 16 B
//     at l * 16 (word 2 * step + half holds k = 128 grp + 64 step + 16 g + 8 half +
//     ...) and ((w >> 4i) & 0x000F000F) | 0x43004300 -- one v_and_or_b32 per output
//     word, constants in VGPRs -- is the bf16 B fragment (128 + q) of k-step `step`,
//     half `half`, dequantized once per stage and reused for the wave's MT row tiles;
//   * the group's (scale, 128 + zero) pairs: 128 B per column tile, eight tiles per
//     DMA instruction, read back as one ds_read_b64 per column tile;
//   * x: the stage is two 64-k images [BM][64] with packed_gemm.hip's swizzle (16-B
//     chunk c of local row r at slot c ^ ((r >> 1) & 5), applied on the per-lane
//     SOURCE address), 8 rows x 128 B per DMA instruction;
//   * an S-slot ring, S - 2 stages in flight across the one raw s_barrier per stage,
//     counted vmcnt (every wave issues the same number of DMA instructions per
//     stage), no __syncthreads in the loop;
//   * tile order, XCD remap, split-K over gridDim.y and the three epilogues are
//     packed_gemm.hip's.
// Numerics are the decode kernels' (w4_skinny_kernel): per group the MFMAs run on
// the exact bf16 values 128 + q into a fresh fp32 accumulator, then
//   acc += s * (part - (128 + z) * xsum),   xsum = the row's sum of x over the group,
// so rows above and below 64 see the same weights (q - z) * s; no bf16-rounded
// dequantized fragment is ever formed.
// xsum: ones-MFMAs per row tile and group in every wave, as w4_skinny_kernel does
// (the result lands in the C layout the fold needs, no LDS hand-off and no second
// barrier); this costs 1/NT extra MFMAs (25% at NT = 4).  Sharing them among the WN
// waves of one wm through LDS is the follow-up if the probe shows the MFMA pipe as
// the limit.
// Plain vector stores only; fixed waits and barriers only.
#include "ft_common.h"
#include "ft_lds.h"

namespace ft {

typedef __bf16 w4pg_bf16x8 __attribute__((ext_vector_type(8)));
typedef float w4pg_floatx4 __attribute__((ext_vector_type(4)));

enum W4pgEpi { kW4pgStore = 0, kW4pgSlab = 1, kW4pgSilu = 2 };

__device__ __forceinline__ w4pg_bf16x8 w4pg_frag(const uint4& v) {
  return __builtin_bit_cast(w4pg_bf16x8, v);
}

// one packed u32 (8 nibbles) -> the 8 bf16 values 128 + q of an MFMA B fragment, mask
// and bias in VGPRs (one v_and_or_b32 per output word, see w4a16.hip w4_frag_r)
__device__ __forceinline__ uint4 w4pg_deq(uint32_t w, uint32_t vm, uint32_t vc) {
  uint4 r;
  r.x = (w & vm) | vc;
  r.y = ((w >> 4) & vm) | vc;
  r.z = ((w >> 8) & vm) | vc;
  r.w = ((w >> 12) & vm) | vc;
  return r;
}

template <int PW, int S>
__device__ __forceinline__ void w4pg_wait_ahead(int ahead) {
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
__global__ __launch_bounds__(512, 1) void w4_packed_gemm_kernel(
    const uint16_t* __restrict__ x, int x_stride, int M, const uint32_t* __restrict__ wq,
    const float* __restrict__ sz, int N, int K, int k_slice, uint16_t* __restrict__ out,
    int out_stride, float* __restrict__ ws) {
  constexpr int NW = WM * WN;
  static_assert(NW == 8, "8 waves");
  constexpr int BM = WM * MT * 16, BN = WN * NT * 16;
  static_assert(BN % 128 == 0, "scale DMA instructions cover 8 column tiles");
  constexpr int A_HALF = BM * 128;            // one 64-k image of the stage
  constexpr int A_BYTES = 2 * A_HALF;
  constexpr int B_BYTES = BN * 64;            // BN / 16 KiB
  constexpr int Z_BYTES = BN * 8;             // 128 B per column tile
  constexpr int STAGE = A_BYTES + B_BYTES + Z_BYTES;
  constexpr int A_PW = 2 * BM / (8 * NW);     // x DMA instructions per wave per stage
  constexpr int B_INST = BN / 16;             // one per column tile
  static_assert(B_INST % NW == 0 && (2 * BM / 8) % NW == 0, "uniform DMA counts");
  constexpr int B_PW = B_INST / NW;
  constexpr int Z_INST = BN / 128;
  constexpr int PW = A_PW + B_PW + 1;         // + one scale instruction
  static_assert(2 * PW < 64, "vmcnt field");
  static_assert(S >= 2 && S * STAGE <= 160 * 1024, "LDS");
  static_assert(EPI != kW4pgSilu || NT % 2 == 0, "SiLU pairs need an even NT");
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
  const int nk = k_slice >> 7;                // groups of this split
  const int groups_total = K >> 7;
  const int grp0 = kbeg >> 7;
  const int ntiles_all = N >> 4;

  const uint32_t lds0 = lds_off(smem);

  // per-lane DMA sources (group 0 of this split); a stage advances x by 128 elements,
  // W by one 1 KiB block, the scales by one 128-B record.  Rows and column tiles past
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
  const uint32_t* b_src[B_PW];
#pragma unroll
  for (int i = 0; i < B_PW; ++i) {
    const int nt = min((n0 >> 4) + i * NW + w, ntiles_all - 1);
    b_src[i] = wq + ((size_t)nt * groups_total + grp0) * 256 + lane * 4;
  }
  // every wave issues one scale instruction (waves past Z_INST repeat one: the same
  // bytes to the same place), so the counted vmcnt waits are uniform
  const int z_inst = w % Z_INST;
  const float* z_src;
  {
    const int nt = min((n0 >> 4) + z_inst * 8 + (lane >> 3), ntiles_all - 1);
    z_src = sz + ((size_t)nt * groups_total + grp0) * 32 + (lane & 7) * 4;
  }

  auto issue = [&](int t) {
    const uint32_t base = lds0 + (t % S) * STAGE;
#pragma unroll
    for (int i = 0; i < A_PW; ++i) glds16(a_src[i] + t * 128, base + (i * NW + w) * 1024);
#pragma unroll
    for (int i = 0; i < B_PW; ++i)
      glds16(b_src[i] + (size_t)t * 256, base + A_BYTES + (i * NW + w) * 1024);
    glds16(z_src + (size_t)t * 32, base + A_BYTES + B_BYTES + z_inst * 1024);
  };

  w4pg_floatx4 acc[MT][NT];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[i][j] = w4pg_floatx4{0.f, 0.f, 0.f, 0.f};

  // fragment read offsets inside a stage
  uint32_t a_off[MT][2];
#pragma unroll
  for (int i = 0; i < MT; ++i) {
    const int rl = wm * MT * 16 + i * 16 + l15;
#pragma unroll
    for (int h = 0; h < 2; ++h) a_off[i][h] = rl * 128 + (((2 * g + h) ^ ((rl >> 1) & 5)) * 16);
  }
  const uint32_t b_off = A_BYTES + (wn * NT) * 1024 + lane * 16;
  const uint32_t z_off = A_BYTES + B_BYTES + (wn * NT) * 128 + l15 * 8;

  const uint4 ones4 = make_uint4(0x3F803F80u, 0x3F803F80u, 0x3F803F80u, 0x3F803F80u);
  const w4pg_bf16x8 ones = w4pg_frag(ones4);
  uint32_t vmask = 0x000F000Fu, vbias = 0x43004300u;
  asm volatile("" : "+v"(vmask), "+v"(vbias));

#pragma unroll
  for (int t = 0; t < S - 1; ++t)
    if (t < nk) issue(t);

  for (int t = 0; t < nk; ++t) {
    // stage t landed (own DMAs), and every wave is done reading stage t-1's slot
    w4pg_wait_ahead<PW, S>(min(S - 2, nk - 1 - t));
    lgkm_wait<0>();
    __builtin_amdgcn_s_barrier();
    if (t + S - 1 < nk) issue(t + S - 1);
    const uint32_t base = lds0 + (t % S) * STAGE;
    uint4 bw[NT];
    uint2 zr[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      bw[j] = ds_read16(base + b_off + j * 1024);
      zr[j] = ds_read8(base + z_off + j * 128);
    }
    uint4 af[2][4];
#pragma unroll
    for (int h = 0; h < 4; ++h) af[0][h] = ds_read16(base + (h >> 1) * A_HALF + a_off[0][h & 1]);
    lgkm_wait<4>();   // the weight words and scales (LDS returns in order)
    uint4 bf[NT][4];
    float sc[NT], zz[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      dep(bw[j]);
      dep(zr[j]);
      bf[j][0] = w4pg_deq(bw[j].x, vmask, vbias);
      bf[j][1] = w4pg_deq(bw[j].y, vmask, vbias);
      bf[j][2] = w4pg_deq(bw[j].z, vmask, vbias);
      bf[j][3] = w4pg_deq(bw[j].w, vmask, vbias);
      sc[j] = __uint_as_float(zr[j].x);
      zz[j] = __uint_as_float(zr[j].y);
    }
#pragma unroll
    for (int i = 0; i < MT; ++i) {
      const int cur = i & 1;
      if (i + 1 < MT) {
#pragma unroll
        for (int h = 0; h < 4; ++h)
          af[cur ^ 1][h] = ds_read16(base + (h >> 1) * A_HALF + a_off[i + 1][h & 1]);
        lgkm_wait<4>();
      } else {
        lgkm_wait<0>();
      }
#pragma unroll
      for (int h = 0; h < 4; ++h) dep(af[cur][h]);
      w4pg_floatx4 xs = w4pg_floatx4{0.f, 0.f, 0.f, 0.f};
      w4pg_floatx4 part[NT];
#pragma unroll
      for (int j = 0; j < NT; ++j) part[j] = w4pg_floatx4{0.f, 0.f, 0.f, 0.f};
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int h = 0; h < 4; ++h) {
        xs = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w4pg_frag(af[cur][h]), ones, xs, 0, 0, 0);
#pragma unroll
        for (int j = 0; j < NT; ++j)
          part[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w4pg_frag(af[cur][h]),
                                                            w4pg_frag(bf[j][h]), part[j], 0, 0, 0);
      }
      __builtin_amdgcn_s_setprio(0);
#pragma unroll
      for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          acc[i][j][r] = fmaf(sc[j], fmaf(-zz[j], xs[r], part[j][r]), acc[i][j][r]);
    }
  }

  // epilogue: C layout, lane (g, l15) holds rows 4g..4g+3 of column l15
  const int mw = m0 + wm * MT * 16;
  const int nw = n0 + wn * NT * 16;
  if (EPI == kW4pgSilu) {
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
            if (EPI == kW4pgSlab)
              slab[(size_t)m * N + n] = acc[i][j][rr];
            else
              out[(size_t)m * out_stride + n] = f32_to_bf16(acc[i][j][rr]);
          }
        }
      }
  }
}

}  // namespace ft

// cfg: 0 = 128 x 256 tile (2 x 4 waves of 64 x 64, 3 LDS slots), 1 = 256 x 128 (4 x 2
// waves of 64 x 64, 2 slots), 2 = 128 x 128 (4 x 2 waves of 32 x 64, 3 slots).
// epi: 0 bf16 out (one split), 1 fp32 slabs ws[splits][M][N] (any split count),
// 2 SiLU-mul of the 16-row interleaved gate/up image (one split, out [M, N / 2]).
// Requirements (checked): N % 16 == 0 (N % 32 for SiLU), K % (128 * splits) == 0.
extern "C" int ft_w4_packed_gemm(const void* x, int x_stride, int M, const uint32_t* wq,
                                 const void* sz, int N, int K, int splits, int epi, int cfg,
                                 void* out, int out_stride, float* ws, hipStream_t stream) {
  if (M <= 0) return 0;
  if (N <= 0 || N % 16 != 0 || (epi == 2 && N % 32 != 0)) return -2;
  if (splits < 1 || K <= 0 || K % (128 * splits) != 0) return -3;
  if (epi < 0 || epi > 2) return -4;
  if (epi == 1 ? ws == nullptr : (splits != 1 || out == nullptr)) return -4;
  const int k_slice = K / splits;
  int bm, bn;
  switch (cfg) {
    case 0: bm = 128; bn = 256; break;
    case 1: bm = 256; bn = 128; break;
    case 2: bm = 128; bn = 128; break;
    default: return -5;
  }
  const int tiles = ((M + bm - 1) / bm) * ((N + bn - 1) / bn);
  dim3 grid(tiles, splits), block(512);
#define FT_W4PG(CFG, WM, WN, MT, NT, S)                                                        \
  if (cfg == CFG) {                                                                            \
    if (epi == 0)                                                                              \
      hipLaunchKernelGGL((ft::w4_packed_gemm_kernel<WM, WN, MT, NT, S, ft::kW4pgStore>), grid, \
                         block, 0, stream, (const uint16_t*)x, x_stride, M, wq,                \
                         (const float*)sz, N, K, k_slice, (uint16_t*)out, out_stride, ws);     \
    else if (epi == 1)                                                                         \
      hipLaunchKernelGGL((ft::w4_packed_gemm_kernel<WM, WN, MT, NT, S, ft::kW4pgSlab>), grid,  \
                         block, 0, stream, (const uint16_t*)x, x_stride, M, wq,                \
                         (const float*)sz, N, K, k_slice, (uint16_t*)out, out_stride, ws);     \
    else                                                                                       \
      hipLaunchKernelGGL((ft::w4_packed_gemm_kernel<WM, WN, MT, NT, S, ft::kW4pgSilu>), grid,  \
                         block, 0, stream, (const uint16_t*)x, x_stride, M, wq,                \
                         (const float*)sz, N, K, k_slice, (uint16_t*)out, out_stride, ws);     \
    return static_cast<int>(hipGetLastError());                                                \
  }
  FT_W4PG(0, 2, 4, 4, 4, 3)
  FT_W4PG(1, 4, 2, 4, 4, 2)
  FT_W4PG(2, 4, 2, 2, 4, 3)
#undef FT_W4PG
  return -5;
}
