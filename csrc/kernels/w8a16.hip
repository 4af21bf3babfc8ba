// W8A16 decode GEMM (1..64 rows): fp8 e4m3 (OCP) weights with one fp32 scale per output
// channel, the format of vLLM's --quantization fp8 and AMD Quark FP8 checkpoints.
//   y[m, n] = s[n] * sum_k x[m, k] * q[n, k]
// q is widened to bf16 (every e4m3 value is exact in bf16) right before its MFMAs,
// the products run on v_mfma_f32_16x16x32_bf16 with fp32 accumulation, and the scale
// is applied ONCE to the fp32 accumulator in the epilogue (to each slab under split-K:
// the sum over slabs is linear, so the consumers in fused_epilogue.hip stay as they
// are).  No per-weight multiply, no bf16-rounded q * s: rows below and above 64
// (w8_packed_gemm.hip) see identical weights.
//
// One kernel form, skinny_gemm.hip's "xr" on the fp8 image (ops.quant.pack_w8:
// [N/16][K/64][lane][16 B], byte 8 * half + e of lane (g, r) = k 64 step + 16 g +
// 8 half + e of column 16 tile + r):
//   * x is staged per KC-wide K chunk in LDS once per workgroup (double-buffered, one
//     barrier per chunk, the xr swizzle);
//   * each wave streams NT column tiles: one non-temporal 16-byte load per lane is a
//     whole 64-wide k-step (1 KiB of consecutive bytes per wave instruction), held in a
//     register ring of one chunk (KS x NT x 16 B per lane) whose slots are refilled
//     with the next chunk's fragment right after they are widened;
//   * fp8x8_to_bf16 (v_cvt_scalef32_pk_bf16_fp8, scale 1) widens a slot to the two bf16
//     B fragments of its k-step once, for all MT row tiles;
//   * split-K over gridDim.y; KC is 512 when the K slice allows it, else 256.
// Epilogues: bf16 store (ws == nullptr), fp32 slabs ws[s][m][n], or EPI 1: SiLU * up of a
// gate/up image interleaved in 16-row groups (NT = 2: a gate tile and its up tile).
// Tails: rows >= M are clamped on load and never stored; a wave's column tiles past
// N / 16 are clamped to the last tile (image and scale reads stay inside) and their
// duplicate work is discarded.
#include "ft_common.h"

#include <type_traits>

namespace ft {

typedef __bf16 w8_bf16x8 __attribute__((ext_vector_type(8)));
typedef float w8_floatx4 __attribute__((ext_vector_type(4)));
typedef unsigned int w8_u32x4 __attribute__((ext_vector_type(4)));

template <int MT, int NT, int KC, int EPI>
__global__ __launch_bounds__(256, 1) void w8_xr_kernel(
    const uint16_t* __restrict__ x, int x_stride, int M, const uint8_t* __restrict__ wq,
    const float* __restrict__ scale, int K, float* __restrict__ ws, uint16_t* __restrict__ out,
    int out_stride, int N, int k_slice) {
  constexpr bool SILU = EPI == 1;
  constexpr int KS = KC / 64;
  constexpr int ROWS = 16 * MT;
  constexpr int CPR = KC / 8;                // 16-B x pieces per row per chunk
  constexpr int XL = ROWS * CPR / 256;
  static_assert(XL >= 1 && (ROWS * CPR) % 256 == 0, "x chunk must tile the workgroup");
  static_assert(!SILU || NT == 2, "the SiLU epilogue pairs a gate tile with its up tile");
  __shared__ __attribute__((aligned(16))) uint16_t s_x[2][ROWS * KC];
  const int tid = threadIdx.x;
  const int lane = lane_id(), wave = wave_id();
  const int l15 = lane & 15, g = lane >> 4;
  const int ntiles = N >> 4;
  const int t0 = (blockIdx.x * 4 + wave) * NT;   // first 16-column tile of this wave
  const int s = blockIdx.y;
  const int kbeg = s * k_slice;
  const int nch = k_slice / KC;

  const uint8_t* wp[NT];
  float sc[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int tile = min(t0 + j, ntiles - 1);
    wp[j] = wq + ((size_t)tile * (K >> 6) + (kbeg >> 6)) * 1024 + lane * 16;
    sc[j] = scale[tile * 16 + l15];
  }
  // this thread's x pieces: row e / CPR, 16-B piece e % CPR of each chunk, e = tid + 256 p
  const uint16_t* xsrc[XL];
#pragma unroll
  for (int p = 0; p < XL; ++p) {
    const int e = tid + 256 * p;
    xsrc[p] = x + (size_t)min(e / CPR, M - 1) * x_stride + kbeg + (e % CPR) * 8;
  }

  w8_floatx4 acc[MT][NT];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[i][j] = w8_floatx4{0.f, 0.f, 0.f, 0.f};

  w8_u32x4 xr[XL];
  w8_u32x4 wr[KS][NT];
#pragma unroll
  for (int p = 0; p < XL; ++p) xr[p] = *reinterpret_cast<const w8_u32x4*>(xsrc[p]);
#pragma unroll
  for (int st = 0; st < KS; ++st)
#pragma unroll
    for (int j = 0; j < NT; ++j)
      wr[st][j] = __builtin_nontemporal_load(reinterpret_cast<const w8_u32x4*>(wp[j] + (size_t)st * 1024));

  // one chunk: x regs -> LDS buffer c & 1, next chunk's x loads, barrier, then per k-step
  // widen + refill + MFMAs.  MORE is a template constant (the last chunk is peeled) so
  // the loop body is branch-free, as in skinny_xr_kernel.
  auto chunk = [&](int c, auto more_tag) {
    constexpr bool MORE = decltype(more_tag)::value;
    uint16_t* sx = s_x[c & 1];
#pragma unroll
    for (int p = 0; p < XL; ++p) {
      const int e = tid + 256 * p;
      const int row = e / CPR, ch = e % CPR;
      const int slot = (ch & ~7) | ((ch & 7) ^ (row & 7));
      *reinterpret_cast<w8_u32x4*>(&sx[row * KC + slot * 8]) = xr[p];
    }
    if constexpr (MORE) {
#pragma unroll
      for (int p = 0; p < XL; ++p) xr[p] = *reinterpret_cast<const w8_u32x4*>(xsrc[p] + (c + 1) * KC);
    }
    __syncthreads();   // chunk c visible; every wave is past chunk c-1's reads of the other buffer
    const size_t nxt = (size_t)(c + 1) * KS * 1024;
#pragma unroll
    for (int st = 0; st < KS; ++st) {
      w8_bf16x8 wf[NT][2];
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        wf[j][0] = __builtin_bit_cast(w8_bf16x8, fp8x8_to_bf16(wr[st][j][0], wr[st][j][1]));
        wf[j][1] = __builtin_bit_cast(w8_bf16x8, fp8x8_to_bf16(wr[st][j][2], wr[st][j][3]));
      }
      if constexpr (MORE) {   // refill this k-step's registers with the next chunk's fragment
#pragma unroll
        for (int j = 0; j < NT; ++j)
          wr[st][j] = __builtin_nontemporal_load(
              reinterpret_cast<const w8_u32x4*>(wp[j] + nxt + (size_t)st * 1024));
      }
#pragma unroll
      for (int i = 0; i < MT; ++i) {
        const int row = 16 * i + l15;
        w8_u32x4 xf[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int ch = st * 8 + 2 * g + h;
          const int slot = (ch & ~7) | ((ch & 7) ^ (row & 7));
          xf[h] = *reinterpret_cast<const w8_u32x4*>(&sx[row * KC + slot * 8]);
        }
#pragma unroll
        for (int j = 0; j < NT; ++j) {
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(w8_bf16x8, xf[0]),
                                                              wf[j][0], acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(w8_bf16x8, xf[1]),
                                                              wf[j][1], acc[i][j], 0, 0, 0);
        }
      }
    }
  };
  for (int c = 0; c + 1 < nch; ++c) chunk(c, std::true_type{});
  chunk(nch - 1, std::false_type{});
  if (t0 >= ntiles) return;
  if constexpr (SILU) {
    const int col = ((t0 * 16) >> 1) + l15;   // (gate tile, up tile) -> 16 h columns
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = 16 * i + g * 4 + r;
        if (m < M) {
          const float gt = acc[i][0][r] * sc[0], up = acc[i][1][r] * sc[1];
          out[(size_t)m * out_stride + col] = f32_to_bf16(gt / (1.f + __expf(-gt)) * up);
        }
      }
    return;
  }
  float* slab = ws + (size_t)s * M * N;
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = 16 * i + g * 4 + r;
      if (m < M) {
#pragma unroll
        for (int j = 0; j < NT; ++j) {
          if (t0 + j < ntiles) {
            const int n = (t0 + j) * 16 + l15;
            const float v = acc[i][j][r] * sc[j];
            if (ws == nullptr)
              out[(size_t)m * out_stride + n] = f32_to_bf16(v);
            else
              slab[(size_t)m * N + n] = v;
          }
        }
      }
    }
}

}  // namespace ft

// Requirements (checked before any launch): 1 <= M <= 64, N % 16 == 0, K % (256 *
// splits) == 0, nt in {1, 2, 4}; ws (fp32 [splits][M][N] slabs, ws_floats elements) is
// required for splits > 1 and selects slab output; silu: nt == 2, N % 32 == 0, one
// split, no workspace, out [M, N / 2].
extern "C" int ft_w8_gemm(const void* x, int x_stride, int M, const uint8_t* wq, const float* scale,
                          int N, int K, float* ws, long ws_floats, void* out, int out_stride,
                          int splits, int nt, int silu, hipStream_t stream) {
  if (M <= 0) return 0;
  if (M > 64 || splits < 1) return -1;
  if (N <= 0 || N % 16 != 0 || (silu && N % 32 != 0)) return -2;
  if (K <= 0 || K % (256 * splits) != 0) return -3;
  if (splits > 1 && (ws == nullptr || silu)) return -4;
  if (nt != 1 && nt != 2 && nt != 4) return -5;
  if (ws == nullptr && out == nullptr) return -6;
  if (silu && (nt != 2 || ws != nullptr)) return -7;
  if (ws != nullptr && ws_floats < (long)splits * M * N) return -8;
  const int mt = (M + 15) / 16;
  const int ntiles = N / 16;
  dim3 grid((ntiles + 4 * nt - 1) / (4 * nt), splits), block(256);
  const int k_slice = K / splits;
  const int kc = k_slice % 512 == 0 ? 512 : 256;
#define FT_W8(MT_, NT_, KC_, E_)                                                             \
  if (mt == MT_ && nt == NT_ && kc == KC_ && silu == E_) {                                   \
    hipLaunchKernelGGL((ft::w8_xr_kernel<MT_, NT_, KC_, E_>), grid, block, 0, stream,        \
                       (const uint16_t*)x, x_stride, M, wq, scale, K, ws, (uint16_t*)out,    \
                       out_stride, N, k_slice);                                              \
    return static_cast<int>(hipGetLastError());                                              \
  }
#define FT_W8_M(NT_, KC_, E_) \
  FT_W8(1, NT_, KC_, E_) FT_W8(2, NT_, KC_, E_) FT_W8(3, NT_, KC_, E_) FT_W8(4, NT_, KC_, E_)
  silu = silu ? 1 : 0;
  FT_W8_M(1, 256, 0) FT_W8_M(2, 256, 0) FT_W8_M(4, 256, 0) FT_W8_M(2, 256, 1)
  FT_W8_M(1, 512, 0) FT_W8_M(2, 512, 0) FT_W8_M(4, 512, 0) FT_W8_M(2, 512, 1)
#undef FT_W8_M
#undef FT_W8
  return -5;
}
