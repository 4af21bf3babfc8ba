// MXFP4 (W4A16) decode GEMM, 1..64 rows: OCP MX e2m1 weights with one e8m0
// (power-of-two) scale per 32 k-values, the format of AMD Quark MXFP4 exports.
//   y[m, n] = sum_k x[m, k] * fp4(q[n, k]) * 2^(sb[n, k / 32] - 127)
// Every product fp4 * 2^e with a scale byte in [2, 252] is a finite normal bf16, so the
// weights are widened AND scaled in registers by v_cvt_scalef32_pk_bf16_fp4 (its scale
// operand is exact for powers of two) right before their MFMAs, the products run on
// v_mfma_f32_16x16x32_bf16 into fp32, and the accumulator IS the result: bit for bit a
// bf16 GEMM on the dequantized weights, no epilogue scale, no per-group fold.  Rows
// below and above 64 (mx4_packed_gemm.hip) see identical weights.
//
// THE IMAGE (ops.quant.pack_mx4; part of the contract):
//   wq uint8 [N/16][K/128][lane][16 B].  Lane (g = lane >> 4, r = lane & 15) of k-step
//   st of column tile t holds column 16 t + r and k = 128 st + 32 g + 0..31: exactly MX
//   block 4 st + g of that column, so a lane needs ONE scale per 16-byte load.  Dword j
//   of the 16 bytes is the B fragment of the step's j-th 16x16x32 MFMA: element e (0..7)
//   is k = 128 st + 32 g + 8 j + e and sits in nibble e of the dword, the LOW nibble of
//   byte e / 2 first (the converter's byte_sel b yields elements 2 b, 2 b + 1 from the
//   low, high nibble of byte b; tests/test_mx4_gemm_gpu.py recovers every weight
//   through the kernel to pin this).  The x fragment of that MFMA is the 16-byte piece
//   16 st + 4 g + j of the row (any k-permutation inside an MFMA is legal as long as A
//   and B agree).
//   sc uint8 [N/16][K/128][64]: the lane's scale byte, 64 consecutive bytes per wave load.
//   A gate_up image is interleaved in 16-row groups with its scale rows.
//
// One kernel form, w8a16.hip's "xr":
//   * x is staged per KC-wide K chunk in LDS once per workgroup (double-buffered, one
//     barrier per chunk, the xr swizzle; a 16-lane read group has one g, so the conflict
//     pattern is w8a16.hip's);
//   * each wave streams NT column tiles: one non-temporal 16-byte load per lane is a
//     whole 128-wide k-step, held with its scale byte in a register ring of one chunk
//     (KS x NT slots) whose slots are refilled with the next chunk's fragment right
//     after they are widened, so no convert waits on a fresh load;
//   * 16 converts widen a slot to the four bf16 B fragments of its k-step once, for all
//     MT row tiles;
//   * split-K over gridDim.y; KC is 512 (4 slots) when the K slice allows it, else 256.
// Epilogues: bf16 store (ws == nullptr), fp32 slabs ws[s][m][n], or EPI 1: SiLU * up of a
// gate/up image interleaved in 16-row groups (NT = 2: a gate tile and its up tile).
// Tails: rows >= M are clamped on load and never stored; a wave's column tiles past
// N / 16 are clamped to the last tile (image and scale reads stay inside) and their
// duplicate work is discarded.  Plain vector stores only.
#include "ft_common.h"

#include <type_traits>

namespace ft {

typedef __bf16 mx4_bf16x8 __attribute__((ext_vector_type(8)));
typedef float mx4_floatx4 __attribute__((ext_vector_type(4)));
typedef unsigned int mx4_u32x4 __attribute__((ext_vector_type(4)));

// one dword (8 e2m1 nibbles, low nibble of byte 0 first) times 2^(byte - 127) -> the 8
// bf16 of an MFMA B fragment
__device__ __forceinline__ mx4_bf16x8 mx4_widen(uint32_t w, float scale) {
  const ft_bf16x2_t a = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 0);
  const ft_bf16x2_t b = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 1);
  const ft_bf16x2_t c = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 2);
  const ft_bf16x2_t d = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 3);
  mx4_u32x4 r = {__builtin_bit_cast(uint32_t, a), __builtin_bit_cast(uint32_t, b),
                 __builtin_bit_cast(uint32_t, c), __builtin_bit_cast(uint32_t, d)};
  return __builtin_bit_cast(mx4_bf16x8, r);
}

template <int MT, int NT, int KC, int EPI>
__global__ __launch_bounds__(256, 1) void mx4_xr_kernel(
    const uint16_t* __restrict__ x, int x_stride, int M, const uint8_t* __restrict__ wq,
    const uint8_t* __restrict__ sc, int K, float* __restrict__ ws, uint16_t* __restrict__ out,
    int out_stride, int N, int k_slice) {
  constexpr bool SILU = EPI == 1;
  constexpr int KS = KC / 128;
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
  const uint8_t* sp[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int tile = min(t0 + j, ntiles - 1);
    const size_t blk = (size_t)tile * (K >> 7) + (kbeg >> 7);
    wp[j] = wq + blk * 1024 + lane * 16;
    sp[j] = sc + blk * 64 + lane;
  }
  // this thread's x pieces: row e / CPR, 16-B piece e % CPR of each chunk, e = tid + 256 p
  const uint16_t* xsrc[XL];
#pragma unroll
  for (int p = 0; p < XL; ++p) {
    const int e = tid + 256 * p;
    xsrc[p] = x + (size_t)min(e / CPR, M - 1) * x_stride + kbeg + (e % CPR) * 8;
  }

  mx4_floatx4 acc[MT][NT];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[i][j] = mx4_floatx4{0.f, 0.f, 0.f, 0.f};

  mx4_u32x4 xr[XL];
  mx4_u32x4 wr[KS][NT];
  uint32_t sr[KS][NT];
#pragma unroll
  for (int p = 0; p < XL; ++p) xr[p] = *reinterpret_cast<const mx4_u32x4*>(xsrc[p]);
#pragma unroll
  for (int st = 0; st < KS; ++st)
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      wr[st][j] = __builtin_nontemporal_load(reinterpret_cast<const mx4_u32x4*>(wp[j] + (size_t)st * 1024));
      sr[st][j] = sp[j][(size_t)st * 64];
    }

  // one chunk: x regs -> LDS buffer c & 1, next chunk's x loads, barrier, then per k-step
  // widen + refill + MFMAs.  MORE is a template constant (the last chunk is peeled) so
  // the loop body is branch-free, as in w8_xr_kernel.
  auto chunk = [&](int c, auto more_tag) {
    constexpr bool MORE = decltype(more_tag)::value;
    uint16_t* sx = s_x[c & 1];
#pragma unroll
    for (int p = 0; p < XL; ++p) {
      const int e = tid + 256 * p;
      const int row = e / CPR, ch = e % CPR;
      const int slot = (ch & ~7) | ((ch & 7) ^ (row & 7));
      *reinterpret_cast<mx4_u32x4*>(&sx[row * KC + slot * 8]) = xr[p];
    }
    if constexpr (MORE) {
#pragma unroll
      for (int p = 0; p < XL; ++p) xr[p] = *reinterpret_cast<const mx4_u32x4*>(xsrc[p] + (c + 1) * KC);
    }
    __syncthreads();   // chunk c visible; every wave is past chunk c-1's reads of the other buffer
    const size_t nxt = (size_t)(c + 1) * KS;
#pragma unroll
    for (int st = 0; st < KS; ++st) {
      mx4_bf16x8 wf[NT][4];
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const float scale = __builtin_bit_cast(float, sr[st][j] << 23);
#pragma unroll
        for (int q = 0; q < 4; ++q) wf[j][q] = mx4_widen(wr[st][j][q], scale);
      }
      if constexpr (MORE) {   // refill this k-step's registers with the next chunk's fragment
#pragma unroll
        for (int j = 0; j < NT; ++j) {
          wr[st][j] = __builtin_nontemporal_load(
              reinterpret_cast<const mx4_u32x4*>(wp[j] + (nxt + st) * 1024));
          sr[st][j] = sp[j][(nxt + st) * 64];
        }
      }
#pragma unroll
      for (int i = 0; i < MT; ++i) {
        const int row = 16 * i + l15;
        mx4_u32x4 xf[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int ch = st * 16 + 4 * g + q;
          const int slot = (ch & ~7) | ((ch & 7) ^ (row & 7));
          xf[q] = *reinterpret_cast<const mx4_u32x4*>(&sx[row * KC + slot * 8]);
        }
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
          for (int q = 0; q < 4; ++q)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(mx4_bf16x8, xf[q]),
                                                                wf[j][q], acc[i][j], 0, 0, 0);
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
          const float gt = acc[i][0][r], up = acc[i][1][r];
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
            if (ws == nullptr)
              out[(size_t)m * out_stride + n] = f32_to_bf16(acc[i][j][r]);
            else
              slab[(size_t)m * N + n] = acc[i][j][r];
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
extern "C" int ft_mx4_gemm(const void* x, int x_stride, int M, const uint8_t* wq, const uint8_t* sc,
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
#define FT_MX4(MT_, NT_, KC_, E_)                                                            \
  if (mt == MT_ && nt == NT_ && kc == KC_ && silu == E_) {                                   \
    hipLaunchKernelGGL((ft::mx4_xr_kernel<MT_, NT_, KC_, E_>), grid, block, 0, stream,       \
                       (const uint16_t*)x, x_stride, M, wq, sc, K, ws, (uint16_t*)out,       \
                       out_stride, N, k_slice);                                              \
    return static_cast<int>(hipGetLastError());                                              \
  }
#define FT_MX4_M(NT_, KC_, E_) \
  FT_MX4(1, NT_, KC_, E_) FT_MX4(2, NT_, KC_, E_) FT_MX4(3, NT_, KC_, E_) FT_MX4(4, NT_, KC_, E_)
  silu = silu ? 1 : 0;
  FT_MX4_M(1, 256, 0) FT_MX4_M(2, 256, 0) FT_MX4_M(4, 256, 0) FT_MX4_M(2, 256, 1)
  FT_MX4_M(1, 512, 0) FT_MX4_M(2, 512, 0) FT_MX4_M(4, 512, 0) FT_MX4_M(2, 512, 1)
#undef FT_MX4_M
#undef FT_MX4
  return -5;
}
