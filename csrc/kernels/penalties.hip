// K14: sampler logit processors -- repetition / presence / frequency penalties and
// logit_bias -- over per-sequence device state.
//
// State: table uint16 [S, V] (row stride `tstride` elements, a multiple of 8 when the
// 16-B path is to be used): bit 15 = "token is in the prompt", bits 0-14 = how often
// the token was generated so far (saturating at 32767); one bias list per slot,
// bias_ids int32 [S, kPenMaxBias] (-1 padded) / bias_vals fp32 [S, kPenMaxBias].
//
// For a row with slot s >= 0 and raw logit l of token v (e = table[s][v], c = e & 0x7fff):
//   1. e != 0:  l = l > 0 ? l / rep : l * rep       (prompt and output tokens)
//   2.          l -= freq * c + pres * (c > 0)      (output tokens)
//   3.          l += bias[v]
// computed in fp32 with every operation rounded on its own (no FMA contraction: the
// result is bit-for-bit ops/reference.py apply_penalties) and rounded once to the
// logits' dtype.  An element with e == 0 and no bias, and every row with slot < 0,
// is copied unchanged.
#include "ft_common.h"

namespace ft {

constexpr int kPenMaxBias = 300;
constexpr int kPenThreads = 256;
constexpr int kPenChunk = kPenThreads * 8;   // columns one workgroup covers per pass
constexpr int kPenMaxGridX = 64;             // workgroups per row (grid-strided beyond)

__device__ __forceinline__ float pen_value(float l, uint32_t e, float rep, float pres, float freq) {
  // __f*_rn: never contracted into an FMA, so the kernel rounds where the reference rounds
  const float c = static_cast<float>(e & 0x7fffu);
  l = l > 0.f ? __fdiv_rn(l, rep) : __fmul_rn(l, rep);
  const float pen = __fadd_rn(__fmul_rn(freq, c), (e & 0x7fffu) ? pres : 0.f);
  return __fsub_rn(l, pen);
}

template <bool BF16>
__device__ __forceinline__ float pen_load(const void* p, long i) {
  if (BF16) return bf16_to_f32(static_cast<const uint16_t*>(p)[i]);
  return static_cast<const float*>(p)[i];
}

template <bool BF16>
__device__ __forceinline__ void pen_store(void* p, long i, float v) {
  if (BF16)
    static_cast<uint16_t*>(p)[i] = f32_to_bf16(v);
  else
    static_cast<float*>(p)[i] = v;
}

// grid (gx, B).  Workgroup bx of a row owns the column chunks c with c % gx == bx: it
// is the only one that reads or writes them, so `out` may alias `logits`.  A biased
// token's final value is computed from its raw logit BEFORE the elementwise pass
// (which may overwrite the raw logit in place) and stored after it, behind a barrier.
template <bool BF16, bool VEC>
__global__ __launch_bounds__(kPenThreads) void penalty_apply_kernel(
    const void* logits_, void* out_, long lstride, long ostride, int vocab,
    const int* __restrict__ slots, const float* __restrict__ rep_, const float* __restrict__ pres_,
    const float* __restrict__ freq_, const uint16_t* __restrict__ table, long tstride, int num_slots,
    const int* __restrict__ bias_ids, const float* __restrict__ bias_vals) {
  const int row = blockIdx.y, bx = blockIdx.x, gx = gridDim.x, tid = threadIdx.x;
  const char* lrow = static_cast<const char*>(logits_) + (long)row * lstride * (BF16 ? 2 : 4);
  char* orow = static_cast<char*>(out_) + (long)row * ostride * (BF16 ? 2 : 4);
  const bool alias = static_cast<const void*>(lrow) == static_cast<void*>(orow);
  int slot = slots[row];
  if (slot >= 0) slot = FT_CHECK_IDX(slot, num_slots, kCkPenSlot, row);
  if (slot >= num_slots) slot = -1;
  if (slot < 0 && alias) return;
  const int nvec = VEC ? vocab / 8 : 0;   // 8-column groups moved 16 B per lane

  if (slot < 0) {   // unpenalised row of an out-of-place call: a copy
    if (VEC) {
      for (int g = bx * kPenThreads + tid; g < nvec; g += gx * kPenThreads) {
        if (BF16) {
          reinterpret_cast<uint4*>(orow)[g] = reinterpret_cast<const uint4*>(lrow)[g];
        } else {
          reinterpret_cast<uint4*>(orow)[2 * g] = reinterpret_cast<const uint4*>(lrow)[2 * g];
          reinterpret_cast<uint4*>(orow)[2 * g + 1] = reinterpret_cast<const uint4*>(lrow)[2 * g + 1];
        }
      }
    }
    for (int v = nvec * 8 + bx * kPenThreads + tid; v < vocab; v += gx * kPenThreads) {
      if (BF16)
        reinterpret_cast<uint16_t*>(orow)[v] = reinterpret_cast<const uint16_t*>(lrow)[v];
      else
        reinterpret_cast<uint32_t*>(orow)[v] = reinterpret_cast<const uint32_t*>(lrow)[v];
    }
    return;
  }

  const float rep = rep_[row], pres = pres_[row], freq = freq_[row];
  const uint16_t* trow = table + (long)slot * tstride;

  // this workgroup's biased tokens (at most two per thread): final values from raw logits
  float bval[2];
  int bid[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int i = tid + k * kPenThreads;
    bid[k] = -1;
    if (i < kPenMaxBias) {
      int id = bias_ids[(long)slot * kPenMaxBias + i];
      if (id >= 0) id = FT_CHECK_IDX(id, vocab, kCkPenToken, row);
      // owner of column id: the vector chunks are dealt round-robin, the scalar tail
      // columns (past nvec * 8) are dealt thread-wise in the same way
      if (id >= 0 && id < vocab) {
        const int owner = id < nvec * 8 ? ((id / 8) / kPenThreads) % gx
                                        : ((id - nvec * 8) / kPenThreads) % gx;
        if (owner == bx) {
          const uint32_t e = trow[id];
          float l = pen_load<BF16>(lrow, id);
          if (e) l = pen_value(l, e, rep, pres, freq);
          bval[k] = __fadd_rn(l, bias_vals[(long)slot * kPenMaxBias + i]);
          bid[k] = id;
        }
      }
    }
  }
  __syncthreads();   // the raw logits of biased tokens are read before anyone overwrites them

  if (VEC) {
    for (int g = bx * kPenThreads + tid; g < nvec; g += gx * kPenThreads) {
      const uint4 e4 = reinterpret_cast<const uint4*>(trow)[g];
      const bool any = (e4.x | e4.y | e4.z | e4.w) != 0u;
      const uint32_t ew[4] = {e4.x, e4.y, e4.z, e4.w};
      if (BF16) {
        uint4 l4 = reinterpret_cast<const uint4*>(lrow)[g];
        if (any) {
          float f[8];
          load8(l4, f);
          uint32_t lw[4] = {l4.x, l4.y, l4.z, l4.w};
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const uint32_t e0 = ew[j] & 0xffffu, e1 = ew[j] >> 16;
            // untouched elements keep their input bits (a NaN payload included)
            if (e0) lw[j] = (lw[j] & 0xffff0000u) | f32_to_bf16(pen_value(f[2 * j], e0, rep, pres, freq));
            if (e1) lw[j] = (lw[j] & 0x0000ffffu) |
                            ((uint32_t)f32_to_bf16(pen_value(f[2 * j + 1], e1, rep, pres, freq)) << 16);
          }
          l4 = make_uint4(lw[0], lw[1], lw[2], lw[3]);
        }
        if (any || !alias) reinterpret_cast<uint4*>(orow)[g] = l4;
      } else {
        float4 a = reinterpret_cast<const float4*>(lrow)[2 * g];
        float4 b = reinterpret_cast<const float4*>(lrow)[2 * g + 1];
        if (any) {
          float f[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const uint32_t e0 = ew[j] & 0xffffu, e1 = ew[j] >> 16;
            if (e0) f[2 * j] = pen_value(f[2 * j], e0, rep, pres, freq);
            if (e1) f[2 * j + 1] = pen_value(f[2 * j + 1], e1, rep, pres, freq);
          }
          a = make_float4(f[0], f[1], f[2], f[3]);
          b = make_float4(f[4], f[5], f[6], f[7]);
        }
        if (any || !alias) {
          reinterpret_cast<float4*>(orow)[2 * g] = a;
          reinterpret_cast<float4*>(orow)[2 * g + 1] = b;
        }
      }
    }
  }
  // scalar tail (vocab % 8 columns), or every column when a pointer or stride rules
  // out 16-B accesses
  for (int v = nvec * 8 + bx * kPenThreads + tid; v < vocab; v += gx * kPenThreads) {
    const uint32_t e = trow[v];
    if (e) {
      pen_store<BF16>(orow, v, pen_value(pen_load<BF16>(lrow, v), e, rep, pres, freq));
    } else if (!alias) {
      if (BF16)
        reinterpret_cast<uint16_t*>(orow)[v] = reinterpret_cast<const uint16_t*>(lrow)[v];
      else
        reinterpret_cast<uint32_t*>(orow)[v] = reinterpret_cast<const uint32_t*>(lrow)[v];
    }
  }
  __syncthreads();   // the elementwise pass of this workgroup's columns is complete
#pragma unroll
  for (int k = 0; k < 2; ++k)
    if (bid[k] >= 0) pen_store<BF16>(orow, bid[k], bval[k]);
}

// one thread per row: saturating +1 on table[slot][sampled token]; rows of one step
// hold distinct slots, so no two threads touch one element
__global__ __launch_bounds__(64) void penalty_update_kernel(uint16_t* __restrict__ table,
                                                            long tstride, int num_slots, int vocab,
                                                            const int* __restrict__ slots,
                                                            const int* __restrict__ sampled,
                                                            int rows) {
  const int r = blockIdx.x * 64 + threadIdx.x;
  if (r >= rows) return;
  int slot = slots[r];
  if (slot < 0) return;
  slot = FT_CHECK_IDX(slot, num_slots, kCkPenSlot, r);
  const int tok = FT_CHECK_IDX(sampled[r], vocab, kCkPenToken, r);
  if (slot >= num_slots || tok < 0 || tok >= vocab) return;
  uint16_t* p = table + (long)slot * tstride + tok;
  const uint16_t e = *p;
  if ((e & 0x7fffu) != 0x7fffu) *p = e + 1;
}

// clears row `slot` and scatters n unique (token, value) pairs into it; workgroup bx
// owns the columns of chunks c % gx == bx for both, so one barrier orders them.
// Workgroup 0 also installs the slot's bias list.
__global__ __launch_bounds__(kPenThreads) void penalty_seed_kernel(
    uint16_t* __restrict__ table, long tstride, int num_slots, int vocab, int slot,
    const int* __restrict__ ids, const int* __restrict__ vals, int n, int* __restrict__ bias_ids,
    float* __restrict__ bias_vals, const int* __restrict__ src_ids,
    const float* __restrict__ src_vals) {
  const int bx = blockIdx.x, gx = gridDim.x, tid = threadIdx.x;
  slot = FT_CHECK_IDX(slot, num_slots, kCkPenSlot, 0);
  if (slot < 0 || slot >= num_slots) return;
  uint16_t* trow = table + (long)slot * tstride;
  const bool vec = (tstride % 8 == 0) && (reinterpret_cast<uintptr_t>(table) % 16 == 0);
  const int nvec = vec ? vocab / 8 : 0;
  for (int g = bx * kPenThreads + tid; g < nvec; g += gx * kPenThreads)
    reinterpret_cast<uint4*>(trow)[g] = make_uint4(0u, 0u, 0u, 0u);
  for (int v = nvec * 8 + bx * kPenThreads + tid; v < vocab; v += gx * kPenThreads) trow[v] = 0;
  __syncthreads();
  for (int i = tid; i < n; i += kPenThreads) {
    const int id = FT_CHECK_IDX(ids[i], vocab, kCkPenToken, i);
    if (id < 0 || id >= vocab) continue;
    const int owner = id < nvec * 8 ? ((id / 8) / kPenThreads) % gx
                                    : ((id - nvec * 8) / kPenThreads) % gx;
    if (owner == bx) trow[id] = static_cast<uint16_t>(vals[i]);
  }
  if (bx == 0) {
    for (int i = tid; i < kPenMaxBias; i += kPenThreads) {
      int id = src_ids[i];
      if (id >= 0) id = FT_CHECK_IDX(id, vocab, kCkPenToken, i);
      bias_ids[(long)slot * kPenMaxBias + i] = (id >= 0 && id < vocab) ? id : -1;
      bias_vals[(long)slot * kPenMaxBias + i] = src_vals[i];
    }
  }
}

// memory-bound: about 2048 workgroups in all, the rest grid-strided
static int pen_grid_x(int vocab, int rows) {
  int gx = (vocab + kPenChunk - 1) / kPenChunk;
  int cap = 2048 / (rows < 1 ? 1 : rows);
  if (cap < 4) cap = 4;
  if (cap > kPenMaxGridX) cap = kPenMaxGridX;
  if (gx > cap) gx = cap;
  return gx < 1 ? 1 : gx;
}

}  // namespace ft

extern "C" int ft_penalty_max_bias() { return ft::kPenMaxBias; }

extern "C" int ft_penalty_apply(const void* logits, void* out, int is_bf16, long lstride,
                                long ostride, int rows, int vocab, const int* slots,
                                const float* rep, const float* pres, const float* freq,
                                const void* table, long tstride, int num_slots,
                                const int* bias_ids, const float* bias_vals, hipStream_t stream) {
  if (rows <= 0 || vocab <= 0) return 0;
  if (rows > 65535) return -1;
  using namespace ft;
  // 16-B accesses need 16-B aligned rows in all three tensors
  const long esz = is_bf16 ? 2 : 4;
  const bool vec = reinterpret_cast<uintptr_t>(logits) % 16 == 0 &&
                   reinterpret_cast<uintptr_t>(out) % 16 == 0 &&
                   reinterpret_cast<uintptr_t>(table) % 16 == 0 && (lstride * esz) % 16 == 0 &&
                   (ostride * esz) % 16 == 0 && tstride % 8 == 0;
  const dim3 grid(pen_grid_x(vocab, rows), rows), block(kPenThreads);
  const uint16_t* t = static_cast<const uint16_t*>(table);
#define FT_PEN_LAUNCH(B, V)                                                                    \
  hipLaunchKernelGGL((penalty_apply_kernel<B, V>), grid, block, 0, stream, logits, out, lstride, \
                     ostride, vocab, slots, rep, pres, freq, t, tstride, num_slots, bias_ids,    \
                     bias_vals)
  if (is_bf16) {
    if (vec) FT_PEN_LAUNCH(true, true); else FT_PEN_LAUNCH(true, false);
  } else {
    if (vec) FT_PEN_LAUNCH(false, true); else FT_PEN_LAUNCH(false, false);
  }
#undef FT_PEN_LAUNCH
  return static_cast<int>(hipGetLastError());
}

extern "C" int ft_penalty_update(void* table, long tstride, int num_slots, int vocab,
                                 const int* slots, const int* sampled, int rows,
                                 hipStream_t stream) {
  if (rows <= 0) return 0;
  hipLaunchKernelGGL(ft::penalty_update_kernel, dim3((rows + 63) / 64), dim3(64), 0, stream,
                     static_cast<uint16_t*>(table), tstride, num_slots, vocab, slots, sampled, rows);
  return static_cast<int>(hipGetLastError());
}

extern "C" int ft_penalty_seed(void* table, long tstride, int num_slots, int vocab, int slot,
                               const int* ids, const int* vals, int n, int* bias_ids,
                               float* bias_vals, const int* src_ids, const float* src_vals,
                               hipStream_t stream) {
  if (slot < 0 || slot >= num_slots || vocab <= 0 || n < 0) return -1;
  hipLaunchKernelGGL(ft::penalty_seed_kernel, dim3(ft::pen_grid_x(vocab, 1)), dim3(ft::kPenThreads), 0,
                     stream, static_cast<uint16_t*>(table), tstride, num_slots, vocab, slot, ids,
                     vals, n, bias_ids, bias_vals, src_ids, src_vals);
  return static_cast<int>(hipGetLastError());
}

// checked build: this unit's error-word / limits hook (ft_common.h)
FT_CHECK_HOOK(penalties)
