// Per-token logprobs: log-softmax of a step's raw logits at the sampled id, plus the
// top-N alternatives (OpenAI `logprobs` / `top_logprobs`, N <= 20).
//
// Runs eagerly right after the sampler, only in steps where some row asked (`want[r]`
// >= 0); rows with want = -1 exit at once.  Everything is fp32 over the logits widened
// to fp32: logprob(t) = (x[t] - M) - log(sum exp(x - M)), M the row maximum (the
// difference first: at |M| ~ 3e4 the sum M + log Z would round away the log).
//
// Like the sampler's multi-workgroup path (sampling.hip) the vocabulary of a row is
// cut into kLpSlices slices, each streamed once by its own workgroup with 16-B lane
// loads:
//   K1 slice  (kLpSlices x rows): the slice's max M_p and Z_p = sum exp(x - M_p), and
//             its own `want` best candidates
//   K2 merge  (rows, one wave): M, Z from the slice stats; the candidates merged into
//             the sorted top-`want`; the sampled id's logit with one load
// The order is total and exact: a candidate is the 64-bit word (ordered key of the
// fp32 value << 32 | ~id), so a larger word is a larger logit or, on equal logits, a
// lower id -- no threshold, no tie bucket to overflow, and every word of a row is
// distinct.  The global top-N is a subset of the union of the slices' top-N.  bf16
// logits over 128k ids tie often; ties cost nothing here.  -0.0 orders as +0.0 (they
// compare equal, so the id decides), as in a stable sort of the values.
//
// Prompt logprobs (ft_prompt_logprobs, SamplingParams.prompt_logprobs) are the same two
// kernels instantiated with kRank: column 0 is a GIVEN id per row (the next prompt
// token), and the row's rank = 1 + #{ids with a greater key} comes out as well.  K1 loads
// the target's logit once per workgroup and counts, in the pass it makes anyway, its own
// ids whose key exceeds the target's; K2 sums the 32 per-slice counts (integers: exact,
// order-free, no atomics, no second read of the row).  Equal keys do not count, so ties
// share a rank and -0.0 ranks as +0.0.  ft_logprobs launches the instantiations without
// kRank: the code, workspace layout and results it always had.
#include "ft_common.h"

namespace ft {

constexpr int kLpMax = 20;                 // OpenAI's cap on top_logprobs
constexpr int kLpCols = 1 + kLpMax;        // column 0: the sampled token
constexpr int kLpSlices = 32;
constexpr int kLpThreads = 256;
constexpr int kLpWaves = kLpThreads / 64;
constexpr int kLpChunks = 2;               // 8-id chunks per thread: slices of <= 4096 ids
constexpr int kLpMaxVocab = kLpSlices * kLpThreads * 8 * kLpChunks;
// per-row scratch, 64-bit words: slice stats (M_p bits | Z_p bits << 32) x kLpSlices,
// then kLpMax candidate words per slice (0 = none)
constexpr int kLpWsCand = kLpSlices, kLpWsRow = kLpWsCand + kLpSlices * kLpMax;
// prompt logprobs (ft_prompt_logprobs) count the target's rank as well: the same row
// layout with one more word per slice behind it, the slice's number of ids whose key
// exceeds the target's
constexpr int kLpWsCount = kLpWsRow, kLpWsRowRank = kLpWsCount + kLpSlices;
static_assert(kLpSlices <= 64 && kLpCols <= 64, "one lane per slice / output column");
static_assert(kLpWaves * kLpMax <= 128, "two candidates per lane in the slice merge");

typedef unsigned long long lp_u64;

// monotonic 32-bit key of an fp32 value (-0.0 as +0.0); never 0 for a non-NaN value
__device__ __forceinline__ uint32_t lp_key(float x) {
  uint32_t u = __float_as_uint(x);
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float lp_key_f32(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
__device__ __forceinline__ lp_u64 lp_word(uint32_t key, int id) {
  return ((lp_u64)key << 32) | (uint32_t)~id;
}

__device__ __forceinline__ lp_u64 wave_max_u64(lp_u64 v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t hi = (uint32_t)__shfl_xor((int)(v >> 32), o, 64);
    const uint32_t lo = (uint32_t)__shfl_xor((int)v, o, 64);
    const lp_u64 t = ((lp_u64)hi << 32) | lo;
    v = t > v ? t : v;
  }
  return v;
}

__device__ __forceinline__ float lp_widen(const uint16_t* x, long i) { return bf16_to_f32(x[i]); }
__device__ __forceinline__ float lp_widen(const float* x, long i) { return x[i]; }

// ids base .. base + 7 of a row (base a multiple of 8, < vocab) widened to fp32; the
// chunk that straddles the end of the vocabulary is read id by id (nothing past
// vocab is touched); returns how many of the 8 are ids of the row
template <typename T>
__device__ __forceinline__ int lp_load8(const T* x, int base, int vocab, float (&f)[8]) {
  if (base + 8 <= vocab) {
    if constexpr (sizeof(T) == 2) {
      load8(*reinterpret_cast<const uint4*>(x + base), f);
    } else {
      const float4 a = *reinterpret_cast<const float4*>(x + base);
      const float4 c = *reinterpret_cast<const float4*>(x + base + 4);
      f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w;
      f[4] = c.x; f[5] = c.y; f[6] = c.z; f[7] = c.w;
    }
    return 8;
  }
  const int n = vocab - base;
#pragma unroll
  for (int j = 0; j < 8; ++j) f[j] = j < n ? lp_widen(x, base + j) : -INFINITY;
  return n;
}

__device__ __forceinline__ int lp_slice_len(int vocab) {
  return ((vocab + kLpSlices * 8 - 1) / (kLpSlices * 8)) * 8;
}

// want[row]: -1 = nothing asked; 0..kLpMax alternatives
__device__ __forceinline__ int lp_want(const int* want, int row) {
  const int w = want[row];
  if (w < 0) return -1;
  return min(FT_CHECK_IDX(w, kLpMax + 1, kCkLogprobWant, row), kLpMax);
}

__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// kRank (ft_prompt_logprobs): `targets` holds the row's given id; the slice also counts
// its ids whose key exceeds the target's key, in the pass it makes anyway
template <typename T, bool kRank>
__global__ __launch_bounds__(kLpThreads) void logprob_slice_kernel(
    const T* __restrict__ logits, long stride, int vocab, const int* __restrict__ want,
    lp_u64* __restrict__ ws, const int* __restrict__ targets) {
  constexpr int kWsRow = kRank ? kLpWsRowRank : kLpWsRow;
  __shared__ float s_m[kLpWaves], s_z[kLpWaves];
  __shared__ lp_u64 s_c[kLpWaves * kLpMax];
  __shared__ int s_n[kRank ? kLpWaves : 1];
  const int row = blockIdx.y, p = blockIdx.x, tid = threadIdx.x, lane = lane_id();
  const int nk = lp_want(want, row);
  if (nk < 0) return;
  const T* x = logits + (long)row * stride;
  const int S = lp_slice_len(vocab);
  const int beg = p * S, end = min(vocab, beg + S);

  // one pass: the thread's ids as ordered keys (0 = no id), the wave's max and exp-sum
  uint32_t key[8 * kLpChunks];
  float f[8 * kLpChunks];
  float m = -INFINITY;
#pragma unroll
  for (int c = 0; c < kLpChunks; ++c) {
    const int base = beg + (tid + c * kLpThreads) * 8;
    float v[8];
    const int n = base < end ? lp_load8<T>(x, base, vocab, v) : 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      f[8 * c + j] = j < n ? v[j] : -INFINITY;
      key[8 * c + j] = j < n ? lp_key(v[j]) : 0u;
      m = fmaxf(m, f[8 * c + j]);
    }
  }
  if constexpr (kRank) {
    // the target's logit, one (uniform) load per workgroup; an id outside the row is
    // never read and counts nothing.  Keys of ids are never 0 and 0 marks "no id", so
    // the comparison needs no validity test of its own.
    const int t = targets[row];
    int above = 0;
    if (t >= 0 && t < vocab) {
      const uint32_t tk = lp_key(lp_widen(x, t));
#pragma unroll
      for (int j = 0; j < 8 * kLpChunks; ++j) above += key[j] > tk ? 1 : 0;
    }
    above = wave_sum_i32(above);
    if (lane == 0) s_n[wave_id()] = above;
  }
  m = wave_max(m);
  float z = 0.f;
  if (m > -INFINITY) {
#pragma unroll
    for (int j = 0; j < 8 * kLpChunks; ++j) z += exp2f((f[j] - m) * 1.4426950408889634f);
  }
  z = wave_sum(z);
  if (lane == 0) {
    s_m[wave_id()] = m;
    s_z[wave_id()] = z;
  }

  // the wave's nk best: nk rounds of a wave argmax over each lane's best remaining id
  auto id_of = [&](int j) { return beg + (tid + (j >> 3) * kLpThreads) * 8 + (j & 7); };
  auto lane_best = [&]() -> lp_u64 {
    uint32_t bk = 0u;
    int bi = 0;
#pragma unroll
    for (int j = 0; j < 8 * kLpChunks; ++j)
      if (key[j] > bk) {   // ids ascend with j: the lowest id of equal keys stays
        bk = key[j];
        bi = id_of(j);
      }
    return bk ? lp_word(bk, bi) : 0ull;
  };
  lp_u64 b = nk > 0 ? lane_best() : 0ull;
  for (int r = 0; r < nk; ++r) {
    const lp_u64 w = wave_max_u64(b);
    if (lane == 0) s_c[wave_id() * kLpMax + r] = w;
    if (w != 0ull && b == w) {
      const int wid = (int)~(uint32_t)w;
#pragma unroll
      for (int j = 0; j < 8 * kLpChunks; ++j)
        if (id_of(j) == wid) key[j] = 0u;
      b = lane_best();
    }
  }
  __syncthreads();
  if (wave_id() != 0) return;

  // wave 0: the slice's stats, and its nk best of the waves' candidates
  lp_u64* wr = ws + (long)row * kWsRow;
  if constexpr (kRank) {
    if (lane == 0) {
      int above = 0;
#pragma unroll
      for (int w = 0; w < kLpWaves; ++w) above += s_n[w];
      wr[kLpWsCount + p] = (lp_u64)(uint32_t)above;
    }
  }
  if (lane == 0) {
    float M = s_m[0];
#pragma unroll
    for (int w = 1; w < kLpWaves; ++w) M = fmaxf(M, s_m[w]);
    float Z = 0.f;
#pragma unroll
    for (int w = 0; w < kLpWaves; ++w)
      Z += s_m[w] > -INFINITY ? s_z[w] * exp2f((s_m[w] - M) * 1.4426950408889634f) : 0.f;
    wr[p] = (lp_u64)__float_as_uint(M) | ((lp_u64)__float_as_uint(Z) << 32);
  }
  lp_u64 c0 = 0ull, c1 = 0ull;
  if (lane % kLpMax < nk && lane < kLpWaves * kLpMax) c0 = s_c[lane];
  if ((lane + 64) % kLpMax < nk && lane + 64 < kLpWaves * kLpMax) c1 = s_c[lane + 64];
  lp_u64 mine = 0ull;
  for (int r = 0; r < nk; ++r) {
    const lp_u64 w = wave_max_u64(c0 > c1 ? c0 : c1);
    if (lane == r) mine = w;
    if (w != 0ull) {   // words are distinct: one lane holds it
      if (c0 == w) c0 = 0ull;
      if (c1 == w) c1 = 0ull;
    }
  }
  if (lane < kLpMax) wr[kLpWsCand + p * kLpMax + lane] = mine;
}

// kRank: `sampled` holds the given target ids; the slices' counts are summed (integers:
// exact, in any order) into out_rank = 1 + ids with a greater logit
template <typename T, bool kRank>
__global__ __launch_bounds__(64) void logprob_merge_kernel(
    const T* __restrict__ logits, long stride, int vocab, const int* __restrict__ sampled,
    const int* __restrict__ want, const lp_u64* __restrict__ ws, float* __restrict__ out_lp,
    int* __restrict__ out_id, int* __restrict__ out_rank) {
  constexpr int kWsRow = kRank ? kLpWsRowRank : kLpWsRow;
  constexpr int NC = kLpSlices * kLpMax / 64;   // candidate words per lane
  static_assert(NC * 64 == kLpSlices * kLpMax, "candidates divide over the wave");
  const int row = blockIdx.x, lane = threadIdx.x;
  const int nk = lp_want(want, row);
  if (nk < 0) return;
  const lp_u64* wr = ws + (long)row * kWsRow;
  float mp = -INFINITY, zp = 0.f;
  if (lane < kLpSlices) {
    const lp_u64 st = wr[lane];
    mp = __uint_as_float((uint32_t)st);
    zp = __uint_as_float((uint32_t)(st >> 32));
  }
  const float M = wave_max(mp);
  const float Z = wave_sum(mp > -INFINITY ? zp * exp2f((mp - M) * 1.4426950408889634f) : 0.f);
  const float logZ = logf(Z);
  // a -inf logit has logprob -inf, never NaN (also when the whole row is -inf)
  auto logprob = [&](float v) { return v == -INFINITY ? -INFINITY : (v - M) - logZ; };

  lp_u64 c[NC];
#pragma unroll
  for (int j = 0; j < NC; ++j) c[j] = wr[kLpWsCand + lane + 64 * j];   // slots >= nk hold 0
  auto lane_best = [&]() -> lp_u64 {
    lp_u64 b = 0ull;
#pragma unroll
    for (int j = 0; j < NC; ++j) b = c[j] > b ? c[j] : b;
    return b;
  };
  lp_u64 b = lane_best(), mine = 0ull;
  for (int r = 0; r < nk; ++r) {
    const lp_u64 w = wave_max_u64(b);
    if (lane == r + 1) mine = w;
    if (w != 0ull && b == w) {
#pragma unroll
      for (int j = 0; j < NC; ++j)
        if (c[j] == w) c[j] = 0ull;
      b = lane_best();
    }
  }
  int above = 0;
  if constexpr (kRank) above = wave_sum_i32(lane < kLpSlices ? (int)(uint32_t)wr[kLpWsCount + lane] : 0);
  if (lane >= kLpCols) return;
  int id = -1;
  float lp = 0.f;
  if (lane == 0) {
    int s;
    if constexpr (kRank) {
      s = sampled[row];   // (the checked build records an id outside the row, and reads nothing)
      (void)FT_CHECK_IDX(s, vocab, kCkPromptTarget, row);
    } else {
      s = FT_CHECK_IDX(sampled[row], vocab, kCkSampled, row);
    }
    if (s >= 0 && s < vocab) {
      id = s;
      lp = logprob(lp_widen(logits + (long)row * stride, s));
    }
    if constexpr (kRank) out_rank[row] = id >= 0 ? 1 + above : 0;
  } else if (mine != 0ull) {
    id = (int)~(uint32_t)mine;
    lp = logprob(lp_key_f32((uint32_t)(mine >> 32)));
  }
  out_lp[(long)row * kLpCols + lane] = lp;
  out_id[(long)row * kLpCols + lane] = id;
}

}  // namespace ft

extern "C" int ft_logprobs_max() { return ft::kLpMax; }
extern "C" int ft_logprobs_ws_words() { return ft::kLpWsRow; }

// ws: rows * ft_logprobs_ws_words() 64-bit words; out_lp / out_id: [rows, 1 + kLpMax]
extern "C" int ft_logprobs(const void* logits, int is_bf16, long stride, int rows, int vocab,
                           const int* sampled, const int* want, void* ws, float* out_lp,
                           int* out_id, hipStream_t stream) {
  if (rows <= 0 || vocab <= 0) return 0;
  if (rows > 65535) return -1;
  if (vocab > ft::kLpMaxVocab) return -3;
  if (stride % 8 != 0 || stride < vocab || reinterpret_cast<uintptr_t>(logits) % 16 != 0) return -4;
  using namespace ft;
  lp_u64* w = static_cast<lp_u64*>(ws);
#define FT_LP_LAUNCH(TT)                                                                        \
  {                                                                                             \
    const TT* lg = static_cast<const TT*>(logits);                                              \
    hipLaunchKernelGGL((logprob_slice_kernel<TT, false>), dim3(kLpSlices, rows),                \
                       dim3(kLpThreads), 0, stream, lg, stride, vocab, want, w,                 \
                       (const int*)nullptr);                                                    \
    hipLaunchKernelGGL((logprob_merge_kernel<TT, false>), dim3(rows), dim3(64), 0, stream, lg,  \
                       stride, vocab, sampled, want, (const lp_u64*)w, out_lp, out_id,          \
                       (int*)nullptr);                                                          \
  }
  if (is_bf16) FT_LP_LAUNCH(uint16_t) else FT_LP_LAUNCH(float)
#undef FT_LP_LAUNCH
  return static_cast<int>(hipGetLastError());
}

extern "C" int ft_prompt_logprobs_ws_words() { return ft::kLpWsRowRank; }

// Prompt logprobs: as ft_logprobs with the given `targets` in place of the sampled ids,
// plus out_rank [rows] = 1 + ids of the row with a greater logit (ties share a rank; 0 for
// a target outside [0, vocab), which is never read).  ws: rows *
// ft_prompt_logprobs_ws_words() 64-bit words.
extern "C" int ft_prompt_logprobs(const void* logits, int is_bf16, long stride, int rows,
                                  int vocab, const int* targets, const int* want, void* ws,
                                  float* out_lp, int* out_id, int* out_rank,
                                  hipStream_t stream) {
  if (rows <= 0 || vocab <= 0) return 0;
  if (rows > 65535) return -1;
  if (vocab > ft::kLpMaxVocab) return -3;
  if (stride % 8 != 0 || stride < vocab || reinterpret_cast<uintptr_t>(logits) % 16 != 0) return -4;
  using namespace ft;
  lp_u64* w = static_cast<lp_u64*>(ws);
#define FT_PLP_LAUNCH(TT)                                                                       \
  {                                                                                             \
    const TT* lg = static_cast<const TT*>(logits);                                              \
    hipLaunchKernelGGL((logprob_slice_kernel<TT, true>), dim3(kLpSlices, rows),                 \
                       dim3(kLpThreads), 0, stream, lg, stride, vocab, want, w, targets);       \
    hipLaunchKernelGGL((logprob_merge_kernel<TT, true>), dim3(rows), dim3(64), 0, stream, lg,   \
                       stride, vocab, targets, want, (const lp_u64*)w, out_lp, out_id,          \
                       out_rank);                                                               \
  }
  if (is_bf16) FT_PLP_LAUNCH(uint16_t) else FT_PLP_LAUNCH(float)
#undef FT_PLP_LAUNCH
  return static_cast<int>(hipGetLastError());
}

// checked build: this unit's error-word / limits hook (ft_common.h)
FT_CHECK_HOOK(logprobs)
