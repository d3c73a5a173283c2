// What the read paths of the memory share (affinity.hip: fp32 list kernels + merge; affinity_prefilter.hip: fp16
// pre-filter + exact re-scoring; dense_read.hip: top_k > 32 and top_k = None): sizes, the order-preserving score keys,
// wave helpers, the bank lookup, the natural-order fp32 score, and the exact tail of a read (sort the k keys, exp,
// sequential sum, divide, usage counters or the hand-over format).  Indices, weights and usage counters of the paths
// are bit-identical BECAUSE they run this one text; a kernel that keeps an inline copy for its register allocation
// says which helper it mirrors.
#pragma once
#include <math.h>

#include "common.h"

#pragma clang fp contract(off)

namespace deva {

// the fp32 list kernels + merge as the fall-back of the pre-filter (affinity.hip); guard != NULL: run only if *guard != 0
int topk_fp32(const float* key_long, const float* shr_long, int n_long, const float* key_work, const float* shr_work,
              int n_work, const float* qk, const float* qe, int hw, int k, int splits, uint64_t* part_keys, void* stream,
              const uint32_t* guard);
int launch_merge(const uint64_t* keys, const uint32_t* cnt, int hw, int k, int lists, int32_t* idx, float* weight,
                 uint64_t* usage_fix, uint64_t* out_keys, uint32_t* out_cnt, uint32_t token_offset, void* stream,
                 const char* what, const uint32_t* guard = nullptr);

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef f32x4 f32x4_u __attribute__((aligned(4)));  // 16-B load from a dword-aligned address

constexpr int CK = 64;
constexpr int QT = 32;            // queries per wave (MFMA N)
constexpr int TOKT = 32;          // tokens per tile (MFMA M)
constexpr int CAP = 64;           // candidate slots per (range, query) handed to the merge kernel (one per lane)
constexpr int K_MAX = 32;         // top-k supported by the list / hand-over sizing
constexpr float TWO40 = 1099511627776.0f;  // usage counters: 2^40 fixed point (exact scaling)

__device__ __forceinline__ uint32_t orderable(float f) {
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float from_orderable(uint32_t o) {
  const uint32_t u = (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o;
  return __uint_as_float(u);
}
// 64-bit candidate keys (hand-over format, merge, re-score, dense): order-preserving score bits << 32 | ~token index,
// so a larger key is a better candidate (higher score first, then lower token index).

// Hand-over point of cross-lane communication through LDS inside one wave: a wavefront-scope acquire-release fence (the
// LDS pipeline executes a wave's accesses in order, so the fence costs no instruction; it is what makes the
// ordering part of the program instead of an assumption about the compiler) plus a wave barrier for the scheduler.
#define DEVA_COMPILER_FENCE()                               \
  do {                                                      \
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); \
    __builtin_amdgcn_wave_barrier();                        \
  } while (0)

__device__ __forceinline__ int wave_count(bool pred) { return __popcll(__builtin_amdgcn_ballot_w64(pred)); }
// number of set bits of a wave ballot below this lane
__device__ __forceinline__ int prefix_below(unsigned long long b) {
  return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
}

// Exact k-th largest of the unique non-zero 64-bit keys held E per lane (0 = empty slot) by bitwise
// bisection with wave ballots: 32 steps on the score half; the index half only if the k-th score is
// tied.  Requires >= k non-zero keys.  Everything >= the returned key is the top-k set.
template <int E>
__device__ __forceinline__ uint64_t kth_largest(const uint64_t (&e)[E], int n_live, int k) {
  uint32_t T = 0;
  for (int b = 31; b >= 0; --b) {
    const uint32_t trial = T | (1u << b);
    int cnt = 0;
#pragma unroll
    for (int i = 0; i < E; ++i)
      if (i < n_live) cnt += wave_count((uint32_t)(e[i] >> 32) >= trial);
    if (cnt >= k) {
      T = trial;
      // exactly k keys at or above the trial: it separates the top-k set, no need to resolve the
      // remaining bits (typically reached after ~10 of the 32 steps)
      if (cnt == k) return (uint64_t)T << 32;
    }
  }
  int above = 0, ties = 0;
#pragma unroll
  for (int i = 0; i < E; ++i)
    if (i < n_live) {
      above += wave_count((uint32_t)(e[i] >> 32) > T);
      ties += wave_count((uint32_t)(e[i] >> 32) == T);
    }
  const int need = k - above;  // ties to keep: the ones with the largest low half (lowest token index)
  uint32_t L = 0;
  if (ties > need) {
    for (int b = 31; b >= 0; --b) {
      const uint32_t trial = L | (1u << b);
      int cnt = 0;
#pragma unroll
      for (int i = 0; i < E; ++i)
        if (i < n_live) cnt += wave_count((uint32_t)(e[i] >> 32) == T && (uint32_t)e[i] >= trial);
      if (cnt >= need) L = trial;
    }
  }
  return ((uint64_t)T << 32) | L;
}

// the memory bank: token-major key rows [n][CK] and shrinkage [n] of the long-term segment (tokens 0 .. n_long - 1)
// followed by the working segment.  (AffArgs of the list kernels spells the same six fields out: its kernarg layout.)
struct Bank {
  const float* key_long;
  const float* shr_long;
  int n_long;
  const float* key_work;
  const float* shr_work;
  int n_total;
};

// a segment the caller does not have (n == 0, NULL) aliases the other one, so that no kernel selects a null pointer
inline Bank make_bank(const float* key_long, const float* shr_long, int n_long, const float* key_work,
                      const float* shr_work, int64_t n_total) {
  Bank b;
  b.key_long = key_long ? key_long : key_work;
  b.shr_long = shr_long ? shr_long : shr_work;
  b.n_long = n_long;
  b.key_work = key_work ? key_work : key_long;
  b.shr_work = shr_work ? shr_work : shr_long;
  b.n_total = (int)n_total;
  return b;
}

// key row and shrinkage of token n
__device__ __forceinline__ const float* bank_row(const Bank& b, int n, float* ms) {
  if (n < b.n_long) {
    *ms = b.shr_long[n];
    return b.key_long + (int64_t)n * CK;
  }
  *ms = b.shr_work[n - b.n_long];
  return b.key_work + (int64_t)(n - b.n_long) * CK;
}

// B operands of query q for MFMA t (channel 2t + half: natural channel order in the accumulation chain) and
// bsq = sum_c qe*qk^2 in the order ATen's CPU sum uses for this reduction (four 16-channel partial sums, then
// ((s0+s1)+s2)+s3 -- probed bit-equal on >99% of queries).  The two list kernels of affinity.hip spell this block
// out inline: substituting the call renumbers their registers.
__device__ __forceinline__ float load_query(const float* __restrict__ qk, const float* __restrict__ qe, int hw, int q,
                                            int half, float (&bqe)[CK / 2], float (&bqk)[CK / 2]) {
  float bs[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int t = 0; t < CK / 2; ++t) {
    const float e0 = qe[(int64_t)(2 * t) * hw + q], e1 = qe[(int64_t)(2 * t + 1) * hw + q];
    const float k0 = qk[(int64_t)(2 * t) * hw + q], k1 = qk[(int64_t)(2 * t + 1) * hw + q];
    bs[t >> 3] += e0 * (k0 * k0);
    bs[t >> 3] += e1 * (k1 * k1);
    bqe[t] = half ? e1 : e0;
    bqk[t] = half ? (k1 * e1) : (k0 * e0);
  }
  return ((bs[0] + bs[1]) + bs[2]) + bs[3];
}

// One score by the scalar FMA chain of v_mfma_f32_32x32x2_f32 (bit-identical to it, MI355X_MICROARCH.md): channels in
// natural order, mk^2 rounded before it enters the chain, qp = qk*qe rounded likewise, then
// ((2B - A) - bsq) * (ms / 8), every step rounded.  row: 16-B aligned key row; qe / qp: the query's operands as CK / 4
// four-channel pieces (registers or LDS).
template <typename Q4>
__device__ __forceinline__ float score_fp32(const float* row, const Q4& qe, const Q4& qp, float bsq, float ms) {
  float accA = 0.0f, accB = 0.0f;
#pragma unroll
  for (int j = 0; j < CK / 4; ++j) {
    const f32x4 x = *reinterpret_cast<const f32x4*>(row + 4 * j);
    const f32x4 qe4 = qe[j], qp4 = qp[j];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const float a = x[u];
      accA = __builtin_fmaf(a * a, qe4[u], accA);
      accB = __builtin_fmaf(a, qp4[u], accB);
    }
  }
  return (((accB + accB) - accA) - bsq) * (ms * 0.125f);  // 1/sqrt(CK) folded into the shrinkage (exact)
}

// ---- the tail of a read, one wave per query: lane r ends up with the r-th best of the query's k keys
// Stand-in key of a top-k slot without a survivor (only if scores are NaN -- a NaN fails every comparison of the
// selection; the reference's topk propagates NaN there): unique, below every real key, score bits of a NaN,
// token = lane (in range) -- the slot gets weight NaN / token `lane` instead of uninitialised LDS contents.
__device__ __forceinline__ uint64_t missing_slot_key(int lane) { return (uint64_t)(0xffffffffu - (uint32_t)lane); }

// Sort by rank counting: lanes 0 .. n-1 hold unique keys (k <= n <= 64), of which the k largest leave sorted --
// lane r < k returns the r-th best, the other lanes 0.  Lane j's key is broadcast through SGPRs (j is wave-uniform);
// lds: a row of 64 keys owned by this wave.
__device__ __forceinline__ uint64_t rank_sort_k(uint64_t cand, int n, int k, int lane, volatile uint64_t* lds) {
  int rank = 0;
  for (int j = 0; j < n; ++j) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)cand, j);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(cand >> 32), j);
    rank += ((((uint64_t)hi << 32) | lo) > cand) ? 1 : 0;
  }
  DEVA_COMPILER_FENCE();
  if (lane < n && rank < k) lds[rank] = cand;
  DEVA_COMPILER_FENCE();
  return lane < k ? lds[lane] : 0ull;
}

// the sorted top-k in the hand-over format (token index shifted by token_offset): a shard's own selection
__device__ __forceinline__ void write_out_keys(uint64_t best, int lane, int q, int k, uint64_t* __restrict__ out_keys,
                                               uint32_t* __restrict__ out_cnt, uint32_t token_offset) {
  const uint32_t token = ~(uint32_t)best + token_offset;
  if (lane < k) out_keys[(int64_t)q * CAP + lane] = (best & 0xffffffff00000000ull) | (uint64_t)(~token);
  if (lane == 0) out_cnt[q] = (uint32_t)k;
}

// exp / normalise / usage of the sorted top-k (best: rank_sort_k's result)
__device__ __forceinline__ void softmax_usage_tail(uint64_t best, int lane, int q, int k, int32_t* __restrict__ idx,
                                                   float* __restrict__ weight, unsigned long long* __restrict__ usage_fix) {
  const bool live = lane < k;
  const float score = from_orderable((uint32_t)(best >> 32));
  const uint32_t token = ~(uint32_t)best;
  const float ex = live ? expf(score) : 0.0f;
  float sum = 0.0f;
  for (int r = 0; r < k; ++r)  // sequential, like torch.sum over the sorted top-k
    sum += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ex), r));
  const float w = ex / sum;
  if (live) {
    idx[(int64_t)q * k + lane] = (int32_t)token;
    weight[(int64_t)q * k + lane] = w;
    if (usage_fix && w == w) atomicAdd(&usage_fix[token], (unsigned long long)(w * TWO40));
  }
}

}  // namespace
}  // namespace deva
