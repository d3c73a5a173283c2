// fp16 pre-filter of the memory read with exact fp32 re-scoring (VERDICT r2 "next" 3b), and the read entry points
// (deva_affinity_read ...) that choose between it and the fp32 list kernels of affinity.hip.
//
// The fused fp32 kernels of affinity.hip are bound by the fp32 matrix rate (1/16 of the f16 rate on gfx950) plus
// the VALU / LDS work of keeping exact candidate lists.  This path scores every (token, query) pair with
// v_mfma_f32_32x32x16_f16 on fp16 copies of the operands, carries a RIGOROUS error bound per score, and
// re-scores only the ~k+5 tokens per query that the bound cannot exclude with the natural-order fp32 FMA
// chain (bit-identical to v_mfma_f32_32x32x2_f32, MI355X_MICROARCH.md) -- selections, weights and usage
// counters are bit-identical to the fp32 kernels by construction, not by tolerance.
//
//   sim(n, q) = -m_n * (A - 2B + bsq),  m_n = ms_n / 8,  A = sum mk^2 qe,  B = sum mk qk qe,  bsq = sum qk^2 qe
//   P = m (A + bsq) >= 0 (needs qe >= 0: checked, else fall-back), Q = 2 m B, sim = Q - P.
//   Cauchy-Schwarz + AM-GM: sum_c |2 m mk qk qe| <= 2 m sqrt(A bsq) <= m (A + bsq) = P, so with d the relative
//   error of a product of two fp16-rounded operands (2^-10, + fp32 accumulation; d = 1.3e-3 is used) both
//   chains are off by at most d * P_true (+ an absolute term for operands below the fp16 normal range):
//       lo = Q~ - (1 + d2) P~ - ABS  <=  sim_fp32 * S  <=  Q~ - (1 - d2) P~ + ABS = hi,   d2 = 2 d / (1 - d)
//   (S = power-of-two scale of the query, see pf_query_operand; the d margin of 33 % over 2^-10 absorbs the fp32
//   round-off of the reference chain itself, ~70 * 2^-24 relative to P).
//
// Centering.  On real clips the keys share a large common component (the best-matching tokens have mk ~ qk), so
// A, B and bsq are ~200x the score they cancel to and a 2^-10 relative bound on P would let thousands of tokens
// through (measured on the 1080p clip: 480 - 6 200 candidates per query).  The distance is invariant under a
// common shift, sum qe (mk - qk)^2 = sum qe ((mk - mu) - (qk - mu))^2, so both sides are centred on the bank's mean
// key mu before they are rounded to fp16 (fp32 subtractions: relative error 2^-24 of the CENTRED value): P shrinks
// 35x on that clip and the same bound admits ~37 candidates.  The fp32 round-off of the REFERENCE chain is relative
// to its uncentred terms, P_unc <= 2 P + 4 m sum qe mu^2: the first part is inside d2, the second is the per-query
// constant E_q = 4e-5 * max m * sum_c qe_c mu_c^2 (8e-6 relative round-off of the 64-step fp32 chains x 4, + margin)
// subtracted from the filter threshold twice like ABS.
//
// Kernels (no LDS lists, no prune rounds, no workgroup barriers):
//   pf_mean     per-block partial channel sums of the bank -> mu;
//   pf_stats    max of mk^2 m, 2|mk| m, m over the bank -> power-of-two scales that put the largest operand
//               just under 2^15 (fp16 max 65 504); non-finite input -> fall-back flag;
//   pf_prep     the bank as fp16 MFMA A-operands, tile-major [tile][9 K-blocks][64 lanes][8 halfs]: every
//               operand load of the passes is one fully coalesced 1-KiB instruction;
//   pass A      group maxima of lo: per (token range, query) PF_GROUPS = 32 groups (one per token slot of the
//               tiles) of DISTINCT tokens, so the k-th largest group maximum over all ranges is a valid
//               lower bound of the k-th best score -- with 512 groups at 1080p it sits within a few per
//               cent of the true k-th best (expected ~k+2 tokens above it); 2 VALU per score;
//   pf_tau      one wave per query: k-th largest of its group maxima -> filter threshold;
//   pass B      hi >= threshold -> candidate (token, hi) into the private sub-list of the (range, query,
//               half-lane): plain predicated stores, no atomics; 2 VALU per score;
//   pf_rescore  one wave per query: gathers the candidates of all ranges (~35), re-scores each with the
//               fp32 FMA chain from its key row, selects the exact top-k on (score, index) keys and
//               finishes with the tail affinity_finalize_kernel runs (affinity_common.h: softmax, usage, or the
//               hand-over format).
// Anything the bound does not cover (negative selection, non-finite or out-of-range operands, a sub-list
// or the re-score buffer overflowing -- flat "near-tie" banks) raises a device flag and the fp32 kernels
// run as the fall-back in the same stream (they return at once when the flag is clear).
#include <math.h>

#include <type_traits>

#include "affinity_common.h"

#pragma clang fp contract(off)

namespace deva {
namespace {

typedef _Float16 h8 __attribute__((ext_vector_type(8)));

constexpr int PF_KB = 9;                      // K-blocks of 16 halfs per token: 4 (P: mk^2 m) + 1 (P: m x bsq) + 4 (Q)
constexpr int PF_TILE_BYTES = PF_KB * 64 * 16;  // [kb][lane][8 halfs]
constexpr int PF_QW = 4;                      // waves (32 queries each) per workgroup, all on the same token range
constexpr int PF_SUB = 64;                    // candidate slots per (range, query, half-lane)
constexpr int PF_MAX_SPLITS = 32;
constexpr int PF_GROUPS = 32;                 // group maxima per (range, query): one per token slot of the tiles
constexpr int PF_RESC_MAX = 2048;             // candidates re-scored per query (up to 32 rounds of 64)
constexpr float PF_D2 = 2.63e-3f;             // 2 d / (1 - d), d = 1.3e-3, + 2e-5 for the reference's fp32 round-off on 2 P
constexpr float PF_ABS = 600.0f;              // operands below 2^-14 (flushed or subnormal): 2 chains x 2^-14 x 2 x 65 x 2^15

struct PfState {     // device block, written by the prep kernel of every read
  uint32_t flag;     // != 0: the fp32 kernels take over
  uint32_t max_p;    // float bits: max (mk - mu)^2 m
  uint32_t max_q;    // max 2 |mk - mu| m
  uint32_t max_m;    // max m
  float mu[CK];      // mean key of the bank (the common shift of both operand sides)
  uint32_t bank_flag;  // the flag as the bank alone sets it (non-finite key / shrinkage): what a read on cached operands starts from
};
static_assert(sizeof(PfState) <= 512, "the state block is 512 bytes of the scratch / of a prepared-bank buffer");
constexpr float PF_EQ = 4e-5f;  // reference fp32 round-off carried by the shift: E_q = PF_EQ * max m * sum qe mu^2

// power of two P with x * P in [2^14, 2^15)
__device__ __forceinline__ float pf_scale(float x) {
  if (!(x > 0.0f) || !(x < INFINITY)) return 1.0f;
  int e;
  (void)frexpf(x, &e);  // x = f * 2^e, f in [0.5, 1)
  e = 15 - e;
  e = e > 100 ? 100 : (e < -100 ? -100 : e);
  return ldexpf(1.0f, e);
}

__device__ __forceinline__ float wave_max_f(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

constexpr int PF_STAT_BLOCKS = 256;

// grid-stride over tokens: per-block partial channel sums of the keys -> sums[block][64] (thread = channel x 4 token lanes)
__global__ __launch_bounds__(256) void affinity_pf_mean_kernel(const Bank b, float* __restrict__ sums) {
  __shared__ float s_part[4][CK];
  const int c = threadIdx.x & 63, g = threadIdx.x >> 6;
  float acc = 0.0f;
  for (int n = blockIdx.x * 4 + g; n < b.n_total; n += PF_STAT_BLOCKS * 4) {
    float ms;
    acc += bank_row(b, n, &ms)[c];
  }
  s_part[g][c] = acc;
  __syncthreads();
  if (g == 0) sums[blockIdx.x * CK + c] = (s_part[0][c] + s_part[1][c]) + (s_part[2][c] + s_part[3][c]);
}

// grid-stride over (token, 16 channels); every block first forms mu from the partial sums, then leaves its partial
// maxima of the CENTRED operands (and a bad-input mark) in part[block][4] -- no atomics, nothing to zero beforehand
__global__ __launch_bounds__(256) void affinity_pf_stats_kernel(const Bank b, const float* __restrict__ sums,
                                                                 uint32_t* __restrict__ part, float* __restrict__ mu_out) {
  __shared__ float s_red[4][4];
  __shared__ float s_mu[CK];
  if (threadIdx.x < CK) {
    float t = 0.0f;
    for (int i = 0; i < PF_STAT_BLOCKS; ++i) t += sums[i * CK + threadIdx.x];
    t = t / (float)b.n_total;
    t = (t == t && fabsf(t) < INFINITY) ? t : 0.0f;  // (non-finite banks fall back anyway)
    s_mu[threadIdx.x] = t;
    if (blockIdx.x == 0) mu_out[threadIdx.x] = t;
  }
  __syncthreads();
  float mp = 0.0f, mq = 0.0f, mm = 0.0f;
  bool bad = false;
  const int total = b.n_total * 4;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += PF_STAT_BLOCKS * 256) {
    const int n = i >> 2;
    float ms;
    const float* row = bank_row(b, n, &ms) + 16 * (i & 3);
    const float m = ms * 0.125f;
    mm = fmaxf(mm, m);
    bad = bad || !(m >= 0.0f && m < INFINITY);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(row + 4 * j);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        bad = bad || !(fabsf(v[u]) < INFINITY);
        const float a = fabsf(v[u] - s_mu[16 * (i & 3) + 4 * j + u]);
        mp = fmaxf(mp, a * a * m);
        mq = fmaxf(mq, 2.0f * a * m);
      }
    }
  }
  mp = wave_max_f(mp);
  mq = wave_max_f(mq);
  mm = wave_max_f(mm);
  bad = bad || !(mp < INFINITY) || !(mq < INFINITY);
  const float fb = __builtin_amdgcn_ballot_w64(bad) ? 1.0f : 0.0f;
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    s_red[wave][0] = mp;
    s_red[wave][1] = mq;
    s_red[wave][2] = mm;
    s_red[wave][3] = fb;
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    const float v = fmaxf(fmaxf(s_red[0][threadIdx.x], s_red[1][threadIdx.x]), fmaxf(s_red[2][threadIdx.x], s_red[3][threadIdx.x]));
    part[blockIdx.x * 4 + threadIdx.x] = __float_as_uint(v);
  }
}

// one thread per (token slot of the padded bank, half-lane): writes the 9 x 16 B this MFMA lane will load
__global__ __launch_bounds__(256) void affinity_pf_prep_kernel(const Bank b, const uint32_t* __restrict__ part,
                                                                PfState* st, PfState* keep, int n_pad, uint8_t* __restrict__ a16) {
  // every block reduces the partial maxima of the stats kernel itself (one wave); block 0 publishes
  // them together with the cleared fall-back flag for the kernels that follow in the stream
  __shared__ float s_max[4];
  if (threadIdx.x < 64) {
    const int lane = threadIdx.x;
    float v[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      float m = 0.0f;
      for (int i = lane; i < PF_STAT_BLOCKS; i += 64) m = fmaxf(m, __uint_as_float(part[i * 4 + c]));
      v[c] = wave_max_f(m);
    }
    if (lane == 0) {
#pragma unroll
      for (int c = 0; c < 4; ++c) s_max[c] = v[c];
      if (blockIdx.x == 0) {
        st->flag = st->bank_flag = v[3] > 0.0f ? 1u : 0u;
        st->max_p = __float_as_uint(v[0]);
        st->max_q = __float_as_uint(v[1]);
        st->max_m = __float_as_uint(v[2]);
      }
    }
    // a prepared-bank buffer keeps the state beside the operands: reads of the unchanged bank start from this image
    if (blockIdx.x == 0 && keep) {
      keep->mu[lane] = st->mu[lane];
      if (lane == 0) {
        keep->flag = keep->bank_flag = v[3] > 0.0f ? 1u : 0u;
        keep->max_p = __float_as_uint(v[0]);
        keep->max_q = __float_as_uint(v[1]);
        keep->max_m = __float_as_uint(v[2]);
      }
    }
  }
  __syncthreads();
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int n = i >> 1, half = i & 1;
  if (n >= n_pad) return;
  const float sp = pf_scale(s_max[0]);
  const float sq = pf_scale(s_max[1]);
  const float sm = pf_scale(s_max[2]);
  uint8_t* dst = a16 + (int64_t)(n >> 5) * PF_TILE_BYTES + ((n & 31) + 32 * half) * 16;
  h8 out[PF_KB];
#pragma unroll
  for (int kb = 0; kb < PF_KB; ++kb)
#pragma unroll
    for (int e = 0; e < 8; ++e) out[kb][e] = (_Float16)0.0f;
  if (n < b.n_total) {
    float ms;
    const float* row = bank_row(b, n, &ms);
    const float m = ms * 0.125f;
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) {
      const f32x4 v0 = *reinterpret_cast<const f32x4*>(row + 16 * kb + 8 * half);
      const f32x4 v1 = *reinterpret_cast<const f32x4*>(row + 16 * kb + 8 * half + 4);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float a = (e < 4 ? v0[e] : v1[e - 4]) - st->mu[16 * kb + 8 * half + e];  // centred on the bank's mean key
        out[kb][e] = (_Float16)(a * a * m * sp);
        out[5 + kb][e] = (_Float16)(2.0f * a * m * sq);
      }
    }
    if (half == 0) out[4][0] = (_Float16)(m * sm);
  }
#pragma unroll
  for (int kb = 0; kb < PF_KB; ++kb) *reinterpret_cast<h8*>(dst + kb * 1024) = out[kb];
}

struct PfArgs {
  const uint8_t* bq16;  // [ceil(hw/32)][9][64][8 halfs] query operands (affinity_pf_query_kernel)
  const uint8_t* a16;
  int n_total;
  int total_tiles;
  const float* qk;
  const float* qe;
  int hw;
  int splits;
  PfState* st;
  float* gmax;         // [splits][hw][32] group maxima of lo (pass A)
  const float* thr;    // [hw] filter threshold (pass B)
  uint64_t* cand;      // [hw][splits][2][PF_SUB]: hi bits << 32 | token
  uint32_t* cand_cnt;  // [hw][splits][2]
};

// The query side of the MFMAs for lane (l31, half): channel 16 kb + 8 half + e of query q, scaled by the
// per-query powers of two that bring P~ and Q~ to the common scale S_q = min over the three operand groups
// of (bank scale x largest query scale that keeps the group below 2^15).  Raises the fall-back flag for a
// negative or non-finite selection / key.
__device__ __forceinline__ void pf_query_operand(const float* __restrict__ qk, const float* __restrict__ qe, int hw, int q,
                                                 int half, const PfState* st, h8 (&bq)[PF_KB], bool* bad_out,
                                                 float* eq_out) {
  float e_[32], p_[32];
  float bsq = 0.0f, e_max = 0.0f, p_max = 0.0f, mq2 = 0.0f;
  bool bad = false;
#pragma unroll
  for (int kb = 0; kb < 4; ++kb)
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int c = 16 * kb + 8 * half + e;
      const float ev = qe[(int64_t)c * hw + q], kraw = qk[(int64_t)c * hw + q];
      const float mu_c = st->mu[c];
      const float kv = kraw - mu_c;  // centred like the bank
      mq2 += ev * (mu_c * mu_c);
      bad = bad || !(ev >= 0.0f && ev < INFINITY) || !(fabsf(kraw) < INFINITY);
      e_[8 * kb + e] = ev;
      p_[8 * kb + e] = kv * ev;
      bsq += ev * (kv * kv);
      e_max = fmaxf(e_max, ev);
      p_max = fmaxf(p_max, fabsf(kv * ev));
    }
  // both half-lanes of a query end up with the same values
  const float bsq_o = __shfl_xor(bsq, 32, 64), e_o = __shfl_xor(e_max, 32, 64), p_o = __shfl_xor(p_max, 32, 64);
  mq2 += __shfl_xor(mq2, 32, 64);
  bsq = half ? (bsq_o + bsq) : (bsq + bsq_o);
  e_max = fmaxf(e_max, e_o);
  p_max = fmaxf(p_max, p_o);
  bad = bad || !(bsq < INFINITY) || !(p_max < INFINITY);
  const float sp = pf_scale(__uint_as_float(st->max_p));
  const float sq = pf_scale(__uint_as_float(st->max_q));
  const float sm = pf_scale(__uint_as_float(st->max_m));
  const float S = fminf(fminf(sp * pf_scale(e_max), sq * pf_scale(p_max)), sm * pf_scale(bsq));
  const float te = S / sp, tp = S / sq, tb = S / sm;  // powers of two: exact
#pragma unroll
  for (int kb = 0; kb < 4; ++kb)
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      bq[kb][e] = (_Float16)(e_[8 * kb + e] * te);
      bq[5 + kb][e] = (_Float16)(p_[8 * kb + e] * tp);
    }
#pragma unroll
  for (int e = 0; e < 8; ++e) bq[4][e] = (_Float16)0.0f;
  if (half == 0) bq[4][0] = (_Float16)(bsq * tb);
  *bad_out = bad || !(mq2 < INFINITY);
  *eq_out = PF_EQ * __uint_as_float(st->max_m) * mq2 * S;  // in the query's scaled units, like ABS
}

// one wave per 32 queries: the fp16 query operands of both passes, computed ONCE per read (every (range, pass) wave
// used to rebuild them: 64 strided loads and the scale logic per query group, which at ~20 tiles per wave cost as
// much as the tiles).  Layout like the bank operand: [query group][9 K-blocks][64 lanes][8 halfs].
// `src`: where the bank's state is read from -- the scratch's own block (`st`, just written by the prep kernel) or, on a read
// of cached bank operands, the image in the prepared-bank buffer, which workgroup 0 then copies to the scratch for the
// kernels that follow (round 5 had a one-wave launch of its own for that copy).  A bad query does not touch st->flag here
// (workgroup 0 may be writing it): every query group leaves its mark in qbad[group], which the check kernel -- the next
// writer of the flag, ahead of all its readers -- folds in.
__global__ __launch_bounds__(256) void affinity_pf_query_kernel(const float* __restrict__ qk, const float* __restrict__ qe,
                                                                 int hw, const PfState* __restrict__ src, PfState* st,
                                                                 uint8_t* __restrict__ bq16, float* __restrict__ eq,
                                                                 uint32_t* __restrict__ qbad) {
  const int lane = threadIdx.x & 63;
  const int group = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (src != st && blockIdx.x == 0 && threadIdx.x < 64) {
    st->mu[lane] = src->mu[lane];
    if (lane == 0) {
      st->flag = st->bank_flag = src->bank_flag;
      st->max_p = src->max_p;
      st->max_q = src->max_q;
      st->max_m = src->max_m;
    }
  }
  const int q0 = group * QT;
  if (q0 >= hw) return;
  const int l31 = lane & 31, half = lane >> 5;
  h8 bq[PF_KB];
  bool bad;
  float e_q;
  pf_query_operand(qk, qe, hw, min(q0 + l31, hw - 1), half, src, bq, &bad, &e_q);
  const bool any_bad = __builtin_amdgcn_ballot_w64(bad && q0 + l31 < hw) != 0;
  if (lane == 0) qbad[group] = any_bad ? 1u : 0u;
  if (half == 0 && q0 + l31 < hw) eq[q0 + l31] = e_q;
  uint8_t* dst = bq16 + (int64_t)group * PF_TILE_BYTES + lane * 16;
#pragma unroll
  for (int kb = 0; kb < PF_KB; ++kb) *reinterpret_cast<h8*>(dst + kb * 1024) = bq[kb];
}

// PASS 0: group maxima of lo; PASS 1: candidates with hi >= threshold.
// QG query groups (of 32) per wave share every token tile the wave loads: the vector-memory path delivers 64 B per
// clock and CU, a 32x32x16 MFMA (32 clocks) consumes a 1-KiB A fragment, so with one query group per wave the
// passes are bound by operand delivery at ~3x the matrix time (measured: 840 clocks per tile against 288 of
// MFMAs); two groups halve the operand bytes per MFMA.  Small frames keep QG = 1 (more workgroups).
template <int PASS, int QG>
__global__ __launch_bounds__(PF_QW * 64, 2) void affinity_pf_pass_kernel(const PfArgs p) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int l31 = lane & 31;
  const int half = lane >> 5;
  const int q0 = (blockIdx.x * PF_QW + wave) * (QT * QG);
  if (q0 >= p.hw) return;
  const int split = blockIdx.y;
  h8 bq[QG][PF_KB];
  bool q_ok[QG];
  int q[QG];
  float thr[QG];
  uint32_t ccnt[QG];
  uint64_t* my_list[QG];
  float g[QG][16];
#pragma unroll
  for (int u = 0; u < QG; ++u) {
    q_ok[u] = q0 + QT * u + l31 < p.hw;
    q[u] = min(q0 + QT * u + l31, p.hw - 1);
    // (a query group past the end of the frame re-reads the last one: its results are discarded)
    const int group = min(q0 / QT + u, (p.hw - 1) / QT);
    const uint8_t* src = p.bq16 + (int64_t)group * PF_TILE_BYTES + lane * 16;
#pragma unroll
    for (int kb = 0; kb < PF_KB; ++kb) bq[u][kb] = *reinterpret_cast<const h8*>(src + kb * 1024);
    // a lane without a query (ragged last group) must never file a candidate into the clamped query's sub-list
    thr[u] = PASS ? (q_ok[u] ? p.thr[q[u]] : INFINITY) : 0.0f;
    ccnt[u] = 0u;
    my_list[u] = p.cand + (((int64_t)q[u] * p.splits + split) * 2 + half) * PF_SUB;
#pragma unroll
    for (int r = 0; r < 16; ++r) g[u][r] = -INFINITY;
  }

  // token ranges are TILE-CYCLIC (range s owns tiles s, s + S, ...): a video memory holds the same location once per
  // memory frame, hw tokens apart -- with contiguous ranges those near-duplicates (the best matches of a query) share
  // one (range, slot) group, whose single maximum then says little about the k-th best, and one half-lane sub-list
  const int n_my = (p.total_tiles - split + p.splits - 1) / p.splits;
  const int t0 = 0, t1 = n_my;  // visit index; tile = split + visit * splits
  const uint8_t* mine = p.a16 + lane * 16;
  auto load = [&](h8 (&x)[PF_KB], int visit) __attribute__((always_inline)) {
    const uint8_t* base = mine + (int64_t)(split + visit * p.splits) * PF_TILE_BYTES;
#pragma unroll
    for (int kb = 0; kb < PF_KB; ++kb) x[kb] = *reinterpret_cast<const h8*>(base + kb * 1024);
  };
  const float c_lo = -(1.0f + PF_D2), c_hi = -(1.0f - PF_D2);

  // full: every token slot of the tile is inside the bank (all tiles but possibly the last one of the bank)
  auto process = [&](const h8 (&x)[PF_KB], int visit, auto full) __attribute__((always_inline)) {
    constexpr bool full_tile = decltype(full)::value;
    const int tile = split + visit * p.splits;
    const int rows_left = p.n_total - tile * TOKT;
    const uint32_t tok0 = (uint32_t)(tile * TOKT + 4 * half);
#pragma unroll
    for (int u = 0; u < QG; ++u) {
      f32x16 accP, accQ;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        accP[r] = 0.0f;
        accQ[r] = 0.0f;
      }
#pragma unroll
      for (int kb = 0; kb < 5; ++kb) accP = __builtin_amdgcn_mfma_f32_32x32x16_f16(x[kb], bq[u][kb], accP, 0, 0, 0);
#pragma unroll
      for (int kb = 5; kb < PF_KB; ++kb) accQ = __builtin_amdgcn_mfma_f32_32x32x16_f16(x[kb], bq[u][kb], accQ, 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int j0 = (r & 3) + 8 * (r >> 2);  // + 4 * half: token slot of accumulator row r
        if (PASS == 0) {
          float lo = __builtin_fmaf(accP[r], c_lo, accQ[r]);
          if (!full_tile && j0 + 4 * half >= rows_left) lo = -INFINITY;
          // plain v_max_f32 (fmaxf would first canonicalise both inputs: one more VALU instruction per score)
          asm("v_max_f32 %0, %1, %2" : "=v"(g[u][r]) : "v"(g[u][r]), "v"(lo));
        } else {
          const float hi = __builtin_fmaf(accP[r], c_hi, accQ[r]);
          bool ok = hi >= thr[u];
          if (!full_tile) ok = ok && (j0 + 4 * half < rows_left);
          if (ok) {
            if (ccnt[u] < (uint32_t)PF_SUB)
              my_list[u][ccnt[u]] = ((uint64_t)__float_as_uint(hi) << 32) | (uint64_t)(tok0 + j0);
            ccnt[u] += 1u;
          }
        }
      }
      // one accumulator set: the next group's MFMAs must not be hoisted above this group's scoring (two sets in
      // flight push pass A over the 256-register budget of two waves per SIMD -> scratch spills)
      if (PASS == 0 && QG > 1) __builtin_amdgcn_sched_barrier(0);
    }
  };

  // the bank's ragged last tile (if this range holds it) is peeled off the loop
  const bool ragged = (n_my > 0) && (split + (n_my - 1) * p.splits == p.total_tiles - 1) && (p.n_total % TOKT != 0);
  const int t1f = ragged ? t1 - 1 : t1;
  h8 xa[PF_KB], xb[PF_KB];
  int t = t0;
  if (t < t1f) load(xa, t);
  while (t < t1f) {
    // (a workgroup barrier here, to keep the four waves on the same tile so that the L1 could merge their operand
    // loads, was measured: 130.9 vs 128.3 us at 10 000 x 8 160 -- the passes are not bound by L2 bandwidth)
    if (t + 1 < t1f) load(xb, t + 1);
    process(xa, t, std::true_type{});
    if (t + 1 >= t1f) break;
    if (t + 2 < t1f) load(xa, t + 2);
    process(xb, t + 1, std::true_type{});
    t += 2;
  }
  if (ragged) {
    load(xa, t1f);
    process(xa, t1f, std::false_type{});
  }

#pragma unroll
  for (int u = 0; u < QG; ++u) {
    if (!q_ok[u]) continue;
    if (PASS == 0) {
      float* dst = p.gmax + ((int64_t)split * p.hw + q[u]) * PF_GROUPS;
#pragma unroll
      for (int r = 0; r < 16; ++r) dst[(r & 3) + 8 * (r >> 2) + 4 * half] = g[u][r];
    } else {
      p.cand_cnt[((int64_t)q[u] * p.splits + split) * 2 + half] = ccnt[u];
      if (ccnt[u] > (uint32_t)PF_SUB) atomicOr(&p.st->flag, 4u);
    }
  }
}

// one wave per query: threshold = the k-th largest of its splits x 32 group maxima, resolved to the top 18 bits of
// the order-preserving score bits (rounded DOWN: still a valid lower bound, at most 2^-9 relative below the exact
// value -- a fraction of the bound's own width --, usually exact through the early exit) minus the absolute slack
constexpr int PF_TAU_E = PF_MAX_SPLITS * PF_GROUPS / 64;
__global__ __launch_bounds__(256) void affinity_pf_tau_kernel(const float* __restrict__ gmax, const float* __restrict__ eq,
                                                              int hw, int k, int splits, float* __restrict__ thr) {
  const int lane = threadIdx.x & 63;
  const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= hw) return;
  const int total = splits * PF_GROUPS;
  uint32_t e[PF_TAU_E];
#pragma unroll
  for (int i = 0; i < PF_TAU_E; ++i) {
    const int gi = i * 64 + lane;
    uint32_t key = 0u;
    if (gi < total) {
      float v = gmax[((int64_t)(gi / PF_GROUPS) * hw + q) * PF_GROUPS + (gi % PF_GROUPS)];
      v = (v == v) ? v : -INFINITY;
      key = orderable(v);
    }
    e[i] = key;
  }
  const int n_live = (total + 63) / 64;
  uint32_t T = 0u;
  for (int b = 31; b >= 14; --b) {
    const uint32_t trial = T | (1u << b);
    int cnt = 0;
#pragma unroll
    for (int i = 0; i < PF_TAU_E; ++i)
      if (i < n_live) cnt += wave_count(e[i] >= trial);
    if (cnt >= k) {
      T = trial;
      if (cnt == k) break;  // separates exactly k groups: the remaining bits cannot raise it past the k-th value
    }
  }
  // T == 0 (fewer than k groups hold tokens): -inf, every score becomes a candidate and the sub-lists overflow
  if (lane == 0) thr[q] = (T == 0u ? -INFINITY : from_orderable(T)) - 2.0f * (PF_ABS + eq[q]);
}

// Candidate totals per query, checked BEFORE the re-score kernel commits anything: a query with more candidates than
// the re-score buffer holds (or fewer than k) raises the fall-back flag here, so that the re-score kernel -- which
// writes idx / weight and adds to the usage counters -- either runs for every query or for none (it reads the flag
// at entry; raised from inside it, the flag let earlier workgroups' usage additions stand and the fp32 fall-back
// counted those queries twice).
__global__ __launch_bounds__(256) void affinity_pf_check_kernel(const uint32_t* __restrict__ cand_cnt, int hw, int k,
                                                                int n_sub, const uint32_t* __restrict__ qbad, PfState* st) {
  const int q = blockIdx.x * 256 + threadIdx.x;
  bool bad = false, bad_query = false;
  if (q < hw) {
    const uint32_t* c = cand_cnt + (int64_t)q * n_sub;
    uint32_t total = 0u;
    for (int i = 0; i < n_sub; ++i) total += c[i] < (uint32_t)PF_SUB ? c[i] : (uint32_t)PF_SUB;
    bad = total > (uint32_t)PF_RESC_MAX || total < (uint32_t)k;
    bad_query = qbad[q / QT] != 0u;  // a negative / non-finite selection or key in the query's group (affinity_pf_query_kernel)
  }
  const uint32_t bits = (__builtin_amdgcn_ballot_w64(bad) ? 8u : 0u) | (__builtin_amdgcn_ballot_w64(bad_query) ? 2u : 0u);
  if (bits && (threadIdx.x & 63) == 0) atomicOr(&st->flag, bits);
}

struct PfRescoreArgs {
  Bank bank;
  const float* qk;
  const float* qe;
  int hw;
  int k;
  int splits;
  PfState* st;
  const uint64_t* cand;
  const uint32_t* cand_cnt;
  int32_t* idx;
  float* weight;
  unsigned long long* usage_fix;
  uint64_t* out_keys;
  uint32_t* out_cnt;
  uint32_t token_offset;
};

// one wave per query (four queries per workgroup): gather candidates, exact fp32 scores (the FMA chain of
// v_mfma_f32_32x32x2_f32: channels in natural order, mk^2 rounded before it enters the chain, qk*qe rounded
// likewise), exact top-k, softmax / usage
__global__ __launch_bounds__(256) void affinity_pf_rescore_kernel(const PfRescoreArgs p) {
  __shared__ uint64_t s_key[4][PF_RESC_MAX];  // candidate tokens, overwritten in place by their exact (score, token) keys
  __shared__ __attribute__((aligned(16))) float s_qe[4][CK];
  __shared__ __attribute__((aligned(16))) float s_qp[4][CK];
  __shared__ float s_term[4][CK];
  __shared__ uint64_t s_buf[4][2][64];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int q = blockIdx.x * 4 + wave;
  const int k = p.k;
  {  // the four queries' operands, loaded by the whole workgroup: 16 B per channel row instead of 4 x 4 B
    const int c = threadIdx.x >> 2, jq = threadIdx.x & 3;
    const int qq = min(blockIdx.x * 4 + jq, p.hw - 1);
    const float ev = p.qe[(int64_t)c * p.hw + qq], kv = p.qk[(int64_t)c * p.hw + qq];
    s_qe[jq][c] = ev;
    s_qp[jq][c] = kv * ev;
    s_term[jq][c] = ev * (kv * kv);
  }
  __syncthreads();
  if (q >= p.hw) return;
  if (p.st->flag != 0u) return;  // the fp32 kernels produce this read

  // ---- bsq in ATen's summation order: four 16-channel partial sums (one per lane 0..3), then ((s0+s1)+s2)+s3
  float part = 0.0f;
  if (lane < 4) {
#pragma unroll
    for (int c = 0; c < 16; ++c) part += s_term[wave][16 * lane + c];
  }
  const float bs0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(part), 0));
  const float bs1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(part), 1));
  const float bs2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(part), 2));
  const float bs3 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(part), 3));
  const float bsq = ((bs0 + bs1) + bs2) + bs3;

  // ---- gather: lane l owns sub-list l = (range, half-lane) of this query (<= 64 of them); its entries go to
  // s_tok[prefix(l) .. prefix(l) + count(l))
  const int n_sub = p.splits * 2;
  const int64_t sub0 = (int64_t)q * n_sub;
  uint32_t mine = 0u;
  if (lane < n_sub) {
    mine = p.cand_cnt[sub0 + lane];
    mine = mine < (uint32_t)PF_SUB ? mine : (uint32_t)PF_SUB;
  }
  uint32_t incl = mine;  // inclusive prefix sum over the lanes
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t up = (uint32_t)__shfl_up((int)incl, o, 64);
    if (lane >= o) incl += up;
  }
  const int total = __builtin_amdgcn_readlane((int)incl, 63);
  const uint32_t base = incl - mine;
  uint32_t longest = mine;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const uint32_t other = (uint32_t)__shfl_xor((int)longest, o, 64);
    longest = other > longest ? other : longest;
  }
  if (total > PF_RESC_MAX || total < k) return;  // unreachable: affinity_pf_check_kernel raised the flag (same totals)
  const uint64_t* my_sub = p.cand + (sub0 + lane) * PF_SUB;
  for (uint32_t s0 = 0; s0 < longest; s0 += 4) {  // four independent loads in flight per lane
    uint64_t ent[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) ent[u] = (s0 + u < mine) ? my_sub[s0 + u] : 0ull;
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (s0 + u < mine) s_key[wave][base + s0 + u] = ent[u] & 0xffffffffull;
  }
  DEVA_COMPILER_FENCE();

  // ---- exact scores, 64 candidates per round (a real loop: the keys go to LDS, the registers of a round are reused)
  for (int r0 = 0; r0 < total; r0 += 64) {
    const int c = r0 + lane;
    const bool live_c = c < total;
    const uint32_t tok = live_c ? (uint32_t)s_key[wave][c] : 0u;
    float ms;
    const float* row = bank_row(p.bank, (int)tok, &ms);
    const float v = score_fp32(row, reinterpret_cast<const f32x4*>(&s_qe[wave][0]),
                               reinterpret_cast<const f32x4*>(&s_qp[wave][0]), bsq, ms);
    s_key[wave][c] = live_c ? (((uint64_t)orderable(v) << 32) | (uint64_t)(~tok)) : 0ull;
  }
  DEVA_COMPILER_FENCE();
  const int rounds = (total + 63) / 64;
  uint64_t e[PF_RESC_MAX / 64];
#pragma unroll
  for (int rr = 0; rr < PF_RESC_MAX / 64; ++rr) e[rr] = (rr < rounds) ? s_key[wave][rr * 64 + lane] : 0ull;
  volatile uint64_t* unsorted = &s_buf[wave][0][0];
  volatile uint64_t* sorted = &s_buf[wave][1][0];
  uint64_t best;  // lane r: the r-th best key
  if (total <= 64) {
    // one round (the usual case): rank counting over the <= 64 unique keys selects AND sorts
    best = rank_sort_k(e[0], total, k, lane, sorted);
  } else {
    const uint64_t thr = kth_largest<PF_RESC_MAX / 64>(e, rounds, k);
    int base_k = 0;
#pragma unroll
    for (int i = 0; i < PF_RESC_MAX / 64; ++i) {
      if (i < rounds) {
        const bool keep = e[i] >= thr && e[i] != 0ull;
        const unsigned long long b = __builtin_amdgcn_ballot_w64(keep);
        if (keep) unsorted[base_k + prefix_below(b)] = e[i];
        base_k += __popcll(b);
      }
    }
    DEVA_COMPILER_FENCE();
    const uint64_t cand = (lane < k && lane < base_k) ? unsorted[lane] : missing_slot_key(lane);
    best = rank_sort_k(cand, k, k, lane, sorted);
  }
  if (p.out_keys) {
    write_out_keys(best, lane, q, k, p.out_keys, p.out_cnt, p.token_offset);
    return;
  }
  softmax_usage_tail(best, lane, q, k, p.idx, p.weight, p.usage_fix);
}

}  // namespace
}  // namespace deva

using namespace deva;

static int g_prefilter = -1;  // -1: DEVA_AFFINITY_PREFILTER not read yet; 0 = never, 1 = automatic (default)
// below these the six launches cost more than the fp32 kernels need (profiles/r03_affinity_read.txt: 65 vs 40 us at
// 2 048 x 1 620, 81 vs 89 us at 10 000 x 1 620 before the query operands were hoisted)
constexpr int PF_MIN_TOKENS = 4096;
constexpr int64_t PF_MIN_SCORES = 8000000;

static int pf_qg(int hw) { return hw >= 4096 ? 2 : 1; }  // query groups per wave (large frames: half the operand traffic)

static int pf_splits(int n_total, int hw) {
  const int tiles = (int)ceil_div(n_total, TOKT);
  const int qblocks = (int)ceil_div(hw, PF_QW * QT * pf_qg(hw));
  int s = (int)ceil_div(512, qblocks);  // two 4-wave workgroups per CU
  // >= 16 tile-cyclic ranges: 512 groups per query keep the k-th largest group maximum tight, and the near-duplicate
  // tokens of consecutive memory frames spread over the ranges (measured on the 4K clip: 5 ranges -> sub-lists of 185)
  if (s < 16) s = 16;
  if (s > tiles / 2) s = tiles / 2;     // >= 2 tiles per range
  if (s > PF_MAX_SPLITS) s = PF_MAX_SPLITS;
  if (s < 1) s = 1;
  return s;
}

struct PfLayout {
  int splits, tiles, old_splits;
  int64_t off_state, off_a16, off_bq16, off_gmax, off_thr, off_eq, off_cand, off_cnt, off_part, bytes;
};

static PfLayout pf_layout(int n_total, int hw, int k) {
  PfLayout L;
  L.splits = pf_splits(n_total, hw);
  L.tiles = (int)ceil_div(n_total, TOKT);
  L.old_splits = deva_affinity_default_splits(n_total, hw);
  auto align = [](int64_t b) { return (b + 255) / 256 * 256; };
  int64_t o = 0;
  L.off_state = o;
  o += 512 + PF_STAT_BLOCKS * 16 + PF_STAT_BLOCKS * CK * 4;  // PfState | [blocks][4] partial maxima | [blocks][64] channel sums
  L.off_a16 = o;
  o += align((int64_t)L.tiles * PF_TILE_BYTES);
  L.off_bq16 = o;
  o += align(ceil_div(hw, QT) * PF_TILE_BYTES);
  L.off_gmax = o;
  o += align((int64_t)L.splits * hw * PF_GROUPS * 4);
  L.off_thr = o;
  o += align((int64_t)hw * 4);
  L.off_eq = o;
  o += align((int64_t)hw * 4);
  L.off_cand = o;
  o += align((int64_t)L.splits * hw * 2 * PF_SUB * 8);
  L.off_cnt = o;
  o += align((int64_t)L.splits * hw * 2 * 4);
  L.off_part = o;
  o += align(deva_affinity_workspace(hw, k, L.old_splits) * 8);
  L.bytes = o;
  return L;
}

extern "C" int deva_affinity_prefilter_enabled(int n_total, int hw, int k) {
  if (g_prefilter < 0) {
    const char* e = getenv("DEVA_AFFINITY_PREFILTER");
    g_prefilter = (e && atoi(e) == 0) ? 0 : 1;
  }
  return g_prefilter && n_total >= PF_MIN_TOKENS && (int64_t)n_total * hw >= PF_MIN_SCORES && k >= 1 && k <= K_MAX;
}

extern "C" int deva_affinity_force_prefilter(int mode) {
  DEVA_REQUIRE(mode == 0 || mode == 1, "deva_affinity_force_prefilter: 0 = fp32 kernels only, 1 = automatic");
  g_prefilter = mode;
  return 0;
}

extern "C" int64_t deva_affinity_read_scratch(int n_total, int hw, int k) {
  if (k > K_MAX) return 64;  // the dense kernel (32 < k <= 64) needs no scratch; a token size keeps callers uniform
  return pf_layout(n_total, hw, k).bytes / 8;
}

extern "C" int64_t deva_affinity_bank_prep_bytes(int n_total) {
  if (n_total <= 0) return 512;
  return 512 + (ceil_div(n_total, TOKT) * (int64_t)PF_TILE_BYTES + 255) / 256 * 256;
}

extern "C" int deva_affinity_read(const float* key_long, const float* shr_long, int n_long, const float* key_work,
                                  const float* shr_work, int n_work, const float* qk, const float* qe, int hw, int k,
                                  uint64_t* scratch, int32_t* idx, float* weight, uint64_t* usage_fix,
                                  uint64_t* out_keys, uint32_t* out_counts, int64_t token_offset, void* stream) {
  return deva_affinity_read_prepared(key_long, shr_long, n_long, key_work, shr_work, n_work, qk, qe, hw, k, scratch, idx, weight,
                                     usage_fix, out_keys, out_counts, token_offset, nullptr, 0, stream);
}

extern "C" int deva_affinity_read_prepared(const float* key_long, const float* shr_long, int n_long, const float* key_work,
                                           const float* shr_work, int n_work, const float* qk, const float* qe, int hw, int k,
                                           uint64_t* scratch, int32_t* idx, float* weight, uint64_t* usage_fix,
                                           uint64_t* out_keys, uint32_t* out_counts, int64_t token_offset,
                                           uint64_t* bank_prep, int bank_prep_valid, void* stream) {
  DEVA_REQUIRE(qk && qe && scratch && hw > 0, "deva_affinity_read: bad query args");
  DEVA_REQUIRE((idx && weight && !out_keys && !out_counts) || (out_keys && out_counts && !idx && !weight && !usage_fix),
               "deva_affinity_read: pass either idx + weight (+ usage_fix) or out_keys + out_counts");
  DEVA_REQUIRE(n_long >= 0 && n_work >= 0, "deva_affinity_read: negative bank size");
  DEVA_REQUIRE(n_long == 0 || (key_long && shr_long), "deva_affinity_read: null long-term segment");
  DEVA_REQUIRE(n_work == 0 || (key_work && shr_work), "deva_affinity_read: null working segment");
  if (k > K_MAX) {  // beyond the list kernels: one dense kernel, no hand-over format (a token-sharded bank cannot use it)
    DEVA_REQUIRE(idx && weight, "deva_affinity_read: k=%d > %d is served by the dense kernel, which has no hand-over format "
                 "(out_keys / out_counts)", k, K_MAX);
    return deva_affinity_dense(key_long, shr_long, n_long, key_work, shr_work, n_work, qk, qe, hw, k, idx, weight, usage_fix,
                               stream);
  }
  DEVA_REQUIRE(k >= 1, "deva_affinity_read: k=%d unsupported", k);
  const int64_t n_total = (int64_t)n_long + n_work;
  DEVA_REQUIRE(n_total >= k, "deva_affinity_read: selected index k out of range (bank has %lld tokens, k=%d)",
               (long long)n_total, k);
  DEVA_REQUIRE(n_total < (1ll << 31) - 64, "deva_affinity_read: bank too large");
  DEVA_REQUIRE(token_offset >= 0 && token_offset < (1ll << 31), "deva_affinity_read: bad token offset");
  hipStream_t st = (hipStream_t)stream;
  const PfLayout L = pf_layout((int)n_total, hw, k);
  uint8_t* base = reinterpret_cast<uint8_t*>(scratch);
  PfState* state = reinterpret_cast<PfState*>(base + L.off_state);
  uint64_t* part = reinterpret_cast<uint64_t*>(base + L.off_part);

  if (deva_affinity_prefilter_enabled((int)n_total, hw, k)) {
    const Bank b = make_bank(key_long, shr_long, n_long, key_work, shr_work, n_total);
    uint32_t* stat_part = reinterpret_cast<uint32_t*>(base + L.off_state + 512);  // [PF_STAT_BLOCKS][4], after the state
    float* sums = reinterpret_cast<float*>(base + L.off_state + 512 + PF_STAT_BLOCKS * 16);  // [PF_STAT_BLOCKS][64]
    // the bank side of the operands (mean key, scales, fp16 fragments) depends on the bank alone: with a prepared-bank
    // buffer it lives there, and a read that the caller declares to be on the UNCHANGED bank (same rows, same n_long /
    // n_work as the read that filled the buffer) skips the three bank kernels
    uint8_t* const a16 = bank_prep ? reinterpret_cast<uint8_t*>(bank_prep) + 512 : base + L.off_a16;
    PfState* const keep = bank_prep ? reinterpret_cast<PfState*>(bank_prep) : nullptr;
    const bool cached = keep && bank_prep_valid;
    if (!cached) {
      hipLaunchKernelGGL(affinity_pf_mean_kernel, dim3(PF_STAT_BLOCKS), dim3(256), 0, st, b, sums);
      hipLaunchKernelGGL(affinity_pf_stats_kernel, dim3(PF_STAT_BLOCKS), dim3(256), 0, st, b, sums, stat_part, state->mu);
      const int n_pad = L.tiles * TOKT;
      hipLaunchKernelGGL(affinity_pf_prep_kernel, dim3((unsigned)ceil_div((int64_t)n_pad * 2, 256)), dim3(256), 0, st, b,
                         stat_part, state, keep, n_pad, a16);
    }
    // (the channel sums are dead once the prep kernel has run: their block holds the query groups' bad-input marks)
    uint32_t* const qbad = reinterpret_cast<uint32_t*>(sums);
    DEVA_REQUIRE(ceil_div(hw, QT) <= PF_STAT_BLOCKS * CK, "deva_affinity_read: frame too large for the pre-filter's scratch");
    hipLaunchKernelGGL(affinity_pf_query_kernel, dim3((unsigned)ceil_div(hw, 4 * QT)), dim3(256), 0, st, qk, qe, hw,
                       cached ? keep : state, state, base + L.off_bq16, reinterpret_cast<float*>(base + L.off_eq), qbad);
    PfArgs a;
    a.bq16 = base + L.off_bq16;
    a.a16 = a16;
    a.n_total = (int)n_total;
    a.total_tiles = L.tiles;
    a.qk = qk;
    a.qe = qe;
    a.hw = hw;
    a.splits = L.splits;
    a.st = state;
    a.gmax = reinterpret_cast<float*>(base + L.off_gmax);
    a.thr = reinterpret_cast<const float*>(base + L.off_thr);
    a.cand = reinterpret_cast<uint64_t*>(base + L.off_cand);
    a.cand_cnt = reinterpret_cast<uint32_t*>(base + L.off_cnt);
    const int qg = pf_qg(hw);
    const dim3 grid((unsigned)ceil_div(hw, PF_QW * QT * qg), (unsigned)L.splits);
    if (qg == 2) {
      hipLaunchKernelGGL((affinity_pf_pass_kernel<0, 2>), grid, dim3(PF_QW * 64), 0, st, a);
    } else {
      hipLaunchKernelGGL((affinity_pf_pass_kernel<0, 1>), grid, dim3(PF_QW * 64), 0, st, a);
    }
    hipLaunchKernelGGL(affinity_pf_tau_kernel, dim3((unsigned)ceil_div(hw, 4)), dim3(256), 0, st, a.gmax,
                       reinterpret_cast<const float*>(base + L.off_eq), hw, k, L.splits,
                       reinterpret_cast<float*>(base + L.off_thr));
    if (qg == 2) {
      hipLaunchKernelGGL((affinity_pf_pass_kernel<1, 2>), grid, dim3(PF_QW * 64), 0, st, a);
    } else {
      hipLaunchKernelGGL((affinity_pf_pass_kernel<1, 1>), grid, dim3(PF_QW * 64), 0, st, a);
    }
    hipLaunchKernelGGL(affinity_pf_check_kernel, dim3((unsigned)ceil_div(hw, 256)), dim3(256), 0, st, a.cand_cnt, hw, k,
                       L.splits * 2, qbad, state);
    PfRescoreArgs r;
    r.bank = b;
    r.qk = qk;
    r.qe = qe;
    r.hw = hw;
    r.k = k;
    r.splits = L.splits;
    r.st = state;
    r.cand = a.cand;
    r.cand_cnt = a.cand_cnt;
    r.idx = idx;
    r.weight = weight;
    r.usage_fix = (unsigned long long*)usage_fix;
    r.out_keys = out_keys;
    r.out_cnt = out_counts;
    r.token_offset = (uint32_t)token_offset;
    hipLaunchKernelGGL(affinity_pf_rescore_kernel, dim3((unsigned)ceil_div(hw, 4)), dim3(256), 0, st, r);
    if (check_launch("deva_affinity_read (pre-filter)")) return 1;
    // fall-back: the fp32 kernels, which return at once while the flag is clear
    if (int rc = topk_fp32(key_long, shr_long, n_long, key_work, shr_work, n_work, qk, qe, hw, k, L.old_splits, part, stream,
                           &state->flag))
      return rc;
    const uint32_t* cnt = reinterpret_cast<const uint32_t*>(part + (int64_t)L.old_splits * hw * CAP);
    return launch_merge(part, cnt, hw, k, L.old_splits, idx, weight, usage_fix, out_keys, out_counts, (uint32_t)token_offset,
                        stream, "deva_affinity_read (fall-back)", &state->flag);
  }
  if (int rc = topk_fp32(key_long, shr_long, n_long, key_work, shr_work, n_work, qk, qe, hw, k, L.old_splits, part, stream,
                         nullptr))
    return rc;
  const uint32_t* cnt = reinterpret_cast<const uint32_t*>(part + (int64_t)L.old_splits * hw * CAP);
  return launch_merge(part, cnt, hw, k, L.old_splits, idx, weight, usage_fix, out_keys, out_counts, (uint32_t)token_offset,
                      stream, "deva_affinity_read");
}

// test hook: the fall-back flag of the last deva_affinity_read on this scratch (device -> host copy, synchronises)
extern "C" int deva_affinity_read_flag(const uint64_t* scratch, void* stream) {
  uint32_t flag = 0;
  if (hipMemcpyAsync(&flag, scratch, sizeof(flag), hipMemcpyDeviceToHost, (hipStream_t)stream) != hipSuccess) return -1;
  if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) return -1;
  return (int)flag;
}

// test / tuning hook: candidate statistics of the last pre-filtered read on `scratch` (synchronises the stream):
// out[0] = fall-back flag, out[1] = largest sub-list count (capacity PF_SUB = 64 per (range, query, half-lane)), out[2] = largest
// number of candidates of one query, out[3] = mean candidates per query x 1000, out[4] = ranges (splits)
extern "C" int deva_affinity_read_stats(const uint64_t* scratch, int n_total, int hw, int k, int64_t* out, void* stream) {
  DEVA_REQUIRE(scratch && out && hw > 0, "deva_affinity_read_stats: bad args");
  const PfLayout L = pf_layout(n_total, hw, k);
  const uint8_t* base = reinterpret_cast<const uint8_t*>(scratch);
  const size_t n_cnt = (size_t)L.splits * hw * 2;
  uint32_t* host = (uint32_t*)malloc(n_cnt * sizeof(uint32_t));
  uint32_t flag = 0;
  if (!host) return 1;
  hipStream_t st = (hipStream_t)stream;
  bool ok = hipMemcpyAsync(&flag, base + L.off_state, 4, hipMemcpyDeviceToHost, st) == hipSuccess &&
            hipMemcpyAsync(host, base + L.off_cnt, n_cnt * 4, hipMemcpyDeviceToHost, st) == hipSuccess &&
            hipStreamSynchronize(st) == hipSuccess;
  if (ok) {
    uint32_t max_sub = 0, max_q = 0;
    uint64_t total = 0;
    for (int q = 0; q < hw; ++q) {
      uint32_t sum = 0;
      for (int s = 0; s < L.splits * 2; ++s) {
        const uint32_t c = host[(size_t)q * L.splits * 2 + s];
        max_sub = c > max_sub ? c : max_sub;
        sum += c;
      }
      max_q = sum > max_q ? sum : max_q;
      total += sum;
    }
    out[0] = flag;
    out[1] = max_sub;
    out[2] = max_q;
    out[3] = (int64_t)(total * 1000 / (uint64_t)hw);
    out[4] = L.splits;
  }
  free(host);
  return ok ? 0 : 1;
}
