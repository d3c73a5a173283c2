// Full-softmax memory read of DEVA on gfx950 (top_k = None: the reference's do_softmax without top-k,
// memory_utils.py:48-76): p[n][q] = exp(s[n][q] - max_n s[.][q]) / sum_n exp(s[n][q] - max), the usage
// counters usage[n] = sum_q p[n][q], and the read-out out[o][c][q] = sum_n V_o[n][c] * p[n][q] of every object.
//
// Scores are the natural-order fp32 values of the list kernels (affinity_topk_kernel / affinity_pf_rescore_kernel):
// A = sum_c mk^2 qe and B = sum_c mk (qk qe) as v_mfma_f32_32x32x2_f32 chains over the channels in natural order,
// bsq in ATen's summation order, v = ((2B - A) - bsq) * (ms / 8).  Four kernels per read, none of which holds the
// N x HW matrix whole:
//   dense_stats_kernel    pass 1: per query and token range, the running max and sum exp(s - max) with online
//                         rescaling; dense_finish_kernel merges the ranges in range order;
//   dense_probs_kernel    pass 2, per query chunk: the scores again, p = exp(s - m) / l (subtract, exp, divide: the
//                         reference's order) into a [tokens][chunk] buffer whose size is bounded (DR_P_BYTES), and
//                         the usage counters -- every p in 2^40 fixed point, summed over the workgroup's 128 queries
//                         in integers (exact, order-free), one 64-bit atomic per token and workgroup;
//   dense_readout_kernel  the read-out GEMM on the fp32 matrix pipes: the value rows of both segments are the A
//                         operand (channels x tokens), the chunk's p rows the B operand, both staged through LDS.
//                         Every output sums the tokens in the virtual long-then-work order (32-token MFMA chains
//                         added to a running total), so the result does not depend on where the segments split.
// Also here: affinity_dense_kernel, the top-k read for 32 < k <= 64 (one kernel, at the end of the file).
#include <math.h>

#include "affinity_common.h"

#pragma clang fp contract(off)

namespace deva {
namespace {

constexpr int DR_WAVES = 4;
constexpr int DR_QB = DR_WAVES * QT;     // queries per workgroup of the score kernels
constexpr int DR_MAX_SPLITS = 64;        // token ranges of pass 1
constexpr int DR_MAX_OBJ = 8;            // objects per read-out launch
constexpr int64_t DR_P_BYTES = 224ll << 20;  // bound of the p buffer of one query chunk
constexpr int RO_CB = 128;               // read-out: channels per workgroup (32 per wave)
constexpr int RO_QB = 64;                // read-out: queries per workgroup (two MFMA blocks per wave)
constexpr int RO_KT = 32;                // read-out: tokens per LDS stage
constexpr int RO_VS = RO_CB + 32;        // LDS row strides: rows 2k and 2k+1 of an MFMA operand on opposite bank halves
constexpr int RO_PS = RO_QB + 32;

// accumulator row r of a 32x32 MFMA block in lane half `half` <-> row (r & 3) + 8 (r >> 2) + 4 half of the block
__device__ __forceinline__ int acc_row(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }

// scores of the 32 tokens n_base.. against the wave's 32 queries: lane (l31, half) receives v[r] for query l31 and
// token n_base + acc_row(r, half).  msl: this wave's 32-float LDS row.
__device__ __forceinline__ void score_tile(const Bank& b, int n_base, int lane, const float (&bqe)[CK / 2],
                                           const float (&bqk)[CK / 2], float bsq, float* msl, float (&v)[16]) {
  const int l31 = lane & 31, half = lane >> 5;
  const int n_mine = min(n_base + l31, b.n_total - 1);
  float ms;
  const float* krow = bank_row(b, n_mine, &ms);
  // channel 2t + half of this lane's token: the upper half-lanes read one float later (see affinity_topk_kernel)
  const float* shifted = krow + half;
  float a_op[CK / 2];
#pragma unroll
  for (int j = 0; j < CK / 4 - 1; ++j) {
    const f32x4 x = *reinterpret_cast<const f32x4_u*>(shifted + 4 * j);
    a_op[2 * j] = x[0];
    a_op[2 * j + 1] = x[2];
  }
  const f32x4 xl = *reinterpret_cast<const f32x4*>(krow + CK - 4);
  a_op[CK / 2 - 2] = half ? xl[1] : xl[0];
  a_op[CK / 2 - 1] = half ? xl[3] : xl[2];
  if (lane < TOKT) msl[lane] = ms * 0.125f;  // 1/sqrt(CK) folded in (exact)
  DEVA_COMPILER_FENCE();
  f32x16 accA, accB;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    accA[r] = 0.0f;
    accB[r] = 0.0f;
  }
#pragma unroll
  for (int t = 0; t < CK / 2; ++t) {
    const float a = a_op[t];
    accA = __builtin_amdgcn_mfma_f32_32x32x2f32(a * a, bqe[t], accA, 0, 0, 0);
    accB = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bqk[t], accB, 0, 0, 0);
  }
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const float4 m4 = *reinterpret_cast<const float4*>(&msl[8 * g + 4 * half]);
    const float m[4] = {m4.x, m4.y, m4.z, m4.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = 4 * g + i;
      v[r] = (((accB[r] + accB[r]) - accA[r]) - bsq) * m[i];  // == ((-A + 2B) - bsq) * ms / 8, every step rounded
    }
  }
  DEVA_COMPILER_FENCE();  // the next tile rewrites msl
}

struct DrStatsArgs {
  Bank bank;
  const float* qk;
  const float* qe;
  int hw;
  int tiles_per_split;
  float2* part;  // [splits][hw]: (max, sum exp(s - max)) of each token range
};

// pass 1: one wave = 32 queries, one workgroup = 128 queries x one token range
__global__ __launch_bounds__(DR_WAVES * 64) void dense_stats_kernel(const DrStatsArgs p) {
  __shared__ __attribute__((aligned(16))) float s_ms[DR_WAVES][TOKT];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l31 = lane & 31, half = lane >> 5;
  const int q0 = blockIdx.x * DR_QB + wave * QT;
  if (q0 >= p.hw) return;  // (no barriers in this kernel)
  const int q = min(q0 + l31, p.hw - 1);
  float bqe[CK / 2], bqk[CK / 2];
  const float bsq = load_query(p.qk, p.qe, p.hw, q, half, bqe, bqk);
  const int tiles = (int)ceil_div(p.bank.n_total, TOKT);
  const int t0 = blockIdx.y * p.tiles_per_split, t1 = min(tiles, t0 + p.tiles_per_split);
  float m = -INFINITY, l = 0.0f;
  for (int tile = t0; tile < t1; ++tile) {
    const int n_base = tile * TOKT;
    float v[16];
    score_tile(p.bank, n_base, lane, bqe, bqk, bsq, &s_ms[wave][0], v);
    const int rows_left = p.bank.n_total - n_base;
    float mx = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r)
      if (acc_row(r, half) < rows_left) mx = fmaxf(mx, v[r]);
    if (mx > m) {
      if (m != -INFINITY) l = l * expf(m - mx);
      m = mx;
    }
    if (m != -INFINITY) {
#pragma unroll
      for (int r = 0; r < 16; ++r)
        if (acc_row(r, half) < rows_left) l += expf(v[r] - m);
    }
  }
  // the two half-lanes of a query hold different rows: merge them (lower half first)
  const float m_o = __shfl_xor(m, 32), l_o = __shfl_xor(l, 32);
  if (half == 0 && q0 + l31 < p.hw) {
    const float mm = fmaxf(m, m_o);
    float ll = 0.0f;
    if (m != -INFINITY) ll += l * expf(m - mm);
    if (m_o != -INFINITY) ll += l_o * expf(m_o - mm);
    p.part[(int64_t)blockIdx.y * p.hw + q0 + l31] = make_float2(mm, ll);
  }
}

// merge the token ranges of pass 1 in range order -> stats[q] = (max, sum)
__global__ __launch_bounds__(256) void dense_finish_kernel(const float2* __restrict__ part, int splits, int hw,
                                                           float2* __restrict__ stats) {
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= hw) return;
  float m = -INFINITY;
  for (int s = 0; s < splits; ++s) m = fmaxf(m, part[(int64_t)s * hw + q].x);
  float l = 0.0f;
  for (int s = 0; s < splits; ++s) {
    const float2 v = part[(int64_t)s * hw + q];
    if (v.x != -INFINITY) l += v.y * expf(v.x - m);
  }
  stats[q] = make_float2(m, l);
}

struct DrProbsArgs {
  Bank bank;
  const float* qk;
  const float* qe;
  int hw;
  const float2* stats;
  int q0;              // first query of the chunk
  int ld;              // row stride of probs (a multiple of DR_QB)
  int tiles_per_wg;
  float* probs;        // [tiles * TOKT][ld]
  unsigned long long* usage_fix;
};

// pass 2 over one query chunk: workgroup = 128 queries x a range of token tiles
__global__ __launch_bounds__(DR_WAVES * 64) void dense_probs_kernel(const DrProbsArgs p) {
  __shared__ __attribute__((aligned(16))) float s_ms[DR_WAVES][TOKT];
  __shared__ __attribute__((aligned(16))) float s_p[TOKT][DR_QB + 4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l31 = lane & 31, half = lane >> 5;
  const int col0 = blockIdx.x * DR_QB;                 // first column of this workgroup inside the chunk
  const int qg = p.q0 + col0 + wave * QT + l31;        // this lane's query
  const bool q_ok = qg < p.hw;
  const int q = min(qg, p.hw - 1);
  float bqe[CK / 2], bqk[CK / 2];
  const float bsq = load_query(p.qk, p.qe, p.hw, q, half, bqe, bqk);
  const float2 st = p.stats[q];
  const int tiles = (int)ceil_div(p.bank.n_total, TOKT);
  const int t0 = blockIdx.y * p.tiles_per_wg, t1 = min(tiles, t0 + p.tiles_per_wg);
  // second phase of a tile: thread = token row tid / 8 x 16 consecutive columns (tid % 8) * 16
  const int prow = threadIdx.x >> 3, pcol = (threadIdx.x & 7) * 16;
  for (int tile = t0; tile < t1; ++tile) {
    const int n_base = tile * TOKT;
    float v[16];
    score_tile(p.bank, n_base, lane, bqe, bqk, bsq, &s_ms[wave][0], v);
    const int rows_left = p.bank.n_total - n_base;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int j = acc_row(r, half);
      s_p[j][wave * QT + l31] = (q_ok && j < rows_left) ? expf(v[r] - st.x) / st.y : 0.0f;
    }
    __syncthreads();
    const float4* src = reinterpret_cast<const float4*>(&s_p[prow][pcol]);
    float4* dst = reinterpret_cast<float4*>(p.probs + (int64_t)(n_base + prow) * p.ld + col0 + pcol);
    unsigned long long fix = 0ull;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float4 x = src[i];
      dst[i] = x;
      const float e[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (e[u] == e[u]) fix += (unsigned long long)(e[u] * TWO40);
    }
    if (p.usage_fix) {
      fix += __shfl_xor(fix, 1);
      fix += __shfl_xor(fix, 2);
      fix += __shfl_xor(fix, 4);
      if ((threadIdx.x & 7) == 0 && prow < rows_left && fix) atomicAdd(&p.usage_fix[n_base + prow], fix);
    }
    __syncthreads();  // s_p is rewritten by the next tile
  }
}

struct DrReadoutArgs {
  const float* probs;
  int ld;
  int n_pad;             // rows of probs (a multiple of RO_KT)
  int n_long, n_total;
  int cv, hw;
  int q0, qc;            // first query and valid columns of the chunk
  const float* val_long[DR_MAX_OBJ];
  const float* val_work[DR_MAX_OBJ];
  float* out[DR_MAX_OBJ];
};

// out[c][q0 + j] = sum_n V[n][c] * probs[n][j]; workgroup = 128 channels x 64 queries of one object, wave w =
// channels 32w .. 32w + 31 x both 32-query blocks
__global__ __launch_bounds__(256) void dense_readout_kernel(const DrReadoutArgs p) {
  __shared__ __attribute__((aligned(16))) float s_v[2][RO_KT][RO_VS];
  __shared__ __attribute__((aligned(16))) float s_p[2][RO_KT][RO_PS];
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, half = lane >> 5;
  const int obj = blockIdx.z;
  const int c0 = blockIdx.y * RO_CB, j0 = blockIdx.x * RO_QB;
  const float* val_long = p.val_long[obj];
  const float* val_work = p.val_work[obj];

  f32x4 gv[4], gp[2];
  auto load = [&](int k0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {  // value rows: 32 tokens x 128 channels
      const int e = tid + 256 * i;
      const int row = e >> 5, c = c0 + (e & 31) * 4;
      const int n = min(k0 + row, p.n_total - 1);  // padding rows (p = 0) re-read the last token
      const float* src = (n < p.n_long) ? (val_long + (int64_t)n * p.cv) : (val_work + (int64_t)(n - p.n_long) * p.cv);
      gv[i] = (c < p.cv) ? *reinterpret_cast<const f32x4*>(src + c) : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {  // p rows: 32 tokens x 64 queries
      const int e = tid + 256 * i;
      const int row = e >> 4, j = (e & 15) * 4;
      gp[i] = *reinterpret_cast<const f32x4*>(p.probs + (int64_t)(k0 + row) * p.ld + j0 + j);
    }
  };
  auto store = [&](int buf) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int e = tid + 256 * i;
      *reinterpret_cast<f32x4*>(&s_v[buf][e >> 5][(e & 31) * 4]) = gv[i];
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int e = tid + 256 * i;
      *reinterpret_cast<f32x4*>(&s_p[buf][e >> 4][(e & 15) * 4]) = gp[i];
    }
  };

  f32x16 tot0, tot1;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    tot0[r] = 0.0f;
    tot1[r] = 0.0f;
  }
  const int stages = p.n_pad / RO_KT;
  load(0);
  for (int s = 0; s < stages; ++s) {
    const int buf = s & 1;
    store(buf);
    __syncthreads();  // (two buffers: the reads of this one two stages ago finished before the previous barrier)
    if (s + 1 < stages) load((s + 1) * RO_KT);
    f32x16 part0, part1;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      part0[r] = 0.0f;
      part1[r] = 0.0f;
    }
#pragma unroll
    for (int kk = 0; kk < RO_KT / 2; ++kk) {
      const int row = 2 * kk + half;
      const float a = s_v[buf][row][wave * 32 + l31];
      const float b0 = s_p[buf][row][l31], b1 = s_p[buf][row][32 + l31];
      part0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b0, part0, 0, 0, 0);
      part1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b1, part1, 0, 0, 0);
    }
    tot0 += part0;
    tot1 += part1;
  }
  float* out = p.out[obj];
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    const int j = j0 + 32 * b + l31;
    if (j < p.qc) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int c = c0 + wave * 32 + acc_row(r, half);
        if (c < p.cv) out[(int64_t)c * p.hw + p.q0 + j] = b ? tot1[r] : tot0[r];
      }
    }
  }
}

struct DrPlan {
  int tiles, n_pad, hw_pad, splits, tiles_per_split, chunk;
  int64_t off_part, off_stats, off_probs, bytes;
};

DrPlan dense_plan(int n_total, int hw) {
  DrPlan L;
  L.tiles = (int)ceil_div(n_total, TOKT);
  L.n_pad = L.tiles * TOKT;
  L.hw_pad = (int)ceil_div(hw, DR_QB) * DR_QB;
  const int qblocks = (int)ceil_div(hw, DR_QB);
  int s = (int)ceil_div(1024, qblocks);  // ~1 024 workgroups in pass 1
  if (s > DR_MAX_SPLITS) s = DR_MAX_SPLITS;
  if (s > L.tiles) s = L.tiles;
  if (s < 1) s = 1;
  L.tiles_per_split = (int)ceil_div(L.tiles, s);
  L.splits = (int)ceil_div(L.tiles, L.tiles_per_split);
  const int64_t fit = DR_P_BYTES / ((int64_t)L.n_pad * 4) / DR_QB * DR_QB;  // columns of one bounded p chunk
  L.chunk = (int)(fit < L.hw_pad ? fit : L.hw_pad);
  auto align = [](int64_t b) { return (b + 255) / 256 * 256; };
  int64_t o = 0;
  L.off_part = o;
  o += align((int64_t)L.splits * hw * 8);
  L.off_stats = o;
  o += align((int64_t)hw * 8);
  L.off_probs = o;
  o += align((int64_t)L.n_pad * L.chunk * 4);
  L.bytes = o;
  return L;
}

bool aligned16(const void* ptr) { return ((uintptr_t)ptr & 15u) == 0; }

// ------------------------------------------------------------------ dense top-k read (32 < k <= 64)
// The list kernels of affinity.hip size their per-range hand-over for k <= K_MAX = 32.  For the rare larger top_k
// (eval_args.py:40 leaves it free) the read runs on this one kernel: lane = query (64 queries per one-wave workgroup,
// query operands in registers), the bank streams through wave-uniform rows, every score is score_fp32 -- the
// natural-order fp32 FMA chain affinity_pf_rescore_kernel runs (bit-identical scores, hence the same selection as the
// list kernels for any k both can serve) --, and each lane keeps its k best (score, ~token) keys in LDS: unsorted,
// smallest tracked, replaced on insert (~k ln(N/k) inserts per query).  Every query finishes like
// affinity_finalize_kernel (an inline copy of the shared tail of affinity_common.h).  VALU-bound: 192 instructions per (token, query); ~4 ms at
// N = 10 000 x 8 160 queries -- a correct path, not a fast one.
constexpr int DK_MAX = 64;

struct DenseArgs {
  Bank bank;
  const float* qk;
  const float* qe;
  int hw, k;
  int32_t* idx;
  float* weight;
  unsigned long long* usage_fix;
};

__global__ __launch_bounds__(64) void affinity_dense_kernel(const DenseArgs p) {
  __shared__ uint64_t s_list[DK_MAX][64];  // [entry][query lane]
  __shared__ uint64_t s_sort[64];
  const int lane = threadIdx.x;
  const int q0 = blockIdx.x * 64;
  const int qq = min(q0 + lane, p.hw - 1);
  const int k = p.k, n = p.bank.n_total;
  float qe[CK], qp[CK];
  float bs[4] = {0.0f, 0.0f, 0.0f, 0.0f};  // bsq in ATen's summation order (see load_query)
#pragma unroll
  for (int c = 0; c < CK; ++c) {
    const float ev = p.qe[(int64_t)c * p.hw + qq], kv = p.qk[(int64_t)c * p.hw + qq];
    qe[c] = ev;
    qp[c] = kv * ev;
    bs[c >> 4] += ev * (kv * kv);
  }
  const float bsq = ((bs[0] + bs[1]) + bs[2]) + bs[3];

  uint64_t kmin = ~0ull;
  int pmin = 0;
  for (int t = 0; t < n; ++t) {  // t is wave-uniform: the row and its shrinkage are scalar loads
    float ms;
    const float* row = bank_row(p.bank, t, &ms);
    // mirrors score_fp32 (affinity_common.h), inline: through the helper this VALU-bound loop measured 0.8 % slower
    float accA = 0.0f, accB = 0.0f;
#pragma unroll
    for (int c = 0; c < CK; ++c) {
      const float a = row[c];
      accA = __builtin_fmaf(a * a, qe[c], accA);
      accB = __builtin_fmaf(a, qp[c], accB);
    }
    const float v = (((accB + accB) - accA) - bsq) * (ms * 0.125f);
    const uint64_t key = ((uint64_t)orderable(v) << 32) | (uint64_t)(~(uint32_t)t);
    if (t < k) {  // (uniform) the first k tokens fill the list
      s_list[t][lane] = key;
      if (key < kmin) {
        kmin = key;
        pmin = t;
      }
    } else if (key > kmin) {
      s_list[pmin][lane] = key;
      kmin = ~0ull;
      for (int e = 0; e < k; ++e) {
        const uint64_t o = s_list[e][lane];
        if (o < kmin) {
          kmin = o;
          pmin = e;
        }
      }
    }
  }
  __syncthreads();

  // ---- per query of the tile: mirrors rank_sort_k + softmax_usage_tail (affinity_common.h), inline: through the helpers
  // this kernel measured 0.3 % slower, outside the parent's spread (profiles/HISTORY.md)
  const bool live = lane < k;
  for (int j = 0; j < 64 && q0 + j < p.hw; ++j) {
    const int q = q0 + j;
    const uint64_t cand = live ? s_list[live ? lane : 0][j] : 0ull;
    int rank = 0;
    for (int r = 0; r < k; ++r) {
      const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)cand, r);
      const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(cand >> 32), r);
      rank += ((((uint64_t)hi << 32) | lo) > cand) ? 1 : 0;
    }
    __syncthreads();  // (one wave: orders the LDS traffic of consecutive queries)
    if (live) s_sort[rank] = cand;
    __syncthreads();
    const uint64_t mine = live ? s_sort[lane] : 0ull;  // lane r holds the r-th best
    const float score = from_orderable((uint32_t)(mine >> 32));
    const uint32_t token = ~(uint32_t)mine;
    const float ex = live ? expf(score) : 0.0f;
    float sum = 0.0f;
    for (int r = 0; r < k; ++r)  // sequential, like torch.sum over the sorted top-k
      sum += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ex), r));
    const float w = ex / sum;
    if (live) {
      p.idx[(int64_t)q * k + lane] = (int32_t)token;
      p.weight[(int64_t)q * k + lane] = w;
      if (p.usage_fix && w == w) atomicAdd(&p.usage_fix[token], (unsigned long long)(w * TWO40));
    }
  }
}

}  // namespace
}  // namespace deva

using namespace deva;

extern "C" int64_t deva_dense_read_scratch(int n_total, int hw) {
  if (n_total <= 0 || hw <= 0) return 256;
  return dense_plan(n_total, hw).bytes;
}

extern "C" int deva_dense_read(const float* key_long, const float* shr_long, int n_long, const float* key_work,
                               const float* shr_work, int n_work, const float* qk, const float* qe, int hw, int n_obj,
                               const float* const* val_long, const float* const* val_work, int cv, float* const* out,
                               uint64_t* usage_fix, void* scratch, int64_t scratch_bytes, float* probs, void* stream) {
  // every check before the first launch
  DEVA_REQUIRE(qk && qe && hw > 0, "deva_dense_read: bad query args");
  DEVA_REQUIRE(n_long >= 0 && n_work >= 0, "deva_dense_read: negative bank size");
  DEVA_REQUIRE(n_long == 0 || (key_long && shr_long), "deva_dense_read: null long-term segment");
  DEVA_REQUIRE(n_work == 0 || (key_work && shr_work), "deva_dense_read: null working segment");
  DEVA_REQUIRE(aligned16(key_long) && aligned16(key_work), "deva_dense_read: key arenas must be 16-B aligned");
  const int64_t n_total = (int64_t)n_long + n_work;
  DEVA_REQUIRE(n_total >= 1, "deva_dense_read: empty bank");
  DEVA_REQUIRE(n_total < (1ll << 31) - 64, "deva_dense_read: bank too large");
  DEVA_REQUIRE(n_obj >= 0, "deva_dense_read: negative object count");
  if (n_obj > 0) {
    DEVA_REQUIRE(val_work && out && (n_long == 0 || val_long), "deva_dense_read: null value / output arrays");
    DEVA_REQUIRE(cv > 0 && cv % 4 == 0, "deva_dense_read: cv=%d must be a positive multiple of 4", cv);
    for (int o = 0; o < n_obj; ++o) {
      DEVA_REQUIRE(out[o], "deva_dense_read: null output of object %d", o);
      DEVA_REQUIRE(n_work == 0 || (val_work[o] && aligned16(val_work[o])),
                   "deva_dense_read: working values of object %d null or not 16-B aligned", o);
      DEVA_REQUIRE(n_long == 0 || (val_long[o] && aligned16(val_long[o])),
                   "deva_dense_read: long-term values of object %d null or not 16-B aligned", o);
    }
  }
  const DrPlan L = dense_plan((int)n_total, hw);
  DEVA_REQUIRE(L.chunk >= DR_QB, "deva_dense_read: bank of %lld tokens too large for the bounded p buffer (max %lld)",
               (long long)n_total, (long long)(DR_P_BYTES / (DR_QB * 4)));
  DEVA_REQUIRE(scratch && aligned16(scratch) && scratch_bytes >= L.bytes,
               "deva_dense_read: scratch of %lld bytes < %lld (deva_dense_read_scratch) or misaligned",
               (long long)scratch_bytes, (long long)L.bytes);
  DEVA_REQUIRE(aligned16(probs), "deva_dense_read: probs must be 16-B aligned");
  hipStream_t st = (hipStream_t)stream;
  uint8_t* base = reinterpret_cast<uint8_t*>(scratch);
  const Bank b = make_bank(key_long, shr_long, n_long, key_work, shr_work, n_total);
  float2* part = reinterpret_cast<float2*>(base + L.off_part);
  float2* stats = reinterpret_cast<float2*>(base + L.off_stats);

  DrStatsArgs sa;
  sa.bank = b;
  sa.qk = qk;
  sa.qe = qe;
  sa.hw = hw;
  sa.tiles_per_split = L.tiles_per_split;
  sa.part = part;
  hipLaunchKernelGGL(dense_stats_kernel, dim3((unsigned)ceil_div(hw, DR_QB), (unsigned)L.splits), dim3(DR_WAVES * 64), 0, st,
                     sa);
  hipLaunchKernelGGL(dense_finish_kernel, dim3((unsigned)ceil_div(hw, 256)), dim3(256), 0, st, part, L.splits, hw, stats);
  if (check_launch("deva_dense_read (pass 1)")) return 1;

  // probs != NULL (test hook): the whole [n_pad][hw_pad] matrix goes there as one chunk
  const int chunk = probs ? L.hw_pad : L.chunk;
  float* pbuf = probs ? probs : reinterpret_cast<float*>(base + L.off_probs);
  for (int q0 = 0; q0 < hw; q0 += chunk) {
    const int qc = min(chunk, hw - q0);
    const int xb = (int)ceil_div(qc, DR_QB);
    DrProbsArgs pa;
    pa.bank = b;
    pa.qk = qk;
    pa.qe = qe;
    pa.hw = hw;
    pa.stats = stats;
    pa.q0 = q0;
    pa.ld = chunk;
    pa.tiles_per_wg = (int)ceil_div((int64_t)L.tiles * xb, 2048);  // ~2 048 workgroups
    if (pa.tiles_per_wg < 1) pa.tiles_per_wg = 1;
    pa.probs = pbuf;
    pa.usage_fix = (unsigned long long*)usage_fix;
    hipLaunchKernelGGL(dense_probs_kernel, dim3((unsigned)xb, (unsigned)ceil_div(L.tiles, pa.tiles_per_wg)),
                       dim3(DR_WAVES * 64), 0, st, pa);
    if (check_launch("deva_dense_read (pass 2)")) return 1;
    for (int o0 = 0; o0 < n_obj; o0 += DR_MAX_OBJ) {
      const int no = min(DR_MAX_OBJ, n_obj - o0);
      DrReadoutArgs ra;
      ra.probs = pbuf;
      ra.ld = chunk;
      ra.n_pad = L.n_pad;
      ra.n_long = n_long;
      ra.n_total = (int)n_total;
      ra.cv = cv;
      ra.hw = hw;
      ra.q0 = q0;
      ra.qc = qc;
      for (int i = 0; i < DR_MAX_OBJ; ++i) {
        const int o = o0 + (i < no ? i : 0);
        const float* vw = (n_work > 0) ? val_work[o] : nullptr;
        const float* vl = (n_long > 0) ? val_long[o] : nullptr;
        ra.val_long[i] = vl ? vl : vw;
        ra.val_work[i] = vw ? vw : vl;
        ra.out[i] = out[o];
      }
      hipLaunchKernelGGL(dense_readout_kernel, dim3((unsigned)ceil_div(qc, RO_QB), (unsigned)ceil_div(cv, RO_CB), (unsigned)no),
                         dim3(256), 0, st, ra);
      if (check_launch("deva_dense_read (read-out)")) return 1;
    }
  }
  return 0;
}

extern "C" int deva_affinity_dense(const float* key_long, const float* shr_long, int n_long, const float* key_work,
                                   const float* shr_work, int n_work, const float* qk, const float* qe, int hw, int k,
                                   int32_t* idx, float* weight, uint64_t* usage_fix, void* stream) {
  DEVA_REQUIRE(qk && qe && idx && weight && hw > 0, "deva_affinity_dense: bad args");
  DEVA_REQUIRE(n_long >= 0 && n_work >= 0, "deva_affinity_dense: negative bank size");
  DEVA_REQUIRE(n_long == 0 || (key_long && shr_long), "deva_affinity_dense: null long-term segment");
  DEVA_REQUIRE(n_work == 0 || (key_work && shr_work), "deva_affinity_dense: null working segment");
  DEVA_REQUIRE(k >= 1 && k <= DK_MAX, "deva_affinity_dense: k=%d unsupported (1..%d)", k, DK_MAX);
  const int64_t n_total = (int64_t)n_long + n_work;
  DEVA_REQUIRE(n_total >= k, "deva_affinity_dense: selected index k out of range (bank has %lld tokens, k=%d)",
               (long long)n_total, k);
  DEVA_REQUIRE(n_total < (1ll << 31) - 64, "deva_affinity_dense: bank too large");
  DenseArgs a;
  a.bank = make_bank(key_long, shr_long, n_long, key_work, shr_work, n_total);
  a.qk = qk;
  a.qe = qe;
  a.hw = hw;
  a.k = k;
  a.idx = idx;
  a.weight = weight;
  a.usage_fix = (unsigned long long*)usage_fix;
  hipLaunchKernelGGL(affinity_dense_kernel, dim3((unsigned)ceil_div(hw, 64)), dim3(64), 0, (hipStream_t)stream, a);
  return check_launch("deva_affinity_dense");
}
