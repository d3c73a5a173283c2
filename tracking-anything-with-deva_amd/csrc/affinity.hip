// Memory read of DEVA on gfx950: anisotropic-L2 similarity -> exact top-k -> softmax (-> usage),
// fused so that the N x HW similarity matrix is never written (the reference materialises it
// ~12 times per frame, memory_utils.py:29-74).  This file: the fp32 candidate-list kernels, the merge / select
// kernel that finishes a read, the usage update and the sparse read-out.  The fp16 pre-filter in front of them is
// affinity_prefilter.hip, the reads beyond k = 32 are dense_read.hip; affinity_common.h holds what they share.
//
// Similarity (memory_utils.py:29-43), per memory token n and query q:
//     A = sum_c mk[n][c]^2 * qe[c][q]          B = sum_c mk[n][c] * (qk[c][q]*qe[c][q])
//     sim = ((-A + 2B) - bsq[q]) * ms[n] / sqrt(64)
// A and B run on the fp32 matrix cores (v_mfma_f32_32x32x2_f32, exact fp32 FMA chains) with the
// channels in natural order, each in its own accumulator and combined in the reference's order, so
// the scores agree with an fp32 FMA GEMM to the last bits -- top-k is discontinuous, a 1e-5
// relative error flips memory tokens in and out of the softmax support.
//
// Work decomposition: one wave owns 32 queries (the MFMA N dimension) and streams a range of
// memory tokens in tiles of 32 (the MFMA M dimension); the query operand lives in registers for
// the whole kernel, the key rows are read straight from the token-major bank and prefetched one
// tile ahead (a 32x64 fp32 tile per 4096 matrix-pipe cycles -- operand traffic is irrelevant here,
// the kernel is bound by the fp32 MFMA rate).  Per query there is a candidate list in LDS
// (LCAP slots of 6 bytes) with a running lower bound of the k-th best: scores >= the bound
// are appended (~k*(1+ln(n/k)) appends per query over n tokens); a list that could
// overflow is pruned to the entries >= the k-th largest of its 64 per-lane maxima (at least k entries
// are >= that value, so the final result stays exact).  That k-th largest is found by rank counting
// over the 64 lane values through a 256-B LDS row (128 independent compare / add pairs) instead of a
// ballot bisection, whose ~10-30 dependent VALU->SALU->branch round trips cost ~3 700 cycles per list
// and, at three prune rounds of 32 lists per range, a third of the kernel at the N = 10 000 shape
// (round-1 profile); the exact bisection on unique (score, token) keys remains as the fallback for
// banks full of identical scores.  grid.y splits the bank into token ranges so small frames still
// fill the chip; every range hands over its (pruned, <= CAP entries) lists with their lengths and a
// second kernel (one wave per query) selects the exact top-k over all ranges, applies exp/normalise
// and accumulates the usage counters.
//
// What the round-2 measurements say about this part (profiles/r02b_affinity_shapes.txt, tools/probe):
// fp32 MFMAs and VALU work do not overlap -- kernel time ~ MFMA cycles + VALU issue cycles + exposed
// waits at any occupancy -- and the exposed waits are the prunes' LDS round trips (per-wave lists) or
// the skew collected by workgroup barriers (shared lists).  Hence the two kernels (shapes 2 / 4 / 8 of
// deva_affinity_force_shape in the header; the automatic choice is by bank size):
//   affinity_topk_wg_kernel   short banks (<= 20 000 - 30 000 tokens): the waves of a workgroup share 32
//                             queries' lists (LDS-atomic appends, one threshold per query, two barriers per
//                             tile) -- fewest appends and prunes.  Four waves, 352 slots, two workgroups per
//                             CU on large frames; eight waves, 704 slots, one workgroup per CU on small
//                             frames (half the token ranges, so half the lists to merge afterwards);
//   affinity_topk_kernel      longer banks: four waves x four query groups, 100-slot per-wave lists, two
//                             workgroups per CU, no barriers.
// Both prefetch the key rows after the last MFMA of a tile and read them in place, and keep their registers
// reserved until the MFMAs read them (DEVA_KEEP_ROWS: otherwise the scoring phase waits for the loads it is
// supposed to cover); rows are filed only when some lane passes, accumulators stay in VGPRs
// (-amdgpu-mfma-vgpr-form, see the Makefile), operand rows are loaded with a per-half-lane offset instead
// of being selected, appends store raw fp32 bits (ordered only when a list is pruned / handed over), and
// the scrambled tile order is advanced incrementally (a 64-bit modulo per tile was ~300 scalar
// instructions on the critical path).  Tried in round 2 and dropped as bit-identical but slower
// (profiles/r02e_affinity_shapes.txt): one workgroup per CU with wider lists, key tiles shared through LDS, prefetch
// before the MFMAs, issue priorities, and an eight-wave ping-pong of matrix and scoring phases.
#include <math.h>

#include <type_traits>

#include "affinity_common.h"

#pragma clang fp contract(off)

namespace deva {
namespace {

// in-kernel candidate lists: LCAP slots of 6 bytes (order-preserving score bits + 16-bit token offset
// inside the range); row stride LCAP + 1 (odd: spreads the LDS banks).
constexpr int LCAP_DUAL = 100;    // two workgroups per CU (2 x 76 KiB)
constexpr int MAX_SPLITS = 32;    // one 64-bit key per lane and range in the merge kernel
constexpr int WAVES = 4;

// The prefetched key rows sit in registers for a whole tile while their loads are in flight.  Only two of
// the four floats of a 16-B piece are MFMA operands, and the register allocator would hand the other two to
// unrelated values of the scoring phase -- writing such a register has to wait (s_waitcnt vmcnt) for the load
// that targets it, which exposes the memory latency the prefetch is there to hide.  Naming every piece as an
// asm input right before its first use keeps all four registers reserved until then (no instruction emitted).
// For the same reason nothing is computed from the prefetched shrinkage until it is stored to LDS.
#define DEVA_KEEP_ROWS(rows)                                     \
  _Pragma("unroll") for (int j_ = 0; j_ < CK / 4; ++j_) {        \
    asm volatile("" ::"v"(rows[j_]));                            \
  }

// Lower bound of the k-th largest of the 64 lane values `m` (order-preserving score bits, 0 = empty
// lane; needs >= k non-empty lanes) by rank counting: the low 6 bits are replaced by the lane number so
// that the values are unique, the 64 values go through a 256-B LDS scratch row, every lane reads them
// back as 16 broadcast 16-B reads and counts the values above its own (128 independent compare / add
// pairs -- no readlane hazards and no dependent VALU -> SALU -> branch chain as in a bisection), and the
// lane of rank k-1 publishes its value with the low bits cleared: at least k lanes have m >= the result.
__device__ __forceinline__ uint32_t kth_lane_value(uint32_t m, int k, int lane, uint32_t* scratch) {
  const uint32_t u = (m & ~63u) | (uint32_t)lane;
  scratch[lane] = u;
  DEVA_COMPILER_FENCE();
  int rank = 0;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const uint4 o = *reinterpret_cast<const uint4*>(scratch + 4 * j);
    rank += (o.x > u) ? 1 : 0;
    rank += (o.y > u) ? 1 : 0;
    rank += (o.z > u) ? 1 : 0;
    rank += (o.w > u) ? 1 : 0;
  }
  DEVA_COMPILER_FENCE();
  const unsigned long long b = __builtin_amdgcn_ballot_w64(rank == k - 1);  // exactly one lane: the values are unique
  return (uint32_t)__builtin_amdgcn_readlane((int)u, __ffsll(b) - 1) & ~63u;
}

// Prune one candidate list (wave-cooperative, 64 <= c <= 64*E entries).  Threshold = (a lower bound of)
// the k-th largest of the 64 per-lane maxima: at least k entries of the list are >= it, so nothing below
// it can belong to the top-k -- the result stays exact.  At most E*k entries survive (k lanes hold a
// maximum >= the threshold, each with <= E entries), typically k .. 1.5k.  Returns the threshold (score
// bits); *kept = number of survivors (compacted to the front, unsorted).
template <int E>
__device__ __forceinline__ uint32_t prune_list(uint32_t* sc, uint16_t* tk, uint32_t c, int k, int lane, int* kept,
                                               uint32_t* scratch) {
  uint32_t raw[E], e[E], t[E];  // the lists hold raw fp32 bits (cheap appends); ordered here
  uint32_t m = 0u;
#pragma unroll
  for (int i = 0; i < E; ++i) {
    const uint32_t j = (uint32_t)lane + 64u * i;
    raw[i] = (j < c) ? sc[j] : 0u;
    e[i] = (j < c) ? orderable(__uint_as_float(raw[i])) : 0u;
    t[i] = (j < c) ? (uint32_t)tk[j] : 0u;
    m = e[i] > m ? e[i] : m;
  }
  const uint32_t thr = kth_lane_value(m, k, lane, scratch);
  const uint32_t thr1 = thr ? thr : 1u;  // empty slots (0) never pass: one compare per entry
  DEVA_COMPILER_FENCE();
  int base = 0;
#pragma unroll
  for (int i = 0; i < E; ++i) {
    const bool keep = e[i] >= thr1;
    const unsigned long long b = __builtin_amdgcn_ballot_w64(keep);
    if (keep) {
      const int w = base + prefix_below(b);
      sc[w] = raw[i];
      tk[w] = (uint16_t)t[i];
    }
    base += __popcll(b);
  }
  DEVA_COMPILER_FENCE();
  *kept = base;
  return thr;
}

// Exact variant (slow path): threshold = the exact k-th largest of the 64 per-lane maxima of the UNIQUE
// 64-bit keys (score bits, token), by ballot bisection.  Exactly k lanes hold a maximum >= it, so at
// most E*k entries survive whatever the scores are -- including banks full of identical keys, where the
// rank-counting prune (which compares 26 score bits) cannot separate anything.
template <int E>
__device__ __forceinline__ uint32_t prune_list_exact(uint32_t* sc, uint16_t* tk, uint32_t c, int k, int lane,
                                                     int* kept) {
  uint64_t e[E];
  uint64_t m[1] = {0ull};
#pragma unroll
  for (int i = 0; i < E; ++i) {
    const uint32_t j = (uint32_t)lane + 64u * i;
    e[i] = (j < c) ? (((uint64_t)orderable(__uint_as_float(sc[j])) << 32) | (uint64_t)(0xffffu - tk[j])) : 0ull;
    m[0] = e[i] > m[0] ? e[i] : m[0];
  }
  const uint64_t thr = kth_largest<1>(m, 1, k);
  DEVA_COMPILER_FENCE();
  int base = 0;
#pragma unroll
  for (int i = 0; i < E; ++i) {
    const bool keep = e[i] >= thr && e[i] != 0ull;
    const unsigned long long b = __builtin_amdgcn_ballot_w64(keep);
    if (keep) {
      const int w = base + prefix_below(b);
      sc[w] = __float_as_uint(from_orderable((uint32_t)(e[i] >> 32)));
      tk[w] = (uint16_t)(0xffffu - (uint32_t)(e[i] & 0xffffu));
    }
    base += __popcll(b);
  }
  DEVA_COMPILER_FENCE();
  *kept = base;
  return (uint32_t)(thr >> 32);
}

struct AffArgs {
  const float* key_long;
  const float* shr_long;
  int n_long;
  const float* key_work;
  const float* shr_work;
  int n_total;
  const float* qk;
  const float* qe;
  int hw;
  int k;
  int splits;
  int total_tiles;
  uint64_t* part;     // [splits][hw][CAP] candidate keys
  uint32_t* part_cnt;  // [splits][hw] live entries of each list
  int ablate;          // timing probes, builds with -DDEVA_AFFINITY_PROBES only (0 otherwise): 1 = file nothing,
                       // 2 = no key loads in the loop, 4 = no scoring, 8 = no MFMAs; results are meaningless when non-zero
  uint64_t* probe;     // probe builds: cycle stamps of the first workgroups' phases (tools/probe/affinity_phases.py)
  const uint32_t* guard;  // != NULL: run only if *guard != 0 (the fp32 path as the fall-back of the fp16 pre-filter)
};

#ifdef DEVA_AFFINITY_PROBES
#define DEVA_ABLATE(bit) ((p.ablate & (bit)) != 0)
#else
#define DEVA_ABLATE(bit) false  // the probe paths are compiled out of the product build
#endif

#ifdef DEVA_AFFINITY_PROBES
#define DEVA_STAMP(slot)                                                                    \
  do {                                                                                      \
    if (pb && it < 64 && lane == 0) pb[it * 8 + (slot)] = __builtin_readcyclecounter();     \
  } while (0)
#else
#define DEVA_STAMP(slot) \
  do {                   \
  } while (0)
#endif

// LCAP: list slots per query; MINB: workgroups per CU the register / LDS budget is sized for.
template <int LCAP, int MINB>
__global__ __launch_bounds__(WAVES * 64, MINB) void affinity_topk_kernel(const AffArgs p) {
  if (p.guard && *p.guard == 0u) return;  // uniform over the grid
  constexpr int LSTRIDE = LCAP + 1;
  constexpr int E = (LCAP + 63) / 64;  // list entries per lane in a prune
  static_assert(LCAP - TOKT >= 64, "a list is pruned only when every lane holds an entry");
  static_assert(LCAP < 65536 && CAP == 64, "hand-over: one key per lane");
  static_assert(E * K_MAX <= LCAP - TOKT, "one exact prune (<= E*k survivors) must get below the in-loop limit");
  static_assert(2 * K_MAX <= CAP, "an exact prune of a two-entries-per-lane list must fit the hand-over");
  __shared__ uint32_t s_sc[WAVES][QT][LSTRIDE];  // candidate scores (fp32 bits)
  __shared__ uint16_t s_tk[WAVES][QT][LSTRIDE];  // candidate tokens (offset inside this range)
  __shared__ __attribute__((aligned(16))) float s_ms[WAVES][TOKT];  // shrinkage / 8 of the current tile
  __shared__ __attribute__((aligned(16))) uint32_t s_rank[WAVES][64];  // scratch row of the prune

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int l31 = lane & 31;
  const int half = lane >> 5;
  const int q0 = (blockIdx.x * WAVES + wave) * QT;
  const bool active = q0 < p.hw;
  if (!active) return;  // a wave without queries (ragged last query block); no barriers in this kernel
  const int split = blockIdx.y;

  // NB plain (non-volatile) LDS accesses: hipcc puts `s_waitcnt vmcnt(0)` next to every volatile
  // access, which would drain the key-row prefetch at each list operation.  Program order on may-alias
  // LDS locations plus the in-order LDS pipeline give the cross-lane visibility needed inside a wave;
  // DEVA_COMPILER_FENCE() marks the hand-over points.
  uint32_t* csc = &s_sc[wave][0][0];
  uint16_t* ctk = &s_tk[wave][0][0];
  float* msl = &s_ms[wave][0];
  uint32_t* srow = csc + l31 * LSTRIDE;
  uint16_t* trow = ctk + l31 * LSTRIDE;

  // ---- query operand (registers, whole kernel): mirrors load_query (affinity_common.h), inline for the register
  // allocation
  const int q = min(q0 + l31, p.hw - 1);
  float bqe[CK / 2], bqk[CK / 2];
  float bs[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int t = 0; t < CK / 2; ++t) {
    const float e0 = p.qe[(int64_t)(2 * t) * p.hw + q], e1 = p.qe[(int64_t)(2 * t + 1) * p.hw + q];
    const float k0 = p.qk[(int64_t)(2 * t) * p.hw + q], k1 = p.qk[(int64_t)(2 * t + 1) * p.hw + q];
    bs[t >> 3] += e0 * (k0 * k0);
    bs[t >> 3] += e1 * (k1 * k1);
    bqe[t] = half ? e1 : e0;
    bqk[t] = half ? (k1 * e1) : (k0 * e0);
  }
  const float bsq = ((bs[0] + bs[1]) + bs[2]) + bs[3];
  const f32x2 bsq2 = {bsq, bsq};

  // Token ranges are tile-cyclic (range s owns tiles s, s+S, s+2S, ...) and every range visits its
  // tiles in a multiplicatively scrambled order.  The filter only works while the threshold is
  // representative of what is still to come: a video memory is ordered in time and space, scores
  // drift upwards towards the best-matching frame / region, and a front-to-back scan of a contiguous
  // range then appends nearly every token it meets (measured: 3x slower than on shuffled keys).
  const int n_my = (p.total_tiles - split + p.splits - 1) / p.splits;  // tiles of this range
  int stride = 61;  // a prime that does not divide n_my: c -> (c * stride) % n_my is a permutation
  if (n_my % 61 == 0) stride = (n_my % 59 == 0) ? 53 : 59;
  // the cyclic index of visit i is (i * stride) % n_my, advanced by one conditional subtraction per tile
  const int step = (n_my > 0) ? stride % n_my : 0;
  auto advance = [&](int c) {
    c += step;
    return c >= n_my ? c - n_my : c;
  };
  // candidate tokens are stored as 16 bits: (cyclic tile index << 5) | row

  // ---- per-query state in registers (the same value in both half-lanes of a query): list length and
  // the running lower bound of the k-th best score
  uint32_t cnt = 0;
  float tau = DEVA_ABLATE(1) ? INFINITY : -INFINITY;

  // Key rows are software-prefetched one tile ahead: lane (l31, half) reads the 256-B row of token
  // n_base + l31 while the matrix pipe works on the previous tile.  Lanes of the upper half start one
  // float later, so that x / z of every 16-B piece are exactly the channels 2t+half the lane feeds to
  // the MFMAs -- no per-element select (VALU work does not overlap the wave's own MFMAs, every
  // instruction saved here is time saved; tools/probe/README.md).  The last piece is read aligned
  // (a shifted read would touch the next row) and selected.
  f32x4 xbuf[CK / 4];
  float ms_buf;
  auto prefetch = [&](int cyc) {
    const int tile = split + p.splits * cyc;
    const int n_mine = min(tile * TOKT + l31, p.n_total - 1);
    const float* krow = (n_mine < p.n_long) ? (p.key_long + (int64_t)n_mine * CK)
                                            : (p.key_work + (int64_t)(n_mine - p.n_long) * CK);
    // 1/sqrt(CK) folded into the shrinkage: (x * ms) * 0.125 == x * (ms * 0.125) exactly
    ms_buf = ((n_mine < p.n_long) ? p.shr_long[n_mine] : p.shr_work[n_mine - p.n_long]);  // scaled when stored: see DEVA_KEEP_ROWS
    const float* shifted = krow + half;
#pragma unroll
    for (int j = 0; j < CK / 4 - 1; ++j) xbuf[j] = *reinterpret_cast<const f32x4_u*>(shifted + 4 * j);
    xbuf[CK / 4 - 1] = *reinterpret_cast<const f32x4*>(krow + CK - 4);
  };
  int cyc = 0;  // cyclic tile index of the current visit
  if (n_my > 0) prefetch(cyc);

  // fast = rank-counting prune first; the exact prune runs if that left the list above the limit (or
  // alone if !fast).  One exact prune leaves <= E*k <= limit entries in the tile loop.
  auto prune_over = [&](uint32_t limit, bool fast) {
    uint64_t need = __builtin_amdgcn_ballot_w64(cnt > limit) & 0xffffffffull;
    while (need) {
      const int qq = __ffsll((unsigned long long)need) - 1;
      need &= need - 1;
      const uint32_t c = (uint32_t)__builtin_amdgcn_readlane((int)cnt, qq);
      int kept = (int)c;
      uint32_t thr = 0u;
      if (fast) thr = prune_list<E>(csc + qq * LSTRIDE, ctk + qq * LSTRIDE, c, p.k, lane, &kept, &s_rank[wave][0]);
      if ((uint32_t)kept > limit) {
        const uint32_t thr2 =
            prune_list_exact<E>(csc + qq * LSTRIDE, ctk + qq * LSTRIDE, (uint32_t)kept, p.k, lane, &kept);
        thr = thr2 > thr ? thr2 : thr;
      }
      if (l31 == qq) {
        cnt = (uint32_t)kept;
        tau = from_orderable(thr);
      }
    }
  };

  for (int it = 0; it < n_my; ++it) {
    const int tile = split + p.splits * cyc;
    const int n_base = tile * TOKT;
    const uint32_t tok0 = (uint32_t)(cyc * TOKT + 4 * half);

    // ---- prune lists that could overflow during this tile (at most 32 appends per query per tile)
    prune_over((uint32_t)(LCAP - TOKT), true);

    // ---- this tile's operand: channel 2t + half of this lane's token.  The MFMAs read the prefetched rows in
    // place (a_op only names their registers) and the next tile's loads start after the last MFMA.
    float a_op[CK / 2];
    DEVA_KEEP_ROWS(xbuf);
#pragma unroll
    for (int j = 0; j < CK / 4 - 1; ++j) {
      a_op[2 * j] = xbuf[j][0];
      a_op[2 * j + 1] = xbuf[j][2];
    }
    a_op[CK / 2 - 2] = half ? xbuf[CK / 4 - 1][1] : xbuf[CK / 4 - 1][0];
    a_op[CK / 2 - 1] = half ? xbuf[CK / 4 - 1][3] : xbuf[CK / 4 - 1][2];
    if (lane < TOKT) msl[lane] = ms_buf * 0.125f;  // 1/sqrt(CK) folded in (exact)
    DEVA_COMPILER_FENCE();

    f32x16 accA, accB;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      accA[r] = 0.0f;
      accB[r] = 0.0f;
    }
    if (!DEVA_ABLATE(8)) {
#pragma unroll
      for (int t = 0; t < CK / 2; ++t) {
        const float a = a_op[t];
        accA = __builtin_amdgcn_mfma_f32_32x32x2f32(a * a, bqe[t], accA, 0, 0, 0);
        accB = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bqk[t], accB, 0, 0, 0);
      }
    } else {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        accA[r] = a_op[r];
        accB[r] = a_op[r + 16];
      }
    }
    DEVA_COMPILER_FENCE();
    if (it + 1 < n_my) cyc = advance(cyc);
    if (!DEVA_ABLATE(2)) prefetch(cyc);

    // ---- scores of this lane: query l31, tokens n_base + (r&3) + 8*(r>>2) + 4*half, two accumulator
    // rows per packed-fp32 instruction.  A row is filed only if some lane of the wave passes its
    // threshold (about every other row once the thresholds have settled); the position in the list the
    // two half-lanes of a query share comes from the ballot.
    float4 ms4[4];  // scaled shrinkage in accumulator-row order: rows 4g..4g+3 <-> tokens 8g+4*half..+3
#pragma unroll
    for (int g = 0; g < 4; ++g) ms4[g] = *reinterpret_cast<const float4*>(&msl[8 * g + 4 * half]);
    const int rows_left = p.n_total - n_base;  // >= TOKT except in the last tile of the bank
    auto file_rows = [&](auto full) {
      constexpr bool full_tile = decltype(full)::value;
#pragma unroll
      for (int r2 = 0; r2 < 8; ++r2) {
        const f32x2 a2 = {accA[2 * r2], accA[2 * r2 + 1]};
        const f32x2 b2 = {accB[2 * r2], accB[2 * r2 + 1]};
        const float4 m4 = ms4[r2 >> 1];
        const f32x2 m2 = (r2 & 1) ? f32x2{m4.z, m4.w} : f32x2{m4.x, m4.y};
        f32x2 v2 = ((b2 + b2) - a2) - bsq2;  // == (-A + 2B) - bsq, every step correctly rounded
        v2 = v2 * m2;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int r = 2 * r2 + h;
          const int j0 = (r & 3) + 8 * (r >> 2);  // + 4 * half
          const float v = v2[h];
          bool ok = v >= tau;
          if (!full_tile) ok = ok && (j0 + 4 * half < rows_left);
          const unsigned long long b = __builtin_amdgcn_ballot_w64(ok);
          if (b) {
            // the two half-lanes of query l31 are lanes l31 and 32 + l31: one 32-bit bit-field extract each
            const uint32_t ok_lo = ((uint32_t)b >> l31) & 1u, ok_hi = ((uint32_t)(b >> 32) >> l31) & 1u;
            if (ok) {
              const uint32_t pos = cnt + (half ? ok_lo : 0u);
              srow[pos] = __float_as_uint(v);  // raw bits: ordered when a list is pruned / handed over
              trow[pos] = (uint16_t)(tok0 + j0);
            }
            cnt += ok_lo + ok_hi;
          }
        }
      }
    };
    if (DEVA_ABLATE(4)) {  // keep the accumulators alive without scoring them
      if (accA[0] + accB[15] == 12345.678f) cnt += 1;
    } else if (rows_left >= TOKT) {
      file_rows(std::true_type{});
    } else {
      file_rows(std::false_type{});
    }
    DEVA_COMPILER_FENCE();
  }

  // ---- hand-over: every list is pruned to at most CAP = 64 entries (one per lane) and written with its
  // length.  A rank-counting round first; exact rounds only for lists still above CAP (an exact round
  // leaves <= 64 * ceil(c/64) * k / 64 entries: <= 2k <= 64 from 100).  The exact top-k
  // selection over all ranges happens in the merge kernel, where one wave per query gives thousands of
  // independent waves -- here it would run serially, 32 lists per wave.
  static_assert(LCAP <= 192, "two exact rounds must reach CAP");
  // (never taken: without this second test the compiler lays out the tile loop's exit branch differently, and the
  // kernel's ISA is held fixed against the measured one)
  if (!active) return;
  prune_over((uint32_t)CAP, true);
  prune_over((uint32_t)CAP, false);
  DEVA_COMPILER_FENCE();
  const int nq = min(QT, p.hw - q0);
  uint64_t* dst = p.part + ((int64_t)split * p.hw + q0) * CAP;
  if (lane < nq) p.part_cnt[(int64_t)split * p.hw + q0 + lane] = cnt;  // lanes 0..31 hold query l31 = lane
  for (int ql = 0; ql < nq; ++ql) {
    const uint32_t c = (uint32_t)__builtin_amdgcn_readlane((int)cnt, ql);
    if ((uint32_t)lane < c) {
      const uint32_t off = (uint32_t)ctk[ql * LSTRIDE + lane];
      const uint32_t token = ((off >> 5) * (uint32_t)p.splits + (uint32_t)split) * TOKT + (off & 31u);
      dst[(int64_t)ql * CAP + lane] =
          ((uint64_t)orderable(__uint_as_float(csc[ql * LSTRIDE + lane])) << 32) | (uint64_t)(~token);
    }
  }
}

// ---------------------------------------------------------------------------------------------------
// Workgroup-shared candidate lists.  The four waves of a workgroup own the SAME 32 queries and split the
// token tiles of the range among themselves (wave w visits tiles w, w+4, ... of the scrambled order);
// they append to one set of 32 lists through LDS atomics and filter against one threshold per query.
// Compared with four waves x four different query groups this
//  * tightens every threshold four times faster (fewer appends: ~k(1+ln(N/k)) per query for the WHOLE
//    range instead of per wave) and needs a quarter of the lists per workgroup, so each list gets four
//    times the slots (LCAP 352 with two workgroups per CU, 704 with one) and is pruned 2-3 times per
//    range instead of 4-6 -- the round-2 ablation showed appends + prunes costing 124 us of 376 us at
//    N = 10 000 x 8 160 (one third of the kernel), ~1 us per pruned list;
//  * gives one workgroup per 32 queries: 255 workgroups at 1080p without splitting the bank at all.
// Appends: a lane that passes reserves a slot with ds_add_rtn (16 independent atomics per tile are issued
// first, the entries written afterwards, so no append waits for its atomic).  Lists are checked between
// two barriers once per tile: wave w prunes lists 8w .. 8w+7 that could overflow during the next tile
// (at most 4 x 32 appends per query per tile).
template <int LCAP, int MINB, int NW>
__global__ __launch_bounds__(NW * 64, MINB) void affinity_topk_wg_kernel(const AffArgs p) {
  if (p.guard && *p.guard == 0u) return;  // uniform over the grid
  constexpr int LSTRIDE = LCAP + 1;
  constexpr int E = (LCAP + 63) / 64;          // list entries per lane in a prune
  constexpr int BURST = NW * TOKT;          // appends per query between two maintenance points
  constexpr int QW = QT / NW;               // lists maintained by one wave
  constexpr bool MS_EARLY = (E <= 6);
  static_assert(LCAP - BURST >= 64, "a list is pruned only when every lane holds an entry");
  static_assert(E * K_MAX <= LCAP - BURST, "one exact prune (<= E*k survivors) must get below the in-loop limit");
  static_assert(2 * K_MAX <= CAP && CAP == 64, "hand-over: one key per lane");
  __shared__ uint32_t s_sc[QT][LSTRIDE];  // candidate scores (fp32 bits)
  __shared__ uint16_t s_tk[QT][LSTRIDE];  // candidate tokens (offset inside this range)
  __shared__ uint32_t s_cnt[QT];
  __shared__ float s_tau[QT];
  __shared__ __attribute__((aligned(16))) float s_ms[NW][TOKT];
  __shared__ __attribute__((aligned(16))) uint32_t s_rank[NW][64];

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int l31 = lane & 31;
  const int half = lane >> 5;
  const int q0 = blockIdx.x * QT;
  const int split = blockIdx.y;
  uint32_t* srow = &s_sc[l31][0];
  uint16_t* trow = &s_tk[l31][0];
  float* msl = &s_ms[wave][0];

  // ---- query operand (registers, whole kernel), identical in the waves: mirrors load_query (affinity_common.h), inline
  // for the register allocation
  const int q = min(q0 + l31, p.hw - 1);
  float bqe[CK / 2], bqk[CK / 2];
  float bs[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int t = 0; t < CK / 2; ++t) {
    const float e0 = p.qe[(int64_t)(2 * t) * p.hw + q], e1 = p.qe[(int64_t)(2 * t + 1) * p.hw + q];
    const float k0 = p.qk[(int64_t)(2 * t) * p.hw + q], k1 = p.qk[(int64_t)(2 * t + 1) * p.hw + q];
    bs[t >> 3] += e0 * (k0 * k0);
    bs[t >> 3] += e1 * (k1 * k1);
    bqe[t] = half ? e1 : e0;
    bqk[t] = half ? (k1 * e1) : (k0 * e0);
  }
  const float bsq = ((bs[0] + bs[1]) + bs[2]) + bs[3];

  // ---- this range's tiles in scrambled order (see affinity_topk_kernel); wave w takes visits w, w+4, ...
  const int n_my = (p.total_tiles - split + p.splits - 1) / p.splits;
  int stride = 61;
  if (n_my % 61 == 0) stride = (n_my % 59 == 0) ? 53 : 59;
  const int n_vis = (n_my > wave) ? (n_my - wave + NW - 1) / NW : 0;  // visits of this wave
  const int n_iter = (n_my + NW - 1) / NW;                             // of the busiest wave
  int cyc = (n_my > 0) ? (int)(((int64_t)wave * stride) % n_my) : 0;
  const int step = (n_my > 0) ? (int)(((int64_t)NW * stride) % n_my) : 0;

  if (threadIdx.x < QT) {
    s_cnt[threadIdx.x] = 0u;
    s_tau[threadIdx.x] = DEVA_ABLATE(1) ? INFINITY : -INFINITY;
  }

  f32x4 xbuf[CK / 4];
  float ms_buf;
  auto prefetch = [&](int cyc_) __attribute__((always_inline)) {
    const int tile = split + p.splits * cyc_;
    const int n_mine = min(tile * TOKT + l31, p.n_total - 1);
    const float* krow = (n_mine < p.n_long) ? (p.key_long + (int64_t)n_mine * CK)
                                            : (p.key_work + (int64_t)(n_mine - p.n_long) * CK);
    ms_buf = ((n_mine < p.n_long) ? p.shr_long[n_mine] : p.shr_work[n_mine - p.n_long]);  // scaled when stored: see DEVA_KEEP_ROWS
    const float* shifted = krow + half;
#pragma unroll
    for (int j = 0; j < CK / 4 - 1; ++j) xbuf[j] = *reinterpret_cast<const f32x4_u*>(shifted + 4 * j);
    xbuf[CK / 4 - 1] = *reinterpret_cast<const f32x4*>(krow + CK - 4);
  };
  if (n_vis > 0) prefetch(cyc);

  // after the rank-counting prune of list qq: exact rounds while it is above `limit`, then publish length / threshold
  auto finish_prune = [&](int qq, int kept, uint32_t thr, uint32_t limit) __attribute__((always_inline)) {
    while ((uint32_t)kept > limit) {
      const uint32_t thr2 = prune_list_exact<E>(&s_sc[qq][0], &s_tk[qq][0], (uint32_t)kept, p.k, lane, &kept);
      thr = thr2 > thr ? thr2 : thr;
    }
    if (lane == 0) {
      s_cnt[qq] = (uint32_t)kept;
      const float t_new = from_orderable(thr);
      if (t_new > s_tau[qq]) s_tau[qq] = t_new;
    }
    DEVA_COMPILER_FENCE();
  };
  auto prune_one = [&](int qq, uint32_t c, uint32_t limit) __attribute__((always_inline)) {
    int kept = (int)c;
    const uint32_t thr = prune_list<E>(&s_sc[qq][0], &s_tk[qq][0], c, p.k, lane, &kept, &s_rank[wave][0]);
    finish_prune(qq, kept, thr, limit);
  };
  // the lists of `todo` this wave takes (every NW-th, starting with the wave-th: any wave can prune any list of the
  // workgroup); lengths from lane qq of c_l.  (Pruning two lists at a time, interleaved to cover each other's LDS round
  // trips, was measured: bit-identical, no faster -- profiles/r02e_affinity_shapes.txt item 11.)
  auto prune_share = [&](uint32_t todo, uint32_t c_l, uint32_t limit) __attribute__((always_inline)) {
    int nth = 0;
    while (todo) {
      const int qq = __ffs((int)todo) - 1;
      todo &= todo - 1;
      if ((nth++ % NW) == wave) prune_one(qq, (uint32_t)__builtin_amdgcn_readlane((int)c_l, qq), limit);
    }
  };

#ifdef DEVA_AFFINITY_PROBES
  uint64_t* pb = (p.probe && blockIdx.x < 8 && blockIdx.y == 0) ? p.probe + (size_t)(blockIdx.x * NW + wave) * 64 * 8 : nullptr;
#endif
  for (int it = 0; it < n_iter; ++it) {
    DEVA_STAMP(0);
    __syncthreads();  // every append of the previous tile has landed: the list lengths are final
    // every wave reads all 32 lengths and thresholds (one LDS access each) and takes the same decision
    const uint32_t c_l = s_cnt[l31];
    float tau = s_tau[l31];
    const uint32_t need = (uint32_t)__builtin_amdgcn_ballot_w64(c_l > (uint32_t)(LCAP - BURST));
    // every wave has read this tile's list lengths (and taken the same pruning decision) before anyone appends
    // again: without this barrier a fast wave's appends could change a slow wave's decision.  It follows the
    // first barrier directly, so the skew of a whole tile (MFMAs, scoring, appends) is collected once per tile.
    DEVA_COMPILER_FENCE();
    __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): the reads above
    __builtin_amdgcn_s_barrier();
    DEVA_COMPILER_FENCE();
    DEVA_STAMP(1);
    if (need) {  // uniform over the workgroup: some list could overflow during the next tile
      prune_share(need, c_l, (uint32_t)(LCAP - BURST));
      __syncthreads();  // pruned lists / raised thresholds are visible
      tau = s_tau[l31];
    }
    DEVA_STAMP(2);
    const bool work = it < n_vis;  // the ragged last round: a wave without a tile only keeps the barriers
    const int tile = split + p.splits * cyc;
    const int n_base = tile * TOKT;
    const uint32_t tok0 = (uint32_t)(cyc * TOKT + 4 * half);
    f32x16 accA, accB;
    float4 ms4[4];  // scaled shrinkage in accumulator-row order: rows 4g..4g+3 <-> tokens 8g+4*half..+3
    if (work) {
      // 1/sqrt(CK) folded in (exact); NaN past the end of the bank: such a score fails every threshold test, so
      // the ragged last tile needs no per-row bound check
      if (lane < TOKT) msl[lane] = (n_base + lane < p.n_total) ? ms_buf * 0.125f : __builtin_nanf("");
      DEVA_COMPILER_FENCE();
      // the MFMAs read the prefetched rows in place (channel 2t + half of this lane's token is x / z of the
      // 16-B pieces); the next tile's loads are issued after the last MFMA, under the scoring
      DEVA_KEEP_ROWS(xbuf);
      const float a30 = half ? xbuf[CK / 4 - 1][1] : xbuf[CK / 4 - 1][0];
      const float a31 = half ? xbuf[CK / 4 - 1][3] : xbuf[CK / 4 - 1][2];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        accA[r] = 0.0f;
        accB[r] = 0.0f;
      }
      if (!DEVA_ABLATE(8)) {
#pragma unroll
        for (int t = 0; t < CK / 2; ++t) {
          const float a = (t == CK / 2 - 2) ? a30 : (t == CK / 2 - 1) ? a31 : xbuf[t >> 1][(t & 1) * 2];
          accA = __builtin_amdgcn_mfma_f32_32x32x2f32(a * a, bqe[t], accA, 0, 0, 0);
          accB = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bqk[t], accB, 0, 0, 0);
        }
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          accA[r] = xbuf[r >> 2][r & 3];
          accB[r] = xbuf[4 + (r >> 2)][r & 3];
        }
      }
      DEVA_COMPILER_FENCE();
      DEVA_STAMP(3);
      if (it + 1 < n_vis) {
        cyc += step;
        cyc = cyc >= n_my ? cyc - n_my : cyc;
        if (!DEVA_ABLATE(2)) prefetch(cyc);
      }
      // this wave's own shrinkage row, read back before the barrier so that its LDS latency is not exposed after
      // it (the 8-wave instantiation has no registers to spare for that and reads it after the barrier)
      if (MS_EARLY) {
#pragma unroll
        for (int g = 0; g < 4; ++g) ms4[g] = *reinterpret_cast<const float4*>(&msl[8 * g + 4 * half]);
      }
    }
    DEVA_COMPILER_FENCE();
    DEVA_STAMP(4);
    DEVA_STAMP(5);
    if (!work) continue;
    if (DEVA_ABLATE(4)) {
      if (accA[0] + accB[15] == 12345.678f) s_cnt[0] = 1u;
      continue;
    }

    // ---- scores of this lane: query l31, tokens n_base + (r&3) + 8*(r>>2) + 4*half.  Phase A: compare
    // and reserve list slots (one LDS atomic per passing lane and row, none waited for); phase B: write.
    if (!MS_EARLY) {
#pragma unroll
      for (int g = 0; g < 4; ++g) ms4[g] = *reinterpret_cast<const float4*>(&msl[8 * g + 4 * half]);
    }
    float v[16];
    uint32_t pos[16];
    unsigned long long okm[16];
    const f32x2 bsq2 = {bsq, bsq};
#pragma unroll
    for (int r2 = 0; r2 < 8; ++r2) {  // two accumulator rows per packed-fp32 instruction
      const f32x2 a2 = {accA[2 * r2], accA[2 * r2 + 1]};
      const f32x2 b2 = {accB[2 * r2], accB[2 * r2 + 1]};
      const float4 m4 = ms4[r2 >> 1];
      const f32x2 m2 = (r2 & 1) ? f32x2{m4.z, m4.w} : f32x2{m4.x, m4.y};
      const f32x2 v2 = (((b2 + b2) - a2) - bsq2) * m2;  // == ((-A + 2B) - bsq) * ms / 8, every step correctly rounded
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int r = 2 * r2 + h;
        v[r] = v2[h];
        const bool ok = v[r] >= tau;
        okm[r] = __builtin_amdgcn_ballot_w64(ok);
        // lanes that do not pass write to the spare slot LCAP of their row (never read): no predicate in phase B
        pos[r] = (uint32_t)LCAP;
        if (ok) pos[r] = atomicAdd(&s_cnt[l31], 1u);
      }
    }
    DEVA_STAMP(6);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      if (okm[r]) {
        const int j0 = (r & 3) + 8 * (r >> 2);
        srow[pos[r]] = __float_as_uint(v[r]);
        trow[pos[r]] = (uint16_t)(tok0 + j0);
      }
    }
    DEVA_COMPILER_FENCE();
    DEVA_STAMP(7);
  }

  // ---- hand-over: every list down to at most CAP entries (exact rounds, if needed, shrink 704 -> 352 -> 192 -> 96 ->
  // 64 at worst), then wave w writes lists w*QW .. with their lengths
  __syncthreads();
  {
    const uint32_t c_l = s_cnt[l31];
    const uint32_t over = (uint32_t)__builtin_amdgcn_ballot_w64(c_l > (uint32_t)CAP);
    prune_share(over, c_l, (uint32_t)CAP);
  }
  __syncthreads();  // lists pruned by other waves are visible
  DEVA_COMPILER_FENCE();
  for (int qq = wave * QW; qq < wave * QW + QW; ++qq) {
    if (q0 + qq >= p.hw) break;
    const uint32_t c = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_cnt[qq]);
    const int64_t list = (int64_t)split * p.hw + q0 + qq;
    if (lane == 0) p.part_cnt[list] = c;
    if ((uint32_t)lane < c) {
      const uint32_t off = (uint32_t)s_tk[qq][lane];
      const uint32_t token = ((off >> 5) * (uint32_t)p.splits + (uint32_t)split) * TOKT + (off & 31u);
      p.part[list * CAP + lane] = ((uint64_t)orderable(__uint_as_float(s_sc[qq][lane])) << 32) | (uint64_t)(~token);
    }
  }
}

// one wave per query: exact top-k over the candidate lists of all ranges (lane l holds entry l of every
// range's list: ME >= splits keys per lane), sorted by rank counting, then exp / normalise / usage.
// With out_keys != NULL the sorted top-k is instead written back in the hand-over format (token index
// shifted by token_offset): the per-shard selection of a token-sharded bank, merged by a second pass of
// this kernel over the gathered lists of all shards.
template <int ME>
__global__ __launch_bounds__(256) void affinity_finalize_kernel(const uint64_t* __restrict__ part,
                                                                const uint32_t* __restrict__ part_cnt, int hw, int k,
                                                                int splits, int32_t* __restrict__ idx,
                                                                float* __restrict__ weight,
                                                                unsigned long long* __restrict__ usage_fix,
                                                                uint64_t* __restrict__ out_keys,
                                                                uint32_t* __restrict__ out_cnt, uint32_t token_offset,
                                                                const uint32_t* __restrict__ guard) {
  if (guard && *guard == 0u) return;  // fall-back of the fp16 pre-filter: nothing to do
  __shared__ uint64_t s_buf[4][2][64];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int q = blockIdx.x * 4 + wave;
  if (q >= hw) return;
  volatile uint64_t* unsorted = &s_buf[wave][0][0];
  volatile uint64_t* sorted = &s_buf[wave][1][0];

  const int n_live = splits;
  uint64_t e[ME];
#pragma unroll
  for (int i = 0; i < ME; ++i) {
    uint64_t v = 0ull;
    if (i < splits) {  // key and length loads are independent (one memory round trip): slots past the length are
      const int64_t list = (int64_t)i * hw + q;  // allocated workspace, read and discarded
      const uint64_t key = part[list * CAP + lane];
      v = ((uint32_t)lane < part_cnt[list]) ? key : 0ull;
    }
    e[i] = v;
  }
  const uint64_t thr = kth_largest<ME>(e, n_live, k);
  // compact the k survivors into LDS (any order), then sort them by rank counting
  int base = 0;
#pragma unroll
  for (int i = 0; i < ME; ++i) {
    if (i < n_live) {
      const bool keep = e[i] >= thr && e[i] != 0ull;
      const unsigned long long b = __builtin_amdgcn_ballot_w64(keep);
      if (keep) unsorted[base + prefix_below(b)] = e[i];
      base += __popcll(b);
    }
  }
  DEVA_COMPILER_FENCE();
  const uint64_t cand = (lane < k && lane < base) ? unsorted[lane] : missing_slot_key(lane);
  const uint64_t best = rank_sort_k(cand, k, k, lane, sorted);
  if (out_keys) {
    write_out_keys(best, lane, q, k, out_keys, out_cnt, token_offset);
    return;
  }
  softmax_usage_tail(best, lane, q, k, idx, weight, usage_fix);
}

__global__ void usage_update_kernel(unsigned long long* __restrict__ usage_fix, int64_t offset,
                                    float* __restrict__ use, float* __restrict__ life, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const unsigned long long f = usage_fix[offset + i];
  usage_fix[offset + i] = 0ull;
  if (use) use[i] += (float)((double)f * (1.0 / (double)TWO40));
  if (life) life[i] += 1.0f;
}

// ------------------------------------------------------------------ sparse readout
// block = 256 threads = 4 waves; tile = 8 queries x 256 channels.  A wave gathers the k value rows
// of 2 queries (each lane a float4 of the 1-KiB row slab), accumulates in registers, and the tile
// is transposed through LDS so each [cv][hw] output row is written as one 32-B segment.
constexpr int RQ = 8;     // queries per block (small tiles: a 480p frame still yields ~400 workgroups)
constexpr int RC = 256;   // channels per block

__global__ __launch_bounds__(256) void readout_sparse_kernel(const int32_t* __restrict__ idx,
                                                             const float* __restrict__ weight, int hw, int k,
                                                             const float* __restrict__ val_long, int n_long,
                                                             const float* __restrict__ val_work, int cv,
                                                             float* __restrict__ out, int tok_lo, int tok_hi,
                                                             const int32_t* __restrict__ map_long,
                                                             const int32_t* __restrict__ map_work) {
  __shared__ float tile[RC][RQ + 1];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int q0 = blockIdx.x * RQ;
  const int c0 = blockIdx.y * RC;
  const int cl = lane * 4;  // channel offset inside the slab
  const bool c_ok = (c0 + cl) < cv;  // cv is a multiple of 4
  for (int qi = 0; qi < RQ / 4; ++qi) {
    const int ql = wave * (RQ / 4) + qi;
    const int q = q0 + ql;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (q < hw) {  // (wave-uniform)
      // lane j resolves term j of the query once: arena row and weight (0 for a term this launch does not add:
      // token of another bank shard, row stored on another rank); then the rows are fetched eight at a time --
      // independent 16-byte loads in flight instead of an index -> row dependency chain per term
      int row = 0, is_long = 0;
      float wj = 0.0f;
      bool live = false;
      if (lane < k) {
        const int t = idx[(int64_t)q * k + lane];
        wj = weight[(int64_t)q * k + lane];
        is_long = (t < n_long) ? 1 : 0;
        row = is_long ? t : t - n_long;
        live = t >= tok_lo && t < tok_hi;
        const int32_t* map = is_long ? map_long : map_work;
        if (live && map) {
          row = map[row];
          live = row >= 0;
        }
        if (!live) {
          row = 0;
          wj = 0.0f;
          is_long = n_long > 0 ? is_long : 0;
        }
      }
      // a term this launch does not add is SKIPPED, not added with weight 0: its stand-in row (row 0 of an arena that may be
      // uninitialised on a rank without local rows) never enters the sum, so 0 * NaN cannot either
      const uint64_t live_bits = __builtin_amdgcn_ballot_w64(live);
      const float* col = nullptr;
      for (int j0 = 0; j0 < k; j0 += 8) {
        float4 v[8];
        float w8[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int j = min(j0 + u, k - 1);
          const int r = __builtin_amdgcn_readlane(row, j);
          const int lg = __builtin_amdgcn_readlane(is_long, j);
          w8[u] = (j0 + u < k) ? __int_as_float(__builtin_amdgcn_readlane(__float_as_int(wj), j)) : 0.0f;
          col = (lg ? val_long : val_work) + (int64_t)r * cv + c0 + cl;
          v[u] = c_ok ? *reinterpret_cast<const float4*>(col) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {  // terms in index order, like the one-at-a-time loop: same sums
          if ((live_bits >> (j0 + u)) & 1ull) {
            acc.x += w8[u] * v[u].x;
            acc.y += w8[u] * v[u].y;
            acc.z += w8[u] * v[u].z;
            acc.w += w8[u] * v[u].w;
          }
        }
      }
    }
    tile[cl + 0][ql] = acc.x;
    tile[cl + 1][ql] = acc.y;
    tile[cl + 2][ql] = acc.z;
    tile[cl + 3][ql] = acc.w;
  }
  __syncthreads();
  const int tq = threadIdx.x % RQ;
  const int tc = threadIdx.x / RQ;  // 0 .. 256/RQ - 1
  if (q0 + tq < hw) {
    for (int c = tc; c < RC; c += 256 / RQ) {
      if (c0 + c < cv) out[(int64_t)(c0 + c) * hw + q0 + tq] = tile[c][tq];
    }
  }
}

}  // namespace
}  // namespace deva

using namespace deva;

extern "C" int64_t deva_affinity_workspace(int hw, int k, int splits) {
  (void)k;
  // [splits][hw][CAP] 64-bit candidate keys, then [splits][hw] 32-bit list lengths
  return (int64_t)splits * hw * CAP + ((int64_t)splits * hw + 1) / 2;
}

// kernel shapes (the numbers are part of the interface: deva_affinity_force_shape, DEVA_AFFINITY_SHAPE):
// 2 = affinity_topk_kernel: per-wave 100-slot lists, two workgroups per CU;
// 4 = affinity_topk_wg_kernel: workgroup-shared lists, 4 waves x the same 32 queries, 352 slots, two workgroups per CU;
// 8 = affinity_topk_wg_kernel: EIGHT waves x the same 32 queries, 704 slots, one workgroup per CU.
// (1, 3, 5, 6, 7 were A/B variants -- one workgroup per CU, key tiles through LDS, early prefetch, ping-pong phases --
// measured bit-identical and slower in round 2, profiles/r02e_affinity_shapes.txt, and are gone.)
// DEVA_AFFINITY_SHAPE overrides the choice (tuning / A-B measurements only).
static int g_forced_shape = -1;  // -1: not initialised (DEVA_AFFINITY_SHAPE is read on first use)

static int affinity_shape(int n_total, int hw) {
  if (g_forced_shape < 0) {
    const char* e = getenv("DEVA_AFFINITY_SHAPE");
    const int v = e ? atoi(e) : 0;
    g_forced_shape = (v == 2 || v == 4 || v == 8) ? v : 0;
  }
  if (g_forced_shape) return g_forced_shape;
  // measured (profiles/r02e_affinity_shapes.txt, total us of filter + finalize):
  //   few query blocks (480p, hw = 1 620): the 8-wave workgroups need half the token ranges for the same number
  //   of workgroups, i.e. half the lists to merge: 42 vs 71 (N = 1 620), 83 vs 94 (8 100), 192 vs 200 (24 580);
  //   from ~30 000 tokens on the 4-wave shape is ahead (286 vs 300 at 40 000) and stays ahead of the per-wave lists
  //   (518 vs 624 at 83 440);
  //   many query blocks (1080p / 4K): shared lists while appends / prunes dominate (312 vs 362 at 10 000 x 8 160,
  //   1 114 vs 1 195 at 10 000 x 32 400), per-wave lists without barriers on longer banks (829 vs 859 at 30 000,
  //   1 039 vs 1 118 at 40 000, 1 873 vs 2 128 at 83 440 x 8 160).
  if (hw <= 4096) return n_total <= 30000 ? 8 : 4;
  return n_total <= 20000 ? 4 : 2;
}

extern "C" int deva_affinity_force_shape(int shape) {
  DEVA_REQUIRE(shape == 0 || shape == 2 || shape == 4 || shape == 8,
               "deva_affinity_force_shape: shape must be 0 (automatic), 2, 4 or 8, not %d", shape);
  g_forced_shape = shape;
  return 0;
}

#ifdef DEVA_AFFINITY_PROBES
static uint64_t* g_probe = nullptr;
// probe builds only (not part of the ABI): device buffer of 8 workgroups x 8 waves x 64 tiles x 8 cycle stamps
extern "C" int deva_affinity_set_probe(uint64_t* buf) {
  g_probe = buf;
  return 0;
}
#endif

extern "C" int deva_affinity_default_splits(int n_total, int hw) {
  // aim at one resident set of workgroups: 256 CUs x (1 or 2) four-wave workgroups
  const int shape = affinity_shape(n_total, hw);
  const int slots = (shape == 2 || shape == 4) ? 512 : 256;
  const bool wg_lists = shape == 4 || shape == 8;
  const int qblocks = (int)ceil_div(hw, wg_lists ? QT : WAVES * QT);
  if (shape == 8) {
    // one 8-wave workgroup per CU, every token range hands over one list per query
    const int tiles8 = (int)ceil_div(n_total, TOKT);
    int r = (256 + qblocks / 2) / qblocks;
    if (r > tiles8 / 16) r = tiles8 / 16;  // >= 2 tiles per wave and range
    if (r > MAX_SPLITS) r = MAX_SPLITS;
    if (r < 1) r = 1;
    while (r < MAX_SPLITS && ceil_div(tiles8, r) > 2047) ++r;
    return r;
  }
  const int tiles = (int)ceil_div(n_total, TOKT);
  // workgroup-shared lists: the grid should be a whole number of resident sets (round, do not overshoot)
  int s = wg_lists ? (slots + qblocks / 2) / qblocks : (int)ceil_div(slots, qblocks);
  if (s > tiles / 4) s = tiles / 4;  // keep >= 4 tiles (128 tokens) per range
  if (s > MAX_SPLITS) s = MAX_SPLITS;
  if (s < 1) s = 1;
  // small banks (first memory frames of a clip): ranges of <= CAP tokens hand every score over without
  // building a threshold or pruning
  const int s_nofilter = (int)ceil_div(tiles, CAP / TOKT);
  if (s_nofilter <= MAX_SPLITS && s_nofilter > s) s = s_nofilter;
  while (s < MAX_SPLITS && ceil_div(tiles, s) > 2047) ++s;  // 16-bit token offsets inside a range
  return s;
}

int deva::topk_fp32(const float* key_long, const float* shr_long, int n_long, const float* key_work,
                    const float* shr_work, int n_work, const float* qk, const float* qe, int hw, int k, int splits,
                    uint64_t* part_keys, void* stream, const uint32_t* guard) {
  DEVA_REQUIRE(qk && qe && part_keys && hw > 0, "deva_affinity_topk: bad query args");
  DEVA_REQUIRE(n_long >= 0 && n_work >= 0, "deva_affinity_topk: negative bank size");
  DEVA_REQUIRE(n_long == 0 || (key_long && shr_long), "deva_affinity_topk: null long-term segment");
  DEVA_REQUIRE(n_work == 0 || (key_work && shr_work), "deva_affinity_topk: null working segment");
  DEVA_REQUIRE(k >= 1 && k <= K_MAX, "deva_affinity_topk: k=%d unsupported (1..%d)", k, K_MAX);
  const int64_t n_total = (int64_t)n_long + n_work;
  DEVA_REQUIRE(n_total >= k, "deva_affinity_topk: selected index k out of range (bank has %lld tokens, k=%d)",
               (long long)n_total, k);
  DEVA_REQUIRE(n_total < (1ll << 31), "deva_affinity_topk: bank too large");
  DEVA_REQUIRE(splits >= 1 && splits <= MAX_SPLITS, "deva_affinity_topk: splits must be 1..%d", MAX_SPLITS);
  AffArgs a;
  a.key_long = key_long ? key_long : key_work;
  a.shr_long = shr_long ? shr_long : shr_work;
  a.n_long = n_long;
  a.key_work = key_work ? key_work : key_long;
  a.shr_work = shr_work ? shr_work : shr_long;
  a.n_total = (int)n_total;
  a.qk = qk;
  a.qe = qe;
  a.hw = hw;
  a.k = k;
  a.splits = splits;
  a.total_tiles = (int)ceil_div(n_total, TOKT);
  DEVA_REQUIRE(ceil_div(a.total_tiles, splits) <= 2047,
               "deva_affinity_topk: %d tokens per range exceed the 16-bit in-range token offset; use more splits",
               (int)ceil_div(a.total_tiles, splits) * TOKT);
  a.part = part_keys;
  a.part_cnt = reinterpret_cast<uint32_t*>(part_keys + (int64_t)splits * hw * CAP);
#ifdef DEVA_AFFINITY_PROBES  // `make PROBES=1`: timing probes for the ablation table (profiles/r02b_affinity_shapes.txt)
  static const int ablate = [] {
    const char* e = getenv("DEVA_AFFINITY_ABLATE");
    return e ? atoi(e) : 0;
  }();
  a.ablate = ablate;
  a.probe = g_probe;
#else
  a.ablate = 0;
  a.probe = nullptr;
#endif
  a.guard = guard;
  dim3 grid((unsigned)ceil_div(hw, WAVES * QT), (unsigned)splits);
  const dim3 grid_wg((unsigned)ceil_div(hw, QT), (unsigned)splits);
  switch (affinity_shape((int)n_total, hw)) {
    case 8:
      hipLaunchKernelGGL((affinity_topk_wg_kernel<704, 1, 8>), grid_wg, dim3(8 * 64), 0, (hipStream_t)stream, a);
      break;
    case 4:
      hipLaunchKernelGGL((affinity_topk_wg_kernel<352, 2, WAVES>), grid_wg, dim3(WAVES * 64), 0, (hipStream_t)stream, a);
      break;
    default:  // 2
      hipLaunchKernelGGL((affinity_topk_kernel<LCAP_DUAL, 2>), grid, dim3(WAVES * 64), 0, (hipStream_t)stream, a);
  }
  return check_launch("deva_affinity_topk");
}

extern "C" int deva_affinity_topk(const float* key_long, const float* shr_long, int n_long, const float* key_work,
                                  const float* shr_work, int n_work, const float* qk, const float* qe, int hw,
                                  int k, int splits, uint64_t* part_keys, void* stream) {
  return topk_fp32(key_long, shr_long, n_long, key_work, shr_work, n_work, qk, qe, hw, k, splits, part_keys, stream,
                   nullptr);
}

int deva::launch_merge(const uint64_t* keys, const uint32_t* cnt, int hw, int k, int lists, int32_t* idx, float* weight,
                       uint64_t* usage_fix, uint64_t* out_keys, uint32_t* out_cnt, uint32_t token_offset, void* stream,
                       const char* what, const uint32_t* guard) {
  const dim3 grid((unsigned)ceil_div(hw, 4));
#define DEVA_MERGE(ME)                                                                                            \
  hipLaunchKernelGGL(affinity_finalize_kernel<ME>, grid, dim3(256), 0, (hipStream_t)stream, keys, cnt, hw, k, lists, \
                     idx, weight, (unsigned long long*)usage_fix, out_keys, out_cnt, token_offset, guard)
  if (lists <= 4) {
    DEVA_MERGE(4);
  } else if (lists <= 8) {
    DEVA_MERGE(8);
  } else if (lists <= 16) {
    DEVA_MERGE(16);
  } else {
    DEVA_MERGE(32);
  }
#undef DEVA_MERGE
  return check_launch(what);
}

extern "C" int deva_affinity_finalize(const uint64_t* part_keys, int hw, int k, int splits, int32_t* idx,
                                      float* weight, uint64_t* usage_fix, void* stream) {
  DEVA_REQUIRE(part_keys && idx && weight && hw > 0, "deva_affinity_finalize: bad args");
  DEVA_REQUIRE(k >= 1 && k <= K_MAX && splits >= 1 && splits <= MAX_SPLITS,
               "deva_affinity_finalize: k/splits out of range");
  const uint32_t* cnt = reinterpret_cast<const uint32_t*>(part_keys + (int64_t)splits * hw * CAP);
  return launch_merge(part_keys, cnt, hw, k, splits, idx, weight, usage_fix, nullptr, nullptr, 0u, stream,
                      "deva_affinity_finalize");
}

extern "C" int deva_affinity_select(const uint64_t* part_keys, int hw, int k, int splits, int64_t token_offset,
                                    uint64_t* out_keys, uint32_t* out_counts, void* stream) {
  DEVA_REQUIRE(part_keys && out_keys && out_counts && hw > 0, "deva_affinity_select: bad args");
  DEVA_REQUIRE(k >= 1 && k <= K_MAX && splits >= 1 && splits <= MAX_SPLITS,
               "deva_affinity_select: k/splits out of range");
  DEVA_REQUIRE(token_offset >= 0 && token_offset < (1ll << 31), "deva_affinity_select: bad token offset");
  const uint32_t* cnt = reinterpret_cast<const uint32_t*>(part_keys + (int64_t)splits * hw * CAP);
  return launch_merge(part_keys, cnt, hw, k, splits, nullptr, nullptr, nullptr, out_keys, out_counts,
                      (uint32_t)token_offset, stream, "deva_affinity_select");
}

extern "C" int deva_affinity_merge(const uint64_t* keys, const uint32_t* counts, int hw, int k, int lists, int32_t* idx,
                                   float* weight, uint64_t* usage_fix, void* stream) {
  DEVA_REQUIRE(keys && counts && idx && weight && hw > 0, "deva_affinity_merge: bad args");
  DEVA_REQUIRE(k >= 1 && k <= K_MAX && lists >= 1 && lists <= MAX_SPLITS,
               "deva_affinity_merge: k/lists out of range");
  return launch_merge(keys, counts, hw, k, lists, idx, weight, usage_fix, nullptr, nullptr, 0u, stream,
                      "deva_affinity_merge");
}

extern "C" int deva_usage_update(uint64_t* usage_fix, int64_t offset, float* use, float* life, int n,
                                 void* stream) {
  DEVA_REQUIRE(usage_fix && n >= 0 && offset >= 0, "deva_usage_update: bad args");
  if (n == 0) return 0;
  hipLaunchKernelGGL(usage_update_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream,
                     (unsigned long long*)usage_fix, offset, use, life, n);
  return check_launch("deva_usage_update");
}

extern "C" int deva_readout_sparse(const int32_t* idx, const float* weight, int hw, int k, const float* val_long,
                                   int n_long, const float* val_work, int cv, float* out, int tok_lo, int tok_hi,
                                   const int32_t* map_long, const int32_t* map_work, void* stream) {
  DEVA_REQUIRE(idx && weight && out && hw > 0 && k > 0 && cv > 0, "deva_readout_sparse: bad args");
  DEVA_REQUIRE(k <= 64, "deva_readout_sparse: k=%d unsupported (one term per lane: 1..64)", k);
  DEVA_REQUIRE(cv % 4 == 0, "deva_readout_sparse: value dim must be a multiple of 4");
  DEVA_REQUIRE(n_long == 0 || val_long, "deva_readout_sparse: null long-term values");
  const float* vl = val_long ? val_long : val_work;
  const float* vw = val_work ? val_work : val_long;
  DEVA_REQUIRE(vl && vw, "deva_readout_sparse: no value segment");
  dim3 grid((unsigned)ceil_div(hw, RQ), (unsigned)ceil_div(cv, RC));
  hipLaunchKernelGGL(readout_sparse_kernel, grid, dim3(256), 0, (hipStream_t)stream, idx, weight, hw, k, vl, n_long,
                     vw, cv, out, tok_lo, tok_hi, map_long, map_work);
  return check_launch("deva_readout_sparse");
}

