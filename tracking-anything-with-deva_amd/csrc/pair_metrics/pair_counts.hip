// deva_pair_counts (include/deva_pair_metrics.h, rules P1-P5): for up to 64 ground-truth objects and up to 64 proposals
// with tables of their own, the area and boundary pixels of every object and proposal and, for every (g, p) pair, the
// intersection and the boundary pixels of either that the other matches.  One bit per slot in a 64-bit word per pixel
// and side, as in csrc/vos_metrics/boundary_counts.hip, whose helpers wave_or / search_box have a second copy
// here: that file is pinned by its own tests and stays as it is.
//
// pair_label_kernel: a lane takes a strip of 8 pixels of one row and reads that row and the next, 9 values each, once.
// The slot of a value (P1) comes from the side's id table in LDS by binary search, or from pred_lut, and only when the
// value differs from the lane's previous one.  The two boundary words of a pixel (P2) go to the scratch side by side,
// one 16-byte store per pixel.  Areas and joint (g, p) counts are added as runs to a per-workgroup table in LDS whose
// non-zero cells are flushed with one integer atomic each.
//
// pair_match_kernel: a wave takes 64 consecutive pixels, a lane each, one 16-byte load.  A pixel whose words are not
// both zero needs the OR of the other side's words over the whole disk of P4 -- no "my own bit is matched" exit exists
// for a pair table, and there is no saturation exit either.  With radius <= 3 every lane walks its own (compile-time)
// box; with a larger radius the 64 lanes walk one pixel's box together, four cells each per step, and reduce across
// the wave.  Then, for every object g present among the 64 own words, one ballot per proposal p present among the words
// those pixels saw gives the count of [g][p]; lane p holds it and the lanes add one row segment to the workgroup's
// table in LDS (2 x n_gt x n_pred x 4 bytes, 32 KB at 64 x 64), and the same the other way round.  Boundary pixels per
// slot stay in registers, lane i for slot i.  One integer atomic per non-zero cell of the workgroup at the end.
// Integer adds everywhere: exact, and independent of the order.
#include <hip/hip_runtime.h>
#include <limits.h>

#include "../plane_values.h"
#include "pair_plan.h"

namespace deva_pair {
namespace {

constexpr int S = DEVA_PAIR_STRIP;
constexpr int N = DEVA_PAIR_MAX_OBJECTS;
static_assert(kWave == N, "lane i of a wave counts slot i");

using plane_values::bit_of;
using plane_values::find_slot;   // P1: the slot of a value in one side's table, -1 for none
using plane_values::load_value;
static_assert(DEVA_PAIR_U8 == plane_values::kU8 && DEVA_PAIR_I32 == plane_values::kI32 && DEVA_PAIR_I64 == plane_values::kI64 &&
                  DEVA_PAIR_INDEX16 == plane_values::kIndex16,
              "the encodings of plane_values.h");

// P2 for one pixel: own slot a against the slots of the E / S / SE neighbours that exist
__device__ __forceinline__ uint64_t boundary_word(int a, int e, int s, int se, bool has_e, bool has_s) {
  uint64_t w = 0;
  if (has_e && e != a) w |= bit_of(a) | bit_of(e);
  if (has_s && s != a) w |= bit_of(a) | bit_of(s);
  if (has_e && has_s && se != a) w |= bit_of(a) | bit_of(se);
  return w;
}

template <int GT, int PR>
__global__ __launch_bounds__(kBlock) void pair_label_kernel(const void* __restrict__ gt, const int* __restrict__ gt_ids, int n_gt,
                                                           const void* __restrict__ pred, const int* __restrict__ pred_ids, int n_pred,
                                                           const uint16_t* __restrict__ lut, int channels, int height, int width,
                                                           ulonglong2* __restrict__ words, uint32_t* __restrict__ singles,
                                                           uint32_t* __restrict__ pairs) {
  extern __shared__ int smem[];  // both id tables [n_gt + n_pred], the areas [n_gt + n_pred], the joint counts [n_gt][n_pred]
  const int slots = n_gt + n_pred, cells = n_gt * n_pred;
  int* table_g = smem;
  int* table_p = smem + n_gt;
  uint32_t* area = reinterpret_cast<uint32_t*>(smem + slots);
  uint32_t* joint = area + slots;
  const int tid = threadIdx.x;
  for (int i = tid; i < n_gt; i += kBlock) table_g[i] = gt_ids[i];
  if constexpr (PR != DEVA_PAIR_INDEX16)
    for (int i = tid; i < n_pred; i += kBlock) table_p[i] = pred_ids[i];
  for (int i = tid; i < slots + cells; i += kBlock) area[i] = 0u;
  __syncthreads();

  int last_g = 0, slot_g = find_slot<GT>(0, table_g, n_gt, nullptr, 0);
  int last_p = 0, slot_p = find_slot<PR>(0, table_p, n_pred, lut, channels);
  const int strips_per_row = (width + S - 1) / S;
  const int64_t strips = (int64_t)height * strips_per_row;
  for (int64_t s = (int64_t)blockIdx.x * kBlock + tid; s < strips; s += (int64_t)gridDim.x * kBlock) {
    const int y = (int)(s / strips_per_row);
    const int x0 = (int)(s - (int64_t)y * strips_per_row) * S;
    const bool has_s = y + 1 < height;
    int g[2][S + 1], p[2][S + 1];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
#pragma unroll
      for (int k = 0; k <= S; ++k) {
        g[r][k] = p[r][k] = -1;
        if (x0 + k < width && (r == 0 || has_s)) {
          const int64_t at = (int64_t)(y + r) * width + x0 + k;
          const int vg = load_value<GT>(gt, at);
          if (vg != last_g) last_g = vg, slot_g = find_slot<GT>(vg, table_g, n_gt, nullptr, 0);
          const int vp = load_value<PR>(pred, at);
          if (vp != last_p) last_p = vp, slot_p = find_slot<PR>(vp, table_p, n_pred, lut, channels);
          g[r][k] = slot_g, p[r][k] = slot_p;
        }
      }
    }
    int run_g = -1, run_p = -1;
    uint32_t run = 0;
    auto flush = [&]() {
      if (run_g >= 0) atomicAdd(&area[run_g], run);
      if (run_p >= 0) atomicAdd(&area[n_gt + run_p], run);
      if (run_g >= 0 && run_p >= 0) atomicAdd(&joint[run_g * n_pred + run_p], run);
    };
#pragma unroll
    for (int k = 0; k < S; ++k) {
      if (x0 + k < width) {
        const bool has_e = x0 + k + 1 < width;
        ulonglong2 w;
        w.x = boundary_word(g[0][k], g[0][k + 1], g[1][k], g[1][k + 1], has_e, has_s);
        w.y = boundary_word(p[0][k], p[0][k + 1], p[1][k], p[1][k + 1], has_e, has_s);
        words[(int64_t)y * width + x0 + k] = w;
        if (g[0][k] == run_g && p[0][k] == run_p) {
          ++run;
        } else {
          if (run) flush();
          run_g = g[0][k], run_p = p[0][k], run = 1u;
        }
      }
    }
    if (run) flush();
  }
  __syncthreads();
  for (int i = tid; i < slots; i += kBlock) {
    const uint32_t v = area[i];
    if (v) atomicAdd(&singles[i * DEVA_PAIR_SINGLE_FIELDS], v);
  }
  for (int i = tid; i < cells; i += kBlock) {
    const uint32_t v = joint[i];
    if (v) atomicAdd(&pairs[i * DEVA_PAIR_FIELDS], v);
  }
}

// or over the 64 lanes, the same value in every lane: four rotations inside each row of 16 lanes (data-parallel
// primitives, no LDS traffic), then the four rows through scalar registers
__device__ __forceinline__ uint32_t wave_or32(uint32_t v) {
  int x = (int)v;
  x |= __builtin_amdgcn_update_dpp(0, x, 0x121, 0xf, 0xf, false);  // row_ror:1
  x |= __builtin_amdgcn_update_dpp(0, x, 0x122, 0xf, 0xf, false);  // row_ror:2
  x |= __builtin_amdgcn_update_dpp(0, x, 0x124, 0xf, 0xf, false);  // row_ror:4
  x |= __builtin_amdgcn_update_dpp(0, x, 0x128, 0xf, 0xf, false);  // row_ror:8
  return (uint32_t)(__builtin_amdgcn_readlane(x, 0) | __builtin_amdgcn_readlane(x, 16) | __builtin_amdgcn_readlane(x, 32) |
                    __builtin_amdgcn_readlane(x, 48));
}

__device__ __forceinline__ uint64_t wave_or(uint64_t v) {
  return ((uint64_t)wave_or32((uint32_t)(v >> 32)) << 32) | wave_or32((uint32_t)v);
}

// or of the words of the cells of the box of radius `box` around (py, px) that lie in the disk of radius^2 = r2 and in
// the image, the cells dealt to the wave's lanes; magic = floor(2^32 / side) + 1 divides every cell index < 2^17 exactly
// (side <= 257: at most 66 049 cells).  Every load is clamped into the image, so its address is inside the scratch.
__device__ __forceinline__ void search_box(const ulonglong2* __restrict__ words, int height, int width, int py, int px, int box,
                                           int r2, int lane, uint64_t& seen_g, uint64_t& seen_p) {
  const uint32_t side = 2u * (uint32_t)box + 1u;
  const uint32_t cells = side * side;
  const uint32_t magic = (uint32_t)(0x100000000ull / side) + 1u;
  constexpr int U = 4;  // cells of a lane in flight together: the loads are unconditional, the words masked
  for (uint32_t first = (uint32_t)lane; first < cells; first += kWave * U) {
    ulonglong2 w[U];
    bool in[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t c = first + (uint32_t)u * kWave;
      const uint32_t row = __umulhi(c, magic);
      const int dy = (int)row - box, dx = (int)(c - row * side) - box;
      const int y = py + dy, x = px + dx;
      in[u] = c < cells && dx * dx + dy * dy <= r2 && y >= 0 && y < height && x >= 0 && x < width;
      w[u] = words[(int64_t)(y < 0 ? 0 : y >= height ? height - 1 : y) * width + (x < 0 ? 0 : x >= width ? width - 1 : x)];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) seen_g |= in[u] ? w[u].x : 0ull, seen_p |= in[u] ? w[u].y : 0ull;
  }
}

// one side of the pair table for the wave's 64 pixels: `own` is a pixel's word of the counted side, `saw` what its disk
// holds of the other.  For every slot a among the own words: lane a adds the pixels that carry it to `boundary`, and
// for every slot b those pixels saw, lane b gets the count of (a, b); the lanes then add the row segment to
// table[a * stride_a + b * stride_b].  Every loop runs on scalar masks: uniform over the wave.
__device__ __forceinline__ void count_side(uint64_t own, uint64_t saw, int lane, uint32_t& boundary, uint32_t* table, int stride_a,
                                           int stride_b) {
  uint64_t present = wave_or(own);
  while (present) {
    const int a = __ffsll((unsigned long long)present) - 1;
    present &= present - 1;
    const bool has = (own >> a) & 1ull;
    const uint32_t carriers = (uint32_t)__popcll(__ballot(has));
    if (lane == a) boundary += carriers;
    uint64_t others = wave_or(has ? saw : 0ull);
    uint32_t mine = 0;
    while (others) {
      const int b = __ffsll((unsigned long long)others) - 1;
      others &= others - 1;
      const uint32_t c = (uint32_t)__popcll(__ballot(has && ((saw >> b) & 1ull)));
      if (lane == b) mine = c;
    }
    if (mine) atomicAdd(&table[a * stride_a + lane * stride_b], mine);
  }
}

__global__ __launch_bounds__(kBlock) void pair_match_kernel(const ulonglong2* __restrict__ words, int n_gt, int n_pred, int height,
                                                           int width, int radius, uint32_t* __restrict__ singles,
                                                           uint32_t* __restrict__ pairs) {
  constexpr int I = DEVA_PAIR_INNER_RADIUS;
  extern __shared__ int smem[];  // boundary pixels [2][64], gt pixels matched by p [n_gt][n_pred], pred pixels matched by g [n_gt][n_pred]
  const int cells = n_gt * n_pred;
  uint32_t* bins = reinterpret_cast<uint32_t*>(smem);
  uint32_t* hit_g = bins + 2 * N;
  uint32_t* hit_p = hit_g + cells;
  for (int i = threadIdx.x; i < 2 * N + 2 * cells; i += kBlock) bins[i] = 0u;
  __syncthreads();
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t pixels = (int64_t)height * width;
  const int64_t chunks = (pixels + kWave - 1) / kWave;
  const int64_t waves = (int64_t)gridDim.x * (kBlock / kWave);
  const int r2 = radius * radius;
  uint32_t n_g = 0, n_p = 0;  // boundary pixels of ground-truth object `lane` and of proposal `lane`
  for (int64_t chunk = (int64_t)blockIdx.x * (kBlock / kWave) + (threadIdx.x >> 6); chunk < chunks; chunk += waves) {
    const int64_t at = chunk * kWave + lane;
    ulonglong2 mine = {0ull, 0ull};
    if (at < pixels) mine = words[at];
    const bool active = (mine.x | mine.y) != 0ull;
    uint64_t todo = __ballot(active);
    if (todo == 0ull) continue;  // (uniform over the wave)
    uint64_t seen_g = 0, seen_p = 0;
    if (radius <= I) {
      // every boundary pixel's own lane: the box of radius I, clipped by the disk.  The loads are unconditional (the
      // address is clamped into the image, the word masked) so that a row's seven are in flight together.
      if (active) {
        const int py = (int)(at / width), px = (int)(at - (int64_t)py * width);
#pragma unroll
        for (int dy = -I; dy <= I; ++dy) {
          const int y = py + dy;
          const int64_t row = (int64_t)(y < 0 ? 0 : y >= height ? height - 1 : y) * width;
#pragma unroll
          for (int dx = -I; dx <= I; ++dx) {
            if (dx * dx + dy * dy > I * I) continue;  // (compile time: the corners of the box are outside every disk of radius <= I)
            const int x = px + dx;
            const bool in = dx * dx + dy * dy <= r2 && y >= 0 && y < height && x >= 0 && x < width;
            const ulonglong2 w = words[row + (x < 0 ? 0 : x >= width ? width - 1 : x)];
            seen_g |= in ? w.x : 0ull, seen_p |= in ? w.y : 0ull;
          }
        }
      }
    } else {
      // all 64 lanes search one pixel's whole box together
      while (todo) {  // (uniform over the wave)
        const int b = __ffsll((unsigned long long)todo) - 1;
        todo &= todo - 1;
        const int64_t pixel = chunk * kWave + b;
        const int py = (int)(pixel / width), px = (int)(pixel - (int64_t)py * width);
        uint64_t more_g = 0, more_p = 0;
        search_box(words, height, width, py, px, radius, r2, lane, more_g, more_p);
        more_g = wave_or(more_g), more_p = wave_or(more_p);
        if (lane == b) seen_g = more_g, seen_p = more_p;
      }
    }
    count_side(mine.x, seen_p, lane, n_g, hit_g, n_pred, 1);
    count_side(mine.y, seen_g, lane, n_p, hit_p, 1, n_pred);
  }
  // the four waves' counters meet in LDS; one integer atomic per non-zero cell of the workgroup
  if (n_g) atomicAdd(&bins[lane], n_g);
  if (n_p) atomicAdd(&bins[N + lane], n_p);
  __syncthreads();
  for (int i = threadIdx.x; i < 2 * N; i += kBlock) {
    const uint32_t v = bins[i];
    const int slot = i & (N - 1);
    const bool pred_side = i >= N;
    if (v && slot < (pred_side ? n_pred : n_gt)) atomicAdd(&singles[((pred_side ? n_gt : 0) + slot) * DEVA_PAIR_SINGLE_FIELDS + 1], v);
  }
  for (int i = threadIdx.x; i < cells; i += kBlock) {
    const uint32_t v = hit_g[i], u = hit_p[i];
    if (v) atomicAdd(&pairs[i * DEVA_PAIR_FIELDS + 1], v);
    if (u) atomicAdd(&pairs[i * DEVA_PAIR_FIELDS + 2], u);
  }
}

template <int GT, int PR>
void launch_label(const struct deva_pair_plan& plan, const void* gt, const int* gt_ids, int n_gt, const void* pred, const int* pred_ids,
                  int n_pred, const uint16_t* lut, int channels, int height, int width, ulonglong2* words, uint32_t* singles,
                  uint32_t* pairs, hipStream_t stream) {
  hipLaunchKernelGGL((pair_label_kernel<GT, PR>), dim3(plan.label_grid), dim3(plan.block), plan.label_lds_bytes, stream, gt, gt_ids,
                     n_gt, pred, pred_ids, n_pred, lut, channels, height, width, words, singles, pairs);
}

template <int GT>
void launch_label_pred(int pred_encoding, const struct deva_pair_plan& plan, const void* gt, const int* gt_ids, int n_gt, const void* pred,
                       const int* pred_ids, int n_pred, const uint16_t* lut, int channels, int height, int width, ulonglong2* words,
                       uint32_t* singles, uint32_t* pairs, hipStream_t stream) {
  switch (pred_encoding) {
    case DEVA_PAIR_U8:
      return launch_label<GT, DEVA_PAIR_U8>(plan, gt, gt_ids, n_gt, pred, pred_ids, n_pred, lut, channels, height, width, words, singles,
                                            pairs, stream);
    case DEVA_PAIR_I32:
      return launch_label<GT, DEVA_PAIR_I32>(plan, gt, gt_ids, n_gt, pred, pred_ids, n_pred, lut, channels, height, width, words, singles,
                                             pairs, stream);
    case DEVA_PAIR_I64:
      return launch_label<GT, DEVA_PAIR_I64>(plan, gt, gt_ids, n_gt, pred, pred_ids, n_pred, lut, channels, height, width, words, singles,
                                             pairs, stream);
    default:
      return launch_label<GT, DEVA_PAIR_INDEX16>(plan, gt, gt_ids, n_gt, pred, pred_ids, n_pred, lut, channels, height, width, words,
                                                 singles, pairs, stream);
  }
}

}  // namespace
}  // namespace deva_pair

extern "C" int deva_pair_counts(const void* gt, int gt_encoding, const int32_t* gt_ids, int n_gt, const void* pred, int pred_encoding,
                                const int32_t* pred_ids, int n_pred, const uint16_t* pred_lut, int channels, int height, int width,
                                int radius, void* scratch, int64_t scratch_bytes, uint32_t* singles, uint32_t* pairs, void* stream) {
  using namespace deva_pair;
  struct deva_pair_plan plan;
  if (int rc = pair_counts_check(gt, gt_encoding, gt_ids, n_gt, pred, pred_encoding, pred_ids, n_pred, pred_lut, channels, height, width,
                                 radius, scratch, scratch_bytes, singles, pairs, &plan))
    return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipError_t e = hipMemsetAsync(singles, 0, sizeof(uint32_t) * DEVA_PAIR_SINGLE_FIELDS * (size_t)(n_gt + n_pred), st);
  if (e == hipSuccess) e = hipMemsetAsync(pairs, 0, sizeof(uint32_t) * DEVA_PAIR_FIELDS * (size_t)n_gt * (size_t)n_pred, st);
  if (e != hipSuccess) {
    set_error("deva_pair_counts: clearing the records: %s", hipGetErrorString(e));
    return 1;
  }
  ulonglong2* words = static_cast<ulonglong2*>(scratch);
  if (gt_encoding == DEVA_PAIR_U8)
    launch_label_pred<DEVA_PAIR_U8>(pred_encoding, plan, gt, gt_ids, n_gt, pred, pred_ids, n_pred, pred_lut, channels, height, width, words,
                                    singles, pairs, st);
  else
    launch_label_pred<DEVA_PAIR_I32>(pred_encoding, plan, gt, gt_ids, n_gt, pred, pred_ids, n_pred, pred_lut, channels, height, width, words,
                                     singles, pairs, st);
  hipLaunchKernelGGL(pair_match_kernel, dim3(plan.match_grid), dim3(plan.block), plan.match_lds_bytes, st, words, n_gt, n_pred, height, width,
                     plan.radius, singles, pairs);
  e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("deva_pair_counts: launch failed: %s", hipGetErrorString(e));
    return 1;
  }
  return 0;
}
