// deva_vos_boundary_counts (include/deva_vos_metrics.h, rules R1-R5): the seven counts per object from which region
// similarity J and boundary accuracy F of a frame follow, for up to 64 objects at once: one bit per object in a 64-bit
// word per pixel.
//
// label_kernel: a lane takes a strip of 8 pixels of one row and reads that row and the next, 9 values each, once.  The slot
// of a value (R1) comes from the id table in LDS by binary search, or from pred_lut, and only when the value differs from
// the lane's previous one.  The boundary word of a side at a pixel (R2) has the bit of the pixel's own object and of the
// neighbour's object for every E / S / SE neighbour that exists and holds another slot.  The two words go to the scratch
// side by side, one 16-byte store per pixel.  Fields 0 - 2 are added as runs to a per-workgroup table in LDS whose
// non-zero entries are flushed with one integer atomic each.
//
// match_kernel: a wave takes 64 consecutive pixels, a lane each, one 16-byte load.  A lane whose words are not both zero
// first searches the box of radius 3 (clipped by the disk of R4) by itself, or-ing the other side's words: 64 boundary
// pixels of a horizontal edge go in parallel, and a prediction near its ground truth is matched there.  For every pixel
// with a bit still unmatched the 64 lanes then walk larger boxes together -- radius 8, then the whole radius; four cells each
// per step, the cell's row and column by a multiply-high, in or out of the disk by dx^2 + dy^2 <= r^2 -- and reduce
// across the wave.  Lane i keeps fields 3 - 6 of object i in registers, fed by one ballot per field for every object
// present among the 64 pixels; the four waves' counters meet in 1 KB of LDS at the end.  No atomic inside the loop, and the
// radius bounds nothing but a trip count.
// Integer adds everywhere: exact, and independent of the order.
#include <hip/hip_runtime.h>
#include <limits.h>

#include "../plane_values.h"
#include "boundary_plan.h"

namespace deva_vos {
namespace {

constexpr int S = DEVA_VOS_STRIP;
static_assert(kBlock == kWave * 4, "match_kernel keeps 4 fields of 64 objects, one per lane of the workgroup");

using plane_values::bit_of;
using plane_values::load_value;
static_assert(DEVA_VOS_U8 == plane_values::kU8 && DEVA_VOS_I32 == plane_values::kI32 && DEVA_VOS_I64 == plane_values::kI64 &&
                  DEVA_VOS_INDEX16 == plane_values::kIndex16,
              "the encodings of plane_values.h");

// R1: the slot of a value, -1 for none
template <int ENC>
__device__ __forceinline__ int find_slot(int value, bool binary, const int* table, int n, const uint16_t* lut, int channels) {
  if (binary) return value != 0 ? 0 : -1;
  return plane_values::find_slot<ENC>(value, table, n, lut, channels);
}

// R2 for one pixel: own slot a against the slots of the E / S / SE neighbours that exist
__device__ __forceinline__ uint64_t boundary_word(int a, int e, int s, int se, bool has_e, bool has_s) {
  uint64_t w = 0;
  if (has_e && e != a) w |= bit_of(a) | bit_of(e);
  if (has_s && s != a) w |= bit_of(a) | bit_of(s);
  if (has_e && has_s && se != a) w |= bit_of(a) | bit_of(se);
  return w;
}

template <int GT, int PR>
__global__ __launch_bounds__(kBlock) void label_kernel(const void* __restrict__ gt, bool gt_binary, const void* __restrict__ pred,
                                                      bool pred_binary, const int* __restrict__ ids, int n,
                                                      const uint16_t* __restrict__ lut, int channels, int height, int width,
                                                      ulonglong2* __restrict__ words, uint32_t* __restrict__ counts) {
  extern __shared__ int smem[];  // the id table [n], then the workgroup's fields 0 - 2 [n][3]
  int* table = smem;
  uint32_t* bins = reinterpret_cast<uint32_t*>(smem + n);
  const int tid = threadIdx.x;
  for (int i = tid; i < n; i += kBlock) table[i] = ids[i];
  for (int i = tid; i < 3 * n; i += kBlock) bins[i] = 0u;
  __syncthreads();

  int last_g = 0, slot_g = gt_binary ? -1 : find_slot<GT>(0, false, table, n, lut, channels);
  int last_p = 0, slot_p = pred_binary ? -1 : find_slot<PR>(0, false, table, n, lut, channels);
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
          if (vg != last_g) last_g = vg, slot_g = find_slot<GT>(vg, gt_binary, table, n, lut, channels);
          const int vp = load_value<PR>(pred, at);
          if (vp != last_p) last_p = vp, slot_p = find_slot<PR>(vp, pred_binary, table, n, lut, channels);
          g[r][k] = slot_g, p[r][k] = slot_p;
        }
      }
    }
    int run_g = -1, run_p = -1;
    uint32_t run = 0;
    auto flush = [&]() {
      if (run_g >= 0) atomicAdd(&bins[3 * run_g + 1], run);
      if (run_p >= 0) atomicAdd(&bins[3 * run_p + 2], run);
      if (run_g >= 0 && run_g == run_p) atomicAdd(&bins[3 * run_g], run);
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
  for (int i = tid; i < 3 * n; i += kBlock) {
    const uint32_t v = bins[i];
    if (v) atomicAdd(&counts[(i / 3) * DEVA_VOS_FIELDS + i % 3], v);
  }
}

// or over the 64 lanes, the same value in every lane: four rotations inside each row of 16 lanes (data-parallel
// primitives: no LDS traffic, unlike a chain of six shuffles), then the four rows through scalar registers
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
__device__ __forceinline__ void search_box(const ulonglong2* __restrict__ words, int height, int width, int py, int px, int box,
                                           int r2, int lane, uint64_t& seen_g, uint64_t& seen_p) {
  const uint32_t side = 2u * (uint32_t)box + 1u;
  const uint32_t cells = side * side;
  const uint32_t magic = (uint32_t)(0x100000000ull / side) + 1u;
  constexpr int U = 4;  // cells of a lane in flight together: the loads are unconditional (clamped into the image), the words masked
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

__device__ __forceinline__ uint64_t from_lane(uint64_t v, int src) {
  return ((uint64_t)(uint32_t)__shfl((int)(v >> 32), src, kWave) << 32) | (uint32_t)__shfl((int)(uint32_t)v, src, kWave);
}

__global__ __launch_bounds__(kBlock) void match_kernel(const ulonglong2* __restrict__ words, int n, int height, int width, int radius,
                                                      uint32_t* __restrict__ counts) {
  constexpr int I = DEVA_VOS_INNER_RADIUS;
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t pixels = (int64_t)height * width;
  const int64_t chunks = (pixels + kWave - 1) / kWave;
  const int64_t waves = (int64_t)gridDim.x * (kBlock / kWave);
  const int r2 = radius * radius;
  const int middle = radius < DEVA_VOS_MIDDLE_RADIUS ? radius : DEVA_VOS_MIDDLE_RADIUS;
  __shared__ uint32_t shared[kWave * 4];  // the workgroup's fields 3 - 6
  shared[threadIdx.x] = 0u;
  __syncthreads();
  uint32_t n_g = 0, n_p = 0, hit_g = 0, hit_p = 0;  // fields 3 - 6 of object `lane`
  for (int64_t chunk = (int64_t)blockIdx.x * (kBlock / kWave) + (threadIdx.x >> 6); chunk < chunks; chunk += waves) {
    const int64_t at = chunk * kWave + lane;
    ulonglong2 mine = {0ull, 0ull};
    if (at < pixels) mine = words[at];
    const bool active = (mine.x | mine.y) != 0ull;
    if (__ballot(active) == 0ull) continue;  // (uniform over the wave)
    // every boundary pixel's own lane: the box of radius I, clipped by the disk.  The loads are unconditional (the
    // address is clamped into the image, the word masked) so that a row's seven are in flight together.
    uint64_t seen_g = 0, seen_p = 0;
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
    // what is still unmatched: all 64 lanes search one pixel's larger boxes together
    uint64_t todo = __ballot(radius > I && ((mine.x & ~seen_p) | (mine.y & ~seen_g)) != 0ull);
    while (todo) {  // (uniform over the wave)
      const int b = __ffsll((unsigned long long)todo) - 1;
      todo &= todo - 1;
      const uint64_t miss_g = from_lane(mine.x & ~seen_p, b), miss_p = from_lane(mine.y & ~seen_g, b);
      const int64_t pixel = chunk * kWave + b;
      const int py = (int)(pixel / width), px = (int)(pixel - (int64_t)py * width);
      uint64_t more_g = 0, more_p = 0;
      search_box(words, height, width, py, px, middle, r2, lane, more_g, more_p);
      more_g = wave_or(more_g), more_p = wave_or(more_p);
      if (middle < radius && (((miss_g & ~more_p) | (miss_p & ~more_g)) != 0ull)) {
        search_box(words, height, width, py, px, radius, r2, lane, more_g, more_p);
        more_g = wave_or(more_g), more_p = wave_or(more_p);
      }
      if (lane == b) seen_g |= more_g, seen_p |= more_p;
    }
    // lane i counts object i: one ballot per field for every object that has a boundary pixel among the 64
    const uint64_t hit_words_g = mine.x & seen_p, hit_words_p = mine.y & seen_g;
    uint64_t present = wave_or(mine.x | mine.y);
    while (present) {  // (uniform over the wave)
      const int i = __ffsll((unsigned long long)present) - 1;
      present &= present - 1;
      const uint32_t c3 = (uint32_t)__popcll(__ballot((mine.x >> i) & 1ull)), c4 = (uint32_t)__popcll(__ballot((mine.y >> i) & 1ull));
      const uint32_t c5 = (uint32_t)__popcll(__ballot((hit_words_g >> i) & 1ull)), c6 = (uint32_t)__popcll(__ballot((hit_words_p >> i) & 1ull));
      if (lane == i) n_g += c3, n_p += c4, hit_g += c5, hit_p += c6;
    }
  }
  // the four waves' counters meet in LDS; one integer atomic per non-zero field of the workgroup
  if (n_g) atomicAdd(&shared[4 * lane], n_g);
  if (n_p) atomicAdd(&shared[4 * lane + 1], n_p);
  if (hit_g) atomicAdd(&shared[4 * lane + 2], hit_g);
  if (hit_p) atomicAdd(&shared[4 * lane + 3], hit_p);
  __syncthreads();
  const uint32_t v = shared[threadIdx.x];
  const int object = (int)threadIdx.x >> 2;
  if (v && object < n) atomicAdd(&counts[object * DEVA_VOS_FIELDS + 3 + (threadIdx.x & 3)], v);
}

template <int GT, int PR>
void launch_label(const deva_vos_plan& plan, const void* gt, bool gt_binary, const void* pred, bool pred_binary, const int* ids, int n,
                  const uint16_t* lut, int channels, int height, int width, ulonglong2* words, uint32_t* counts, hipStream_t stream) {
  hipLaunchKernelGGL((label_kernel<GT, PR>), dim3(plan.label_grid), dim3(plan.block), plan.lds_bytes, stream, gt, gt_binary, pred,
                     pred_binary, ids, n, lut, channels, height, width, words, counts);
}

template <int GT>
void launch_label_pred(int pred_plain, const deva_vos_plan& plan, const void* gt, bool gt_binary, const void* pred, bool pred_binary,
                       const int* ids, int n, const uint16_t* lut, int channels, int height, int width, ulonglong2* words,
                       uint32_t* counts, hipStream_t stream) {
  switch (pred_plain) {
    case DEVA_VOS_U8:
      return launch_label<GT, DEVA_VOS_U8>(plan, gt, gt_binary, pred, pred_binary, ids, n, lut, channels, height, width, words, counts,
                                           stream);
    case DEVA_VOS_I32:
      return launch_label<GT, DEVA_VOS_I32>(plan, gt, gt_binary, pred, pred_binary, ids, n, lut, channels, height, width, words, counts,
                                            stream);
    case DEVA_VOS_I64:
      return launch_label<GT, DEVA_VOS_I64>(plan, gt, gt_binary, pred, pred_binary, ids, n, lut, channels, height, width, words, counts,
                                            stream);
    default:
      return launch_label<GT, DEVA_VOS_INDEX16>(plan, gt, gt_binary, pred, pred_binary, ids, n, lut, channels, height, width, words,
                                                counts, stream);
  }
}

}  // namespace
}  // namespace deva_vos

extern "C" int deva_vos_boundary_counts(const void* gt, int gt_encoding, const void* pred, int pred_encoding, const int32_t* ids,
                                        int n_objects, const uint16_t* pred_lut, int channels, int height, int width, int radius,
                                        void* scratch, int64_t scratch_bytes, uint32_t* counts, void* stream) {
  using namespace deva_vos;
  deva_vos_plan plan;
  if (int rc = boundary_counts_check(gt, gt_encoding, pred, pred_encoding, ids, n_objects, pred_lut, channels, height, width, radius,
                                     scratch, scratch_bytes, counts, &plan))
    return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipError_t e = hipMemsetAsync(counts, 0, sizeof(uint32_t) * DEVA_VOS_FIELDS * (size_t)n_objects, st);
  if (e != hipSuccess) {
    set_error("deva_vos_boundary_counts: clearing the records: %s", hipGetErrorString(e));
    return 1;
  }
  const bool gt_binary = (gt_encoding & DEVA_VOS_BINARY) != 0, pred_binary = (pred_encoding & DEVA_VOS_BINARY) != 0;
  const int pred_plain = pred_encoding & ~DEVA_VOS_BINARY;
  ulonglong2* words = static_cast<ulonglong2*>(scratch);
  if ((gt_encoding & ~DEVA_VOS_BINARY) == DEVA_VOS_U8)
    launch_label_pred<DEVA_VOS_U8>(pred_plain, plan, gt, gt_binary, pred, pred_binary, ids, n_objects, pred_lut, channels, height, width,
                                   words, counts, st);
  else
    launch_label_pred<DEVA_VOS_I32>(pred_plain, plan, gt, gt_binary, pred, pred_binary, ids, n_objects, pred_lut, channels, height, width,
                                    words, counts, st);
  hipLaunchKernelGGL(match_kernel, dim3(plan.match_grid), dim3(plan.block), 0, st, words, n_objects, height, width, plan.radius,
                     counts);
  e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("deva_vos_boundary_counts: launch failed: %s", hipGetErrorString(e));
    return 1;
  }
  return 0;
}
