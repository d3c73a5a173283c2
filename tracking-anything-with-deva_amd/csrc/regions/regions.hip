// deva_regions_label and deva_regions_clean (include/deva_regions.h, rules R1-R7): 8-connected components of byte planes by
// union-find on int32 labels, and the small-hole / small-island clean-up on top of them.
//
// A label is 0 for a pixel of the other kind, else 1 + the position of a pixel of the same component (region_union.h);
// union by the smaller position makes a component's root its first pixel in row-major order, which is the output format
// of deva_regions_label and the tie rule of R3 at once.
//
//   local    one workgroup per tile of 32 x 32 pixels, four pixels a lane.  The tile is labelled in 4 KB of LDS (a pixel
//            unites with W and with N, or with NW and NE where N is of the other kind) and written out with the root's
//            position in the plane; the tile's area slots are cleared on the way.
//   border   one lane per pixel right of a vertical tile edge (unites with the three pixels left of it) and per pixel
//            below a horizontal one (with the three above it): every 8-adjacent pair that two tiles share, the
//            diagonal pairs at tile corners included.  Union-find on global memory, device-scope atomics.
//   flatten  one lane per pixel: the pixel points at its root, and the wave adds its pixels to the root's area slot, one
//            integer atomic per component present among the wave's 64 pixels.
//   decide   one lane per pixel, only roots act: is any component small, is any not, and the largest (area, then the
//            earlier first pixel) as one 64-bit maximum; through LDS, one atomic per workgroup and word.
//   rewrite  one lane per pixel: R2 fills, R3 removes and writes every byte as 0 / 1; R3 also reduces the area and the
//            box over the wave (shuffles), the workgroup (LDS) and the plane (one atomic per workgroup and word).
//
// No kernel waits on another workgroup; a stage that needs the plane finished is a launch of its own.  Every kernel
// walks its work in a grid-stride loop, so the grids of the plan may be capped.
#include <hip/hip_runtime.h>
#include <limits.h>

#include "../launch_check.h"
#include "region_plan.h"
#include "region_union.h"

namespace deva_regions {
namespace {

constexpr int T = kTile;
static_assert(T == 32 && kBlock == 256, "a lane of the local stage takes the pixels tid, tid + 256, ... of a 32 x 32 tile");

struct Lds {   // workgroup scope: the tile's labels
  static __device__ __forceinline__ int load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
  static __device__ __forceinline__ int fetch_min(int* p, int v) {
    return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
};
struct Global {   // device scope: the plane's labels
  static __device__ __forceinline__ int load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  static __device__ __forceinline__ int fetch_min(int* p, int v) {
    return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
};

// the decision words of a plane in flight (kStateWords ints, cleared by init)
struct State {
  uint32_t flags[2];        // per pass (0: R2, 1: R3): bit 0 a small component exists, bit 1 one that is not small
  unsigned long long best;  // R3: max over components of area << 32 | (INT_MAX - first pixel)
  int filled, removed, area;
  int x0, y0, x1, y1;
  int pad[5];
};
static_assert(sizeof(State) == 4 * kStateWords, "the plan reserves kStateWords ints");

// the planes of a pass: plane k's bytes at planes + k * pixels, its labels at labels + k * stride (ints), its areas and
// state likewise (null for deva_regions_label)
struct Pass {
  uint8_t* planes;
  int* labels;
  int* areas;
  State* state;
  int64_t stride, state_stride;   // in ints / in States
  int count, height, width;
};

__global__ __launch_bounds__(kBlock) void regions_init_kernel(Pass ps) {
  for (int k = blockIdx.x * kBlock + threadIdx.x; k < ps.count; k += gridDim.x * kBlock) {
    State s = {};
    s.x0 = s.y0 = INT_MAX;
    s.x1 = s.y1 = -1;
    ps.state[k * ps.state_stride] = s;
  }
}

__global__ __launch_bounds__(kBlock) void regions_local_kernel(Pass ps, int of_zeros, int tiles_x, int tiles_y) {
  __shared__ int lab[T * T];
  const int tid = threadIdx.x, per_plane = tiles_x * tiles_y;
  const int64_t tiles = (int64_t)ps.count * per_plane, pixels = (int64_t)ps.height * ps.width;
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int k = (int)(t / per_plane), in_plane = (int)(t - (int64_t)k * per_plane);
    const int y0 = in_plane / tiles_x * T, x0 = in_plane % tiles_x * T;
    const uint8_t* src = ps.planes + k * pixels;
#pragma unroll
    for (int i = tid; i < T * T; i += kBlock) {
      const int y = y0 + i / T, x = x0 + i % T;
      const bool in = y < ps.height && x < ps.width;
      lab[i] = in && ((src[(int64_t)y * ps.width + x] != 0) != (of_zeros != 0)) ? i + 1 : 0;
    }
    __syncthreads();
#pragma unroll
    for (int i = tid; i < T * T; i += kBlock) {
      const int ly = i / T, lx = i % T;
      if (lab[i] == 0) continue;   // (a label never becomes or ceases to be 0)
      if (lx > 0 && lab[i - 1]) unite<Lds>(lab, i, i - 1);
      if (ly > 0) {
        if (lab[i - T]) {
          unite<Lds>(lab, i, i - T);   // NW and NE hang on N through their own W unions
        } else {
          if (lx > 0 && lab[i - T - 1]) unite<Lds>(lab, i, i - T - 1);
          if (lx < T - 1 && lab[i - T + 1]) unite<Lds>(lab, i, i - T + 1);
        }
      }
    }
    __syncthreads();
#pragma unroll
    for (int i = tid; i < T * T; i += kBlock) {
      const int y = y0 + i / T, x = x0 + i % T;
      if (y < ps.height && x < ps.width) {
        int out = 0;
        if (lab[i]) {
          const int r = find_root<Lds>(lab, i);   // the tile's order is the plane's: the smallest position in either
          out = (y0 + r / T) * ps.width + x0 + r % T + 1;
        }
        const int64_t at = (int64_t)y * ps.width + x;
        ps.labels[k * ps.stride + at] = out;
        if (ps.areas) ps.areas[k * ps.stride + at] = 0;
      }
    }
    __syncthreads();   // the next tile reuses lab
  }
}

__global__ __launch_bounds__(kBlock) void regions_border_kernel(Pass ps, int tiles_x, int tiles_y) {
  const int h = ps.height, w = ps.width;
  const int64_t vertical = (int64_t)(tiles_x - 1) * h, per_plane = vertical + (int64_t)(tiles_y - 1) * w;
  const int64_t items = ps.count * per_plane;
  for (int64_t it = (int64_t)blockIdx.x * kBlock + threadIdx.x; it < items; it += (int64_t)gridDim.x * kBlock) {
    const int k = (int)(it / per_plane);
    int64_t r = it - k * per_plane;
    int* L = ps.labels + k * ps.stride;
    if (r < vertical) {   // the pixel right of a vertical edge, and the three left of it
      const int edge = (int)(r / h), y = (int)(r - (int64_t)edge * h), x = (edge + 1) * T;
      const int p = y * w + x;
      if (L[p] == 0) continue;
      for (int yy = y - 1; yy <= y + 1; ++yy)
        if (yy >= 0 && yy < h && L[yy * w + x - 1]) unite<Global>(L, p, yy * w + x - 1);
    } else {              // the pixel below a horizontal edge, and the three above it
      r -= vertical;
      const int edge = (int)(r / w), x = (int)(r - (int64_t)edge * w), y = (edge + 1) * T;
      const int p = y * w + x;
      if (L[p] == 0) continue;
      for (int xx = x - 1; xx <= x + 1; ++xx)
        if (xx >= 0 && xx < w && L[(y - 1) * w + xx]) unite<Global>(L, p, (y - 1) * w + xx);
    }
  }
}

// the chunk of kBlock consecutive pixels of one plane a workgroup takes next: -> plane and the lane's pixel (or -1)
__device__ __forceinline__ void chunk_pixel(int64_t chunk, int64_t chunks_per_plane, int pixels, int& k, int& p) {
  k = (int)(chunk / chunks_per_plane);
  const int64_t at = (chunk - k * chunks_per_plane) * kBlock + threadIdx.x;
  p = at < pixels ? (int)at : -1;
}

template <bool COUNT>
__global__ __launch_bounds__(kBlock) void regions_flatten_kernel(Pass ps) {
  const int pixels = ps.height * ps.width, lane = threadIdx.x & (kWave - 1);
  const int64_t chunks_per_plane = ((int64_t)pixels + kBlock - 1) / kBlock, chunks = ps.count * chunks_per_plane;
  for (int64_t c = blockIdx.x; c < chunks; c += gridDim.x) {   // (uniform over the workgroup)
    int k, p;
    chunk_pixel(c, chunks_per_plane, pixels, k, p);
    int* L = ps.labels + k * ps.stride;
    int root = -1;
    if (p >= 0 && Global::load(L + p) != 0) {
      root = find_root<Global>(L, p);   // (roots are final: the merging launches are over)
      __hip_atomic_store(L + p, root + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if constexpr (COUNT) {
      uint64_t todo = __ballot(root >= 0);
      while (todo) {   // (uniform over the wave) one atomic per component among the wave's pixels
        const int leader = __ffsll((unsigned long long)todo) - 1;
        const int r = __shfl(root, leader);
        const uint64_t same = __ballot(root == r);
        if (lane == leader) atomicAdd(ps.areas + k * ps.stride + r, (int)__popcll(same));
        todo &= ~same;
      }
    }
  }
}

__global__ __launch_bounds__(kBlock) void regions_decide_kernel(Pass ps, int pass, int min_area) {
  __shared__ uint32_t s_flags;
  __shared__ unsigned long long s_best;
  const int pixels = ps.height * ps.width;
  const int64_t chunks_per_plane = ((int64_t)pixels + kBlock - 1) / kBlock, chunks = ps.count * chunks_per_plane;
  for (int64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
    int k, p;
    chunk_pixel(c, chunks_per_plane, pixels, k, p);
    if (threadIdx.x == 0) s_flags = 0u, s_best = 0ull;
    __syncthreads();
    if (p >= 0 && ps.labels[k * ps.stride + p] == p + 1) {   // a root: the component's first pixel, its area in its slot
      const int area = ps.areas[k * ps.stride + p];
      atomicOr(&s_flags, area < min_area ? 1u : 2u);
      if (pass == 1) atomicMax(&s_best, ((unsigned long long)(uint32_t)area << 32) | (uint32_t)(INT_MAX - p));
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      State* st = ps.state + k * ps.state_stride;
      if (s_flags) atomicOr(&st->flags[pass], s_flags);
      if (s_best) atomicMax(&st->best, s_best);
    }
    __syncthreads();
  }
}

__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
  for (int d = kWave / 2; d; d >>= 1) v = min(v, __shfl_xor(v, d));
  return v;
}
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
  for (int d = kWave / 2; d; d >>= 1) v = max(v, __shfl_xor(v, d));
  return v;
}

__global__ __launch_bounds__(kBlock) void regions_rewrite_kernel(Pass ps, int pass, int min_area) {
  __shared__ int s_count[2], s_box[4];   // changed pixels, mask pixels; x0, y0, x1, y1
  const int pixels = ps.height * ps.width, lane = threadIdx.x & (kWave - 1);
  const int64_t chunks_per_plane = ((int64_t)pixels + kBlock - 1) / kBlock, chunks = ps.count * chunks_per_plane;
  for (int64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
    int k, p;
    chunk_pixel(c, chunks_per_plane, pixels, k, p);
    State* st = ps.state + k * ps.state_stride;
    if (threadIdx.x == 0) s_count[0] = s_count[1] = 0, s_box[0] = s_box[1] = INT_MAX, s_box[2] = s_box[3] = -1;
    __syncthreads();
    const uint32_t flags = st->flags[pass];   // (written by the launch before this one)
    const bool any_small = flags & 1u, any_big = flags & 2u;
    const int keep = INT_MAX - (int)(uint32_t)st->best;
    uint8_t* plane = ps.planes + (int64_t)k * pixels;
    bool mask = false, acted = false;
    if (p >= 0) {
      mask = plane[p] != 0;
      const int label = ps.labels[k * ps.stride + p];   // 0 for the kind this pass does not label
      if (label && any_small) {
        const bool small = ps.areas[k * ps.stride + label - 1] < min_area;
        acted = pass == 0 ? small : any_big ? small : label - 1 != keep;
      }
      if (acted) mask = pass == 0;
      if (pass == 1 || acted) plane[p] = mask ? 1 : 0;
    }
    const uint64_t acted_lanes = __ballot(acted), mask_lanes = __ballot(mask);
    if (lane == 0 && acted_lanes) atomicAdd(&s_count[0], (int)__popcll(acted_lanes));
    if (pass == 1 && mask_lanes) {   // (uniform over the wave)
      const int y = mask ? p / ps.width : 0, x = mask ? p - y * ps.width : 0;
      const int x0 = wave_min(mask ? x : INT_MAX), y0 = wave_min(mask ? y : INT_MAX);
      const int x1 = wave_max(mask ? x : -1), y1 = wave_max(mask ? y : -1);
      if (lane == 0) {
        atomicAdd(&s_count[1], (int)__popcll(mask_lanes));
        atomicMin(&s_box[0], x0), atomicMin(&s_box[1], y0), atomicMax(&s_box[2], x1), atomicMax(&s_box[3], y1);
      }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      if (s_count[0]) atomicAdd(pass == 0 ? &st->filled : &st->removed, s_count[0]);
      if (s_count[1]) {
        atomicAdd(&st->area, s_count[1]);
        atomicMin(&st->x0, s_box[0]), atomicMin(&st->y0, s_box[1]), atomicMax(&st->x1, s_box[2]), atomicMax(&st->y1, s_box[3]);
      }
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(kBlock) void regions_record_kernel(Pass ps, int* records) {
  for (int k = blockIdx.x * kBlock + threadIdx.x; k < ps.count; k += gridDim.x * kBlock) {
    const State s = ps.state[k * ps.state_stride];
    int* r = records + k * DEVA_REGIONS_FIELDS;
    const bool empty = s.area == 0;
    r[0] = (s.flags[0] | s.flags[1]) & 1u ? 1 : 0;
    r[1] = s.filled, r[2] = s.removed, r[3] = s.area;
    r[4] = empty ? 0 : s.x0, r[5] = empty ? 0 : s.y0, r[6] = empty ? 0 : s.x1, r[7] = empty ? 0 : s.y1;
  }
}

// the three stages of one labelling of a pass
template <bool COUNT>
void launch_labelling(const struct deva_regions_plan& plan, const Pass& ps, int of_zeros, uint32_t local_grid, uint32_t border_grid,
                      uint32_t pixel_grid, hipStream_t st) {
  hipLaunchKernelGGL(regions_local_kernel, dim3(local_grid), dim3(kBlock), 0, st, ps, of_zeros, plan.tiles_x, plan.tiles_y);
  if (border_grid) hipLaunchKernelGGL(regions_border_kernel, dim3(border_grid), dim3(kBlock), 0, st, ps, plan.tiles_x, plan.tiles_y);
  hipLaunchKernelGGL(regions_flatten_kernel<COUNT>, dim3(pixel_grid), dim3(kBlock), 0, st, ps);
}

LAUNCH_CHECK_DEFINE_LAUNCHED()

}  // namespace
}  // namespace deva_regions

extern "C" int deva_regions_label(const uint8_t* planes, int n, int height, int width, int of_zeros, int32_t* labels, void* scratch,
                                  int64_t scratch_bytes, void* stream) {
  using namespace deva_regions;
  (void)scratch, (void)scratch_bytes;   // `labels` is the union-find array
  struct deva_regions_plan plan;
  if (int rc = label_check(planes, n, height, width, labels, &plan)) return rc;
  if (n == 0) return 0;
  const int64_t pixels = (int64_t)height * width;
  const Pass ps = {const_cast<uint8_t*>(planes), labels, nullptr, nullptr, pixels, 0, n, height, width};
  launch_labelling<false>(plan, ps, of_zeros, plan.local_grid, plan.border_grid, plan.pixel_grid, static_cast<hipStream_t>(stream));
  return launched("deva_regions_label");
}

extern "C" int deva_regions_clean(uint8_t* planes, int n, int height, int width, int min_area, int32_t* records, void* scratch,
                                  int64_t scratch_bytes, void* stream) {
  using namespace deva_regions;
  struct deva_regions_plan plan;
  if (int rc = clean_check(planes, n, height, width, min_area, records, scratch, scratch_bytes, &plan)) return rc;
  if (n == 0) return 0;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int64_t pixels = (int64_t)height * width;
  const PlaneLayout lay = plane_layout(pixels);
  char* base = static_cast<char*>(scratch);
  for (int first = 0; first < n; first += plan.planes_per_pass) {   // the same scratch again: the stream orders the passes
    const int count = n - first < plan.planes_per_pass ? n - first : plan.planes_per_pass;
    struct deva_regions_plan part;   // the grids of this pass (the last one may be shorter)
    if (int rc = region_plan("deva_regions_clean", height, width, count, -1, &part)) return rc;
    const Pass ps = {planes + first * pixels,
                     reinterpret_cast<int*>(base + lay.labels),
                     reinterpret_cast<int*>(base + lay.areas),
                     reinterpret_cast<State*>(base + lay.state),
                     plan.plane_bytes / 4,
                     plan.plane_bytes / (int64_t)sizeof(State),
                     count,
                     height,
                     width};
    const uint32_t small_grid = (uint32_t)((count + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(regions_init_kernel, dim3(small_grid), dim3(kBlock), 0, st, ps);
    for (int pass = 0; pass < 2; ++pass) {   // R2 on the complement, then R3 on the mask that R2 left
      launch_labelling<true>(part, ps, pass == 0 ? 1 : 0, part.local_grid, part.border_grid, part.pixel_grid, st);
      hipLaunchKernelGGL(regions_decide_kernel, dim3(part.pixel_grid), dim3(kBlock), 0, st, ps, pass, min_area);
      hipLaunchKernelGGL(regions_rewrite_kernel, dim3(part.pixel_grid), dim3(kBlock), 0, st, ps, pass, min_area);
    }
    hipLaunchKernelGGL(regions_record_kernel, dim3(small_grid), dim3(kBlock), 0, st, ps, records + (int64_t)first * DEVA_REGIONS_FIELDS);
    if (int rc = launched("deva_regions_clean")) return rc;
  }
  return 0;
}
