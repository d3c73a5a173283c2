// deva_runs_count and deva_runs_write (include/deva_mask_runs.h, rules E1-E7): mask planes [N][H][W] -> COCO run
// boundaries, on the device.
//
// A mask's column-major scan (E2) is cut into segments of 64 rows: segment x * tiles_y + ty holds the rows of tile row
// ty in column x, so segments ascend with the position p, and a segment's boundaries are one 64-bit word.
//
//   count  a workgroup owns a 64 x 64 tile of one mask (a grid-stride loop over mask x tile).
//          load   a work item is 16 bytes of a tile row, counted from the 16-byte boundary at or below the row's first
//                 pixel: a piece that lies wholly inside the tile's columns is one 16-byte load (aligned by
//                 construction, E7), the pieces at the ragged ends go element by element.  Its pixels, thresholded
//                 (E1), are OR-ed as bits into the row's 64-bit word in LDS.  Word 0 is the row above the tile: the
//                 tile above's last row, or for the top tile row the plane's last row one column to the left, which
//                 is the pixel before a column's first one in scan order (E2: 0 before p = 0).
//          words  lane = row: row ^ row above holds the boundary bits of the row's 64 columns; one ballot per column
//                 turns them into the column's word, which goes to the scratch with its popcount.
//          stats  off the row words of wave 0: popcounts, and the first and last set row and column (E4).
//   scan   runs_scan_kernel: one workgroup per mask, the popcounts to exclusive offsets in place, kScanItems per lane and
//          step; runs_base_kernel: one workgroup, n -> base and total (E5).
//   write  lane = segment for the loads (coalesced words), then lane = row for every word of the wave that has a bit:
//          the rank of a set bit is the popcount of the bits below it, and p leaves under `capacity` (E5).
//
// Every load lies inside [N][H][W], every store inside the scratch, n_out, base, total, stats and bounds[0, capacity).
#include <hip/hip_runtime.h>

#include "../block_scan.h"
#include "../launch_check.h"
#include "mask_runs_plan.h"

namespace deva_runs {
namespace {

static_assert(kTile == 64 && kBlock == 256, "a wave is a segment's 64 rows, a workgroup's 4 waves take 16 columns each");
static_assert(kScanItems * kBlock == DEVA_RUNS_SCAN_CHUNK && DEVA_RUNS_MASK_CHUNK == kBlock, "the scans' steps");
constexpr int kWaves = kBlock / 64;
constexpr int kWaveColumns = kTile / kWaves;

struct CountArgs {
  const void* planes;
  int32_t* off;       // popcounts here, offsets after the scan
  uint32_t* bits;
  int32_t* stats;     // or null
  float threshold;
  int n, height, width, tiles_x, tiles_y, segments;
};

__device__ __forceinline__ bool is_one(uint8_t v, float) { return v != 0; }
__device__ __forceinline__ bool is_one(float v, float threshold) { return v > threshold; }   // (false for NaN)

// the pixel bits of one aligned 16-byte piece
__device__ __forceinline__ uint32_t piece_bits(const uint8_t* p, float) {
  const uint4 v = *reinterpret_cast<const uint4*>(p);
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
  uint32_t m = 0;
#pragma unroll
  for (int e = 0; e < 16; ++e) m |= (uint32_t)(((w[e / 4] >> (8 * (e % 4))) & 0xffu) != 0) << e;
  return m;
}
__device__ __forceinline__ uint32_t piece_bits(const float* p, float threshold) {
  const float4 v = *reinterpret_cast<const float4*>(p);
  return (uint32_t)(v.x > threshold) | (uint32_t)(v.y > threshold) << 1 | (uint32_t)(v.z > threshold) << 2 |
         (uint32_t)(v.w > threshold) << 3;
}

template <typename T>
__global__ __launch_bounds__(kBlock) void runs_count_kernel(CountArgs a) {
  constexpr int E = 16 / (int)sizeof(T);      // elements of a 16-byte piece
  constexpr int kPieces = kTile / E + 1;      // pieces of a row that begins up to E - 1 elements above a boundary
  __shared__ unsigned long long rows[kTile + 1];   // [0]: the row above the tile; [1 + r]: tile row r
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int per_plane = a.tiles_x * a.tiles_y;
  const int64_t tiles = (int64_t)a.n * per_plane, pixels = (int64_t)a.height * a.width;
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {   // (uniform over the workgroup)
    // the mask runs fastest: the workgroups in flight at one time spread over all masks, and so do their atomics on the
    // five stats words of a mask (all tiles of a mask meet there, and atomics on one cache line take turns)
    const int in_plane = (int)(t / a.n), k = (int)(t - (int64_t)in_plane * a.n);
    const int ty = in_plane / a.tiles_x, y0 = ty * kTile, x0 = in_plane % a.tiles_x * kTile;
    const int th = min(kTile, a.height - y0), tw = min(kTile, a.width - x0);
    const T* plane = static_cast<const T*>(a.planes) + k * pixels;
    if (tid <= kTile) rows[tid] = 0;
    __syncthreads();
    // ---- load
    if (wave == 0) {
      bool one = false;
      if (lane < tw) {
        if (ty > 0)
          one = is_one(plane[(int64_t)(y0 - 1) * a.width + x0 + lane], a.threshold);
        else if (x0 + lane > 0)
          one = is_one(plane[(int64_t)(a.height - 1) * a.width + x0 + lane - 1], a.threshold);
      }
      const unsigned long long above = __ballot(one);
      if (lane == 0) rows[0] = above;
    }
    for (int item = tid; item < th * kPieces; item += kBlock) {
      const int r = item / kPieces;
      const T* row = plane + (int64_t)(y0 + r) * a.width + x0;
      const int shift = (int)((reinterpret_cast<uintptr_t>(row) & 15) / sizeof(T));
      const int c0 = item % kPieces * E - shift;   // the tile column of the piece's first element: -(E - 1) .. kTile
      uint32_t m = 0;
      if (c0 >= 0 && c0 + E <= tw) {
        m = piece_bits(row + c0, a.threshold);
      } else {
#pragma unroll
        for (int e = 0; e < E; ++e)
          if (c0 + e >= 0 && c0 + e < tw) m |= (uint32_t)is_one(row[c0 + e], a.threshold) << e;
      }
      if (m) atomicOr(&rows[1 + r], c0 >= 0 ? (unsigned long long)m << c0 : (unsigned long long)m >> -c0);   // (m != 0: c0 < kTile)
    }
    __syncthreads();
    // ---- words
    const unsigned long long mine = rows[1 + lane];            // (zero from row th on and from column tw on)
    const unsigned long long diff = lane < th ? mine ^ rows[lane] : 0ull;
    unsigned long long word = 0;
#pragma unroll 4   // (fully unrolled, the 16 ballot words are all live in SGPRs at once and some spill)
    for (int j = 0; j < kWaveColumns; ++j) {
      const unsigned long long w = __ballot((diff >> (wave * kWaveColumns + j)) & 1);
      if (lane == j) word = w;
    }
    const int c = wave * kWaveColumns + lane;
    if (lane < kWaveColumns && c < tw) {
      const int64_t seg = (int64_t)k * a.segments + (int64_t)(x0 + c) * a.tiles_y + ty;
      a.bits[2 * seg] = (uint32_t)word;
      a.bits[2 * seg + 1] = (uint32_t)(word >> 32);
      a.off[seg] = __popcll(word);
    }
    // ---- stats
    if (a.stats && wave == 0) {
      const unsigned long long set_rows = __ballot(mine != 0);
      if (set_rows) {                                           // (uniform over the wave)
        int area = __popcll(mine);
        unsigned long long columns = mine;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
          area += __shfl_xor(area, d);
          columns |= __shfl_xor(columns, d);
        }
        if (lane == 0) {
          int32_t* s = a.stats + 5 * (int64_t)k;
          atomicAdd(s, area);
          atomicMin(s + 1, x0 + (int)__ffsll((long long)columns) - 1);
          atomicMin(s + 2, y0 + (int)__ffsll((long long)set_rows) - 1);
          atomicMax(s + 3, x0 + 63 - (int)__clzll((long long)columns));
          atomicMax(s + 4, y0 + 63 - (int)__clzll((long long)set_rows));
        }
      }
    }
    __syncthreads();   // the next tile reuses the LDS
  }
}

// E4's empty mask
__global__ __launch_bounds__(kBlock) void runs_stats_init_kernel(int32_t* stats, int n) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i < n * 5) {
    const int f = i % 5;
    stats[i] = f == 0 ? 0 : (f <= 2 ? INT32_MAX : -1);
  }
}

// one workgroup per mask: popcounts -> exclusive offsets, in place; n_out[k] = their sum (below 2^31: E6)
__global__ __launch_bounds__(kBlock) void runs_scan_kernel(int32_t* off, int segments, int32_t* n_out) {
  __shared__ int wave_sums[kWaves];
  const int tid = threadIdx.x;
  int32_t* mine = off + (int64_t)blockIdx.x * segments;
  int running = 0;
  for (int begin = 0; begin < segments; begin += DEVA_RUNS_SCAN_CHUNK) {   // (12 * segments <= DEVA_RUNS_MAX_SCRATCH: no overflow)
    const int64_t i0 = (int64_t)begin + tid * kScanItems;
    int v[kScanItems], sum = 0;
#pragma unroll
    for (int e = 0; e < kScanItems; ++e) {
      v[e] = i0 + e < segments ? mine[i0 + e] : 0;
      sum += v[e];
    }
    int before, all;
    block_scan::block_exclusive<block_scan::Sum>(sum, 0, wave_sums, tid, before, all);
    before += running;
#pragma unroll
    for (int e = 0; e < kScanItems; ++e) {
      if (i0 + e < segments) mine[i0 + e] = before;
      before += v[e];
    }
    running += all;
  }
  if (tid == 0) n_out[blockIdx.x] = running;
}

// one workgroup: base[k] = first + n[0] + ... + n[k-1], total = first + all of them (E5)
__global__ __launch_bounds__(kBlock) void runs_base_kernel(const int32_t* n_in, int n, const int64_t* first, int64_t* base,
                                                           int64_t* total) {
  __shared__ long long wave_sums[kWaves];
  const long long all = block_scan::block_offsets(n_in, n, first ? (long long)*first : 0ll, base, wave_sums, threadIdx.x);
  if (threadIdx.x == 0) *total = all;
}

struct WriteArgs {
  const int32_t* off;
  const uint32_t* bits;
  const int64_t* base;
  int32_t* bounds;
  int64_t capacity;
  int n, height, tiles_y, segments;
};

__global__ __launch_bounds__(kBlock) void runs_write_kernel(WriteArgs a) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int per_mask = (a.segments + kBlock - 1) / kBlock;
  const int64_t chunks = (int64_t)a.n * per_mask;
  for (int64_t t = blockIdx.x; t < chunks; t += gridDim.x) {   // (uniform over the workgroup)
    const int k = (int)(t / per_mask);
    const int64_t wave_first = (t - (int64_t)k * per_mask) * kBlock + (tid - lane);   // the wave's first segment
    const int64_t s = wave_first + lane, at = (int64_t)k * a.segments + s;
    unsigned long long word = 0;
    int off = 0;
    if (s < a.segments) {
      word = (unsigned long long)a.bits[2 * at] | (unsigned long long)a.bits[2 * at + 1] << 32;
      off = a.off[at];
    }
    unsigned long long busy = __ballot(word != 0);
    if (!busy) continue;                                        // (uniform over the wave; no barrier in this kernel)
    const int64_t base = a.base[k];
    while (busy) {
      const int j = (int)__ffsll((long long)busy) - 1;
      busy &= busy - 1;
      const unsigned long long w = __shfl(word, j);
      const int64_t slot = base + __shfl(off, j) + __popcll(w & ((1ull << lane) - 1));
      if (((w >> lane) & 1) && slot < a.capacity) {
        const int64_t seg = wave_first + j;
        const int x = (int)(seg / a.tiles_y), ty = (int)(seg - (int64_t)x * a.tiles_y);
        a.bounds[slot] = x * a.height + ty * kTile + lane;      // p = x * H + y < H * W < 2^31
      }
    }
  }
}

LAUNCH_CHECK_DEFINE_LAUNCHED()

}  // namespace
}  // namespace deva_runs

extern "C" int deva_runs_count(const void* planes, int dtype, float threshold, int n, int height, int width, void* scratch,
                               int64_t scratch_bytes, int32_t* n_out, int64_t* base, int64_t* total, const int64_t* first,
                               int32_t* stats, void* stream) {
  using namespace deva_runs;
  struct deva_runs_plan plan;
  if (int rc = count_check(planes, dtype, n, height, width, scratch, scratch_bytes, n_out, base, total, first, stats, &plan)) return rc;
  if (n == 0) return 0;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const Scratch sc = carve(scratch, n, plan);
  if (stats) hipLaunchKernelGGL(runs_stats_init_kernel, dim3((n * 5 + kBlock - 1) / kBlock), dim3(kBlock), 0, st, stats, n);
  const CountArgs a = {planes, sc.off, sc.bits, stats, threshold, n, height, width, plan.tiles_x, plan.tiles_y, plan.segments};
  if (dtype == DEVA_RUNS_F32)
    hipLaunchKernelGGL(runs_count_kernel<float>, dim3(plan.count_grid), dim3(kBlock), 0, st, a);
  else
    hipLaunchKernelGGL(runs_count_kernel<uint8_t>, dim3(plan.count_grid), dim3(kBlock), 0, st, a);
  hipLaunchKernelGGL(runs_scan_kernel, dim3(n), dim3(kBlock), 0, st, sc.off, plan.segments, n_out);
  hipLaunchKernelGGL(runs_base_kernel, dim3(1), dim3(kBlock), 0, st, n_out, n, first, base, total);
  return launched("deva_runs_count");
}

extern "C" int deva_runs_write(int n, int height, int width, const void* scratch, int64_t scratch_bytes, const int64_t* base,
                               int32_t* bounds, int64_t capacity, void* stream) {
  using namespace deva_runs;
  struct deva_runs_plan plan;
  if (int rc = write_check(n, height, width, scratch, scratch_bytes, base, bounds, capacity, &plan)) return rc;
  if (n == 0 || capacity == 0) return 0;
  const Scratch sc = carve(const_cast<void*>(scratch), n, plan);
  const WriteArgs a = {sc.off, sc.bits, base, bounds, capacity, n, height, plan.tiles_y, plan.segments};
  hipLaunchKernelGGL(runs_write_kernel, dim3(plan.write_grid), dim3(kBlock), 0, static_cast<hipStream_t>(stream), a);
  return launched("deva_runs_write");
}
