// deva_overlap_intersections (include/deva_rle_overlap.h, rules O1-O9): the overlap of every detection with every
// ground-truth mask from their COCO run lengths, on the device.  No plane, no pixel: two launches over the run arrays.
//
//   scan   overlap_scan_kernel: a workgroup per mask of either side (a grid-stride loop).  v[k] = s[k+1] - s[k] for odd
//          k (a one-run), 0 otherwise; their exclusive scan, kScanItems per lane and step, is ones_before[k], kept for
//          the ground-truth side only (the scratch); its total is the mask's area.
//   pairs  overlap_pair_kernel: a workgroup owns one g and kChunkD consecutive d (a grid-stride loop, d-chunk fastest, so
//          the workgroups in flight share few g).  The box test (O6) leaves a flag per d in LDS; if every flag is down,
//          g's runs are never read.  Otherwise g's starts and ones_before go to LDS when they fit (kLdsRuns) and every
//          lane runs `lane_pairs` of overlap_walk.h: one search, then a merge down its stretch of the chunk's starts.
//          The lanes of a wave search different places of the same two LDS arrays, so their reads conflict on banks as
//          random addresses do; the merge that follows reads ascending addresses per lane.  At just under 16 KB a
//          workgroup the LDS would let every SIMD hold eight waves; the compiler's 103 SGPRs make it seven.
//
// Every load lies inside the two run arrays as O2 checked them, the boxes and the scratch; every store inside the scratch,
// inter (d * pitch + g, g < G), area_d and area_g.
#include <hip/hip_runtime.h>

#include "../block_scan.h"
#include "../launch_check.h"
#include "overlap_walk.h"
#include "rle_overlap_plan.h"

namespace deva_overlap {
namespace {

static_assert(kBlock == 256 && kScanItems * kBlock == DEVA_OVERLAP_SCAN_CHUNK, "the scan's step");
static_assert(kChunkD <= 64, "the chunk's flags and counters are handled by the first wave");
constexpr int kWaves = kBlock / 64;

struct ScanArgs {
  const int32_t* dt;   // run arrays: first[0 .. n], then the starts
  const int32_t* gt;
  int32_t* before_g;   // [first_g[G]]: ones_before of the ground-truth side, laid out as its starts
  uint32_t* area_d;
  uint32_t* area_g;
  int d, g;
};

__global__ __launch_bounds__(kBlock) void overlap_scan_kernel(ScanArgs a) {
  __shared__ int wave_sums[kWaves];
  const int tid = threadIdx.x;
  for (int m = blockIdx.x; m < a.d + a.g; m += gridDim.x) {   // (uniform over the workgroup)
    const bool gt = m >= a.d;
    const int k = gt ? m - a.d : m, n = gt ? a.g : a.d;
    const int32_t* runs = gt ? a.gt : a.dt;
    const int begin = runs[k], words = runs[k + 1] - begin;   // words = the mask's runs + 1
    const int32_t* s = runs + n + 1 + begin;
    int32_t* before = gt ? a.before_g + begin : nullptr;
    int running = 0;
    for (int at = 0; at < words; at += DEVA_OVERLAP_SCAN_CHUNK) {
      const int i0 = at + tid * kScanItems;
      int v[kScanItems], sum = 0;
#pragma unroll
      for (int e = 0; e < kScanItems; ++e) {
        const int i = i0 + e;
        v[e] = ((i & 1) && i + 1 < words) ? s[i + 1] - s[i] : 0;
        sum += v[e];
      }
      int here, all;
      block_scan::block_exclusive<block_scan::Sum>(sum, 0, wave_sums, tid, here, all);
      here += running;
      running += all;
      if (before) {
#pragma unroll
        for (int e = 0; e < kScanItems; ++e) {
          if (i0 + e < words) before[i0 + e] = here;
          here += v[e];
        }
      }
    }
    if (tid == 0) (gt ? a.area_g : a.area_d)[k] = (uint32_t)running;   // < 2^31 (O2)
  }
}

struct PairArgs {
  const int32_t* dt;
  const int32_t* gt;
  const int32_t* before_g;
  const int32_t* box_d;   // or null, with box_g
  const int32_t* box_g;
  uint32_t* inter;
  int64_t pitch;
  int d, g, d_chunks;
};

__global__ __launch_bounds__(kBlock) void overlap_pair_kernel(PairArgs a) {
  __shared__ int32_t lds_starts[kLdsRuns + 1];
  __shared__ int32_t lds_before[kLdsRuns + 1];
  __shared__ uint32_t sums[kChunkD];
  __shared__ int32_t live[kChunkD];
  const int tid = threadIdx.x;
  const int32_t* starts_d = a.dt + a.d + 1;
  const int64_t items = (int64_t)a.g * a.d_chunks;
  for (int64_t t = blockIdx.x; t < items; t += gridDim.x) {   // (uniform over the workgroup)
    const int g = (int)(t / a.d_chunks), d0 = (int)(t - (int64_t)g * a.d_chunks) * kChunkD;
    const int nd = min(kChunkD, a.d - d0);
    bool meets = false;
    if (tid < kChunkD) {
      meets = tid < nd && (!a.box_d || boxes_meet(a.box_d + 4 * (int64_t)(d0 + tid), a.box_g + 4 * (int64_t)g));
      sums[tid] = 0;
      live[tid] = meets;
    }
    if (__syncthreads_or(meets)) {                             // (uniform; the barrier also publishes sums and live)
      const int begin = a.gt[g], rg = a.gt[g + 1] - begin - 1;
      const int32_t* gs = a.gt + a.g + 1 + begin;
      const int32_t* gob = a.before_g + begin;
      auto add = [&](int dd, uint32_t v) { atomicAdd(&sums[dd], v); };
      if (rg <= kLdsRuns) {
        for (int i = tid; i <= rg; i += kBlock) {
          lds_starts[i] = gs[i];
          lds_before[i] = gob[i];
        }
        __syncthreads();
        lane_pairs(a.dt + d0, starts_d, nd, live, lds_starts, lds_before, rg, tid, kBlock, add);
      } else {
        lane_pairs(a.dt + d0, starts_d, nd, live, gs, gob, rg, tid, kBlock, add);
      }
      __syncthreads();
    }
    if (tid < nd) a.inter[(int64_t)(d0 + tid) * a.pitch + g] = sums[tid];
    __syncthreads();   // the next item reuses the LDS
  }
}

LAUNCH_CHECK_DEFINE_LAUNCHED()

}  // namespace
}  // namespace deva_overlap

extern "C" int deva_overlap_intersections(const int32_t* dt_host, const int32_t* dt_device, int64_t dt_words, int d, const int32_t* gt_host,
                                          const int32_t* gt_device, int64_t gt_words, int g, int height, int width, const int32_t* box_d,
                                          const int32_t* box_g, void* scratch, int64_t scratch_bytes, uint32_t* inter, int64_t pitch,
                                          uint32_t* area_d, uint32_t* area_g, void* stream) {
  using namespace deva_overlap;
  struct deva_overlap_plan plan;
  if (int rc = intersections_check(dt_host, dt_device, dt_words, d, gt_host, gt_device, gt_words, g, height, width, box_d, box_g, scratch,
                                   scratch_bytes, inter, pitch, area_d, area_g, &plan))
    return rc;
  if (d == 0 || g == 0) return 0;
  hipStream_t st = static_cast<hipStream_t>(stream);
  int32_t* before_g = static_cast<int32_t*>(scratch);
  const ScanArgs scan = {dt_device, gt_device, before_g, area_d, area_g, d, g};
  hipLaunchKernelGGL(overlap_scan_kernel, dim3(plan.scan_grid), dim3(kBlock), 0, st, scan);
  const PairArgs pairs = {dt_device, gt_device, before_g, box_d, box_g, inter, pitch, d, g, plan.d_chunks};
  hipLaunchKernelGGL(overlap_pair_kernel, dim3(plan.pair_grid), dim3(kBlock), 0, st, pairs);
  return launched("deva_overlap_intersections");
}
