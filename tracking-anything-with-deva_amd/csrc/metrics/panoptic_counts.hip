// deva_metrics_panoptic_counts (include/deva_metrics.h, rules C1-C4): the G x P table of (ground-truth slot, predicted slot)
// pixel counts of one frame, in one pass over the two planes.
//
// Every lane takes strips of 16 consecutive pixels (48 / 32 / 64 / 128 bytes of RGB / int16 / int32 / int64: 16-byte
// loads).  The sorted id tables sit in LDS and an id is found by binary search, but only when it differs from the lane's
// previous one: panoptic maps are long runs, so the last (id, slot) of either side stays in registers.  Equal consecutive
// (g, p) pairs are merged into one run before anything is added.  Runs go to a per-workgroup copy of the table in LDS
// (LDS = true; the plan decides) whose non-zero bins are flushed with one integer atomic each, or straight to the
// global table.  Integer adds: exact, and independent of the order.
#include <hip/hip_runtime.h>
#include <limits.h>

#include "panoptic_plan.h"

namespace deva_metrics {
namespace {

constexpr int S = DEVA_METRICS_STRIP;

// ids (C1; the channel for INDEX16) of the pixels first .. first + valid - 1 of a plane; a full strip is read 16 bytes at
// a time (first is a multiple of 16 and the plane is 16-byte aligned, so every load is), a cut one element by element
template <int ENC>
__device__ __forceinline__ void load_strip(const void* plane, int64_t first, int valid, int (&ids)[S]) {
  if constexpr (ENC == DEVA_METRICS_RGB8) {
    const uint8_t* p = static_cast<const uint8_t*>(plane) + first * 3;
    if (valid == S) {
      const uint4* q = reinterpret_cast<const uint4*>(p);
      const uint4 a = q[0], b = q[1], c = q[2];
      const uint32_t w[12] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w};
#pragma unroll
      for (int k = 0; k < S; ++k) {  // r + 256 g + 65536 b: the 24 bits at byte 3 k
        const int i = (3 * k) >> 2, sh = ((3 * k) & 3) * 8;
        const uint64_t pair = (uint64_t)w[i] | ((uint64_t)(i + 1 < 12 ? w[i + 1] : 0u) << 32);
        ids[k] = (int)((pair >> sh) & 0xffffffu);
      }
    } else {
#pragma unroll
      for (int k = 0; k < S; ++k)
        if (k < valid) ids[k] = (int)p[3 * k] | ((int)p[3 * k + 1] << 8) | ((int)p[3 * k + 2] << 16);
    }
  } else if constexpr (ENC == DEVA_METRICS_I32) {
    const int* p = static_cast<const int*>(plane) + first;
    if (valid == S) {
      const int4* q = reinterpret_cast<const int4*>(p);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int4 v = q[j];
        ids[4 * j] = v.x, ids[4 * j + 1] = v.y, ids[4 * j + 2] = v.z, ids[4 * j + 3] = v.w;
      }
    } else {
#pragma unroll
      for (int k = 0; k < S; ++k)
        if (k < valid) ids[k] = p[k];
    }
  } else if constexpr (ENC == DEVA_METRICS_I64) {
    const long long* p = static_cast<const long long*>(plane) + first;
    auto narrow = [](long long v) { return v < 0 || v > (long long)INT_MAX ? -1 : (int)v; };  // (C1: unlisted)
    if (valid == S) {
      const longlong2* q = reinterpret_cast<const longlong2*>(p);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const longlong2 v = q[j];
        ids[2 * j] = narrow(v.x), ids[2 * j + 1] = narrow(v.y);
      }
    } else {
#pragma unroll
      for (int k = 0; k < S; ++k)
        if (k < valid) ids[k] = narrow(p[k]);
    }
  } else {
    const short* p = static_cast<const short*>(plane) + first;
    if (valid == S) {
      const uint4* q = reinterpret_cast<const uint4*>(p);
      const uint4 a = q[0], b = q[1];
      const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        ids[2 * j] = (int)(short)(w[j] & 0xffffu), ids[2 * j + 1] = (int)(short)(w[j] >> 16);
      }
    } else {
#pragma unroll
      for (int k = 0; k < S; ++k)
        if (k < valid) ids[k] = p[k];
    }
  }
}

// C2: the slot of an id in a sorted table of n ids (LDS)
__device__ __forceinline__ int find_slot(const int* table, int n, int id) {
  if (id == 0) return 0;
  if (id < 0) return 1;
  int lo = 0, hi = n;  // the first entry >= id
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (table[mid] < id) lo = mid + 1;
    else hi = mid;
  }
  return lo < n && table[lo] == id ? lo + 2 : 1;
}

template <int GT, int PR, bool LDS>
__global__ __launch_bounds__(kBlock) void panoptic_counts_kernel(const void* __restrict__ gt, const int* __restrict__ gt_ids, int n_gt,
                                                                const void* __restrict__ pred, const int* __restrict__ pred_ids,
                                                                int n_pred, const uint16_t* __restrict__ lut, int channels,
                                                                int64_t pixels, uint32_t* __restrict__ counts) {
  extern __shared__ int smem[];  // gt table [n_gt], predicted table [n_pred], then (LDS) the workgroup's bins [G * P]
  int* tab_g = smem;
  int* tab_p = smem + n_gt;
  uint32_t* bins = reinterpret_cast<uint32_t*>(smem + n_gt + n_pred);
  const int P = n_pred + 2;
  const int n_bins = (n_gt + 2) * P;
  const int tid = threadIdx.x;
  for (int i = tid; i < n_gt; i += kBlock) tab_g[i] = gt_ids[i];
  if constexpr (PR != DEVA_METRICS_INDEX16)
    for (int i = tid; i < n_pred; i += kBlock) tab_p[i] = pred_ids[i];
  if constexpr (LDS)
    for (int i = tid; i < n_bins; i += kBlock) bins[i] = 0u;
  __syncthreads();

  int last_g = 0, slot_g = 0;                                             // (id 0 is slot 0 on either side)
  int last_p = PR == DEVA_METRICS_INDEX16 ? INT_MIN : 0, slot_p = 0;      // (no int16 channel is INT_MIN)
  int run_bin = 0;
  uint32_t run = 0;
  auto add = [&](int bin, uint32_t n) {
    if constexpr (LDS) atomicAdd(&bins[bin], n);
    else atomicAdd(&counts[bin], n);
  };
  const int64_t strips = (pixels + S - 1) / S;
  for (int64_t s = (int64_t)blockIdx.x * kBlock + tid; s < strips; s += (int64_t)gridDim.x * kBlock) {
    const int64_t first = s * S;
    const int valid = pixels - first < S ? (int)(pixels - first) : S;
    int g[S], p[S];
    load_strip<GT>(gt, first, valid, g);
    load_strip<PR>(pred, first, valid, p);
#pragma unroll
    for (int k = 0; k < S; ++k) {
      if (k < valid) {
        if (g[k] != last_g) {
          last_g = g[k];
          slot_g = find_slot(tab_g, n_gt, last_g);
        }
        if (p[k] != last_p) {
          last_p = p[k];
          if constexpr (PR == DEVA_METRICS_INDEX16) {  // C3
            const int e = last_p >= 0 && last_p < channels ? (int)lut[last_p] : 1;
            slot_p = e < P ? e : 1;
          } else {
            slot_p = find_slot(tab_p, n_pred, last_p);
          }
        }
        const int bin = slot_g * P + slot_p;
        if (bin == run_bin) {
          ++run;
        } else {
          if (run) add(run_bin, run);
          run_bin = bin, run = 1u;
        }
      }
    }
  }
  if (run) add(run_bin, run);
  if constexpr (LDS) {
    __syncthreads();
    for (int i = tid; i < n_bins; i += kBlock) {
      const uint32_t v = bins[i];
      if (v) atomicAdd(&counts[i], v);
    }
  }
}

template <int GT, int PR>
void launch(const deva_metrics_plan& plan, const void* gt, const int* gt_ids, int n_gt, const void* pred, const int* pred_ids,
            int n_pred, const uint16_t* lut, int channels, int64_t pixels, uint32_t* counts, hipStream_t stream) {
  if (plan.path == DEVA_METRICS_PATH_LDS)
    hipLaunchKernelGGL((panoptic_counts_kernel<GT, PR, true>), dim3(plan.grid), dim3(plan.block), plan.lds_bytes, stream, gt, gt_ids,
                       n_gt, pred, pred_ids, n_pred, lut, channels, pixels, counts);
  else
    hipLaunchKernelGGL((panoptic_counts_kernel<GT, PR, false>), dim3(plan.grid), dim3(plan.block), plan.lds_bytes, stream, gt, gt_ids,
                       n_gt, pred, pred_ids, n_pred, lut, channels, pixels, counts);
}

template <int GT>
void launch_pred(int pred_encoding, const deva_metrics_plan& plan, const void* gt, const int* gt_ids, int n_gt, const void* pred,
                 const int* pred_ids, int n_pred, const uint16_t* lut, int channels, int64_t pixels, uint32_t* counts,
                 hipStream_t stream) {
  switch (pred_encoding) {
    case DEVA_METRICS_RGB8:
      return launch<GT, DEVA_METRICS_RGB8>(plan, gt, gt_ids, n_gt, pred, pred_ids, n_pred, lut, channels, pixels, counts, stream);
    case DEVA_METRICS_I32:
      return launch<GT, DEVA_METRICS_I32>(plan, gt, gt_ids, n_gt, pred, pred_ids, n_pred, lut, channels, pixels, counts, stream);
    case DEVA_METRICS_I64:
      return launch<GT, DEVA_METRICS_I64>(plan, gt, gt_ids, n_gt, pred, pred_ids, n_pred, lut, channels, pixels, counts, stream);
    default:
      return launch<GT, DEVA_METRICS_INDEX16>(plan, gt, gt_ids, n_gt, pred, pred_ids, n_pred, lut, channels, pixels, counts,
                                              stream);
  }
}

}  // namespace
}  // namespace deva_metrics

extern "C" int deva_metrics_panoptic_counts(const void* gt, int gt_encoding, const int32_t* gt_ids, int n_gt, const void* pred,
                                            int pred_encoding, const int32_t* pred_ids, int n_pred, const uint16_t* pred_lut,
                                            int channels, int height, int width, uint32_t* counts, void* stream) {
  using namespace deva_metrics;
  deva_metrics_plan plan;
  if (int rc = panoptic_counts_check(gt, gt_encoding, gt_ids, n_gt, pred, pred_encoding, pred_ids, n_pred, pred_lut, channels, height,
                                     width, counts, &plan))
    return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipError_t e = hipMemsetAsync(counts, 0, sizeof(uint32_t) * (size_t)(n_gt + 2) * (size_t)(n_pred + 2), st);
  if (e != hipSuccess) {
    set_error("deva_metrics_panoptic_counts: clearing the table: %s", hipGetErrorString(e));
    return 1;
  }
  const int64_t pixels = (int64_t)height * width;
  if (gt_encoding == DEVA_METRICS_RGB8)
    launch_pred<DEVA_METRICS_RGB8>(pred_encoding, plan, gt, gt_ids, n_gt, pred, pred_ids, n_pred, pred_lut, channels, pixels, counts, st);
  else
    launch_pred<DEVA_METRICS_I32>(pred_encoding, plan, gt, gt_ids, n_gt, pred, pred_ids, n_pred, pred_lut, channels, pixels, counts, st);
  e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("deva_metrics_panoptic_counts: launch failed: %s", hipGetErrorString(e));
    return 1;
  }
  return 0;
}
