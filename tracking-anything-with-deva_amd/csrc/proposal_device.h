// Device code that the proposal filter (proposals.hip, libdeva_hip.so) and the filter from low-resolution logits
// (lowres/lowres.hip, libdeva_lowres.so) both compile: the arguments of a batch, the live test, the per-lane tally of
// rule 2 and 4 with its reduction into the mask's record, and the decide kernel.  One text, two translation units, as
// affinity_common.h, rle_walk.h and region_union.h are; everything is in an unnamed namespace, so neither library
// exports or shares a symbol of it.
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>

#include "proposal_plan.h"

namespace deva {
namespace {

struct PropArgs {
  const float* logits;  // plane 0 of this launch
  const float* iou;     // its predicted IoU
  int nb, hw, w;
  float t_hi, t_lo, t_mask, t_iou, t_stab;
  int iou_on, stab_on;  // the reference's `> 0.0` guards, decided on the doubles
  uint8_t* arena;
  int capacity;
  int32_t* stats;
  int32_t* slots;
  int32_t* count;
  int32_t* table;
};

__device__ __forceinline__ bool prop_live(const PropArgs& a, int k) { return !a.iou_on || a.iou[k] > a.t_iou; }

// ------------------------------------------------------------------------------------------ stats
struct PropTally {
  int hi, lo, x_min, x_max, i_min, i_max;
};

__device__ __forceinline__ void prop_take(const PropArgs& a, float v, int i, int x, PropTally& s) {
  s.hi += v > a.t_hi;
  s.lo += v > a.t_lo;
  if (v > a.t_mask) {
    s.x_min = min(s.x_min, x), s.x_max = max(s.x_max, x);
    s.i_min = min(s.i_min, i), s.i_max = max(s.i_max, i);
  }
}

// the tallies of a workgroup of 256 lanes into the record of mask k: wave shuffles, LDS, then one integer atomic per
// workgroup and field -- the same record whatever the order of the workgroups.  Every lane of the workgroup calls it.
__device__ __forceinline__ void prop_commit(const PropArgs& a, int k, PropTally s, int32_t (*red)[6]) {
  const int t = threadIdx.x;
  for (int o = 32; o > 0; o >>= 1) {
    s.hi += __shfl_xor(s.hi, o), s.lo += __shfl_xor(s.lo, o);
    s.x_min = min(s.x_min, __shfl_xor(s.x_min, o)), s.x_max = max(s.x_max, __shfl_xor(s.x_max, o));
    s.i_min = min(s.i_min, __shfl_xor(s.i_min, o)), s.i_max = max(s.i_max, __shfl_xor(s.i_max, o));
  }
  if ((t & 63) == 0) {
    int32_t* r = red[t >> 6];
    r[0] = s.hi, r[1] = s.lo, r[2] = s.x_min, r[3] = s.i_min, r[4] = s.x_max, r[5] = s.i_max;
  }
  __syncthreads();
  if (t == 0) {
    for (int v = 1; v < 4; ++v) {
      s.hi += red[v][0], s.lo += red[v][1];
      s.x_min = min(s.x_min, red[v][2]), s.i_min = min(s.i_min, red[v][3]);
      s.x_max = max(s.x_max, red[v][4]), s.i_max = max(s.i_max, red[v][5]);
    }
    int32_t* r = a.stats + k * kPropStat;  // integer atomics: the same record whatever the order of the workgroups
    if (s.hi) atomicAdd(r + 0, s.hi);
    if (s.lo) atomicAdd(r + 1, s.lo);
    if (s.x_max >= 0) {
      atomicMin(r + 2, s.x_min), atomicMin(r + 3, s.i_min);
      atomicMax(r + 4, s.x_max), atomicMax(r + 5, s.i_max);
    }
  }
}

// ------------------------------------------------------------------------------------------ decide
__global__ void __launch_bounds__(kPropBatch) prop_decide_kernel(PropArgs a) {
  __shared__ int32_t wave_sum[kPropBatch / 64];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int32_t passed_before = a.count[0];
  bool pass = false;
  float stability = 0.0f;
  int32_t box[4] = {0, 0, 0, 0};
  if (t < a.nb) {
    int32_t* s = a.stats + t * kPropStat;
    if (prop_live(a, t)) {
      // int32 / int32 as torch divides them: both to fp32, one correctly rounded division; 0 / 0 is NaN and fails >=
      stability = __fdiv_rn((float)s[0], (float)s[1]);
      pass = !a.stab_on || stability >= a.t_stab;
      if (s[4] >= 0) box[0] = s[2], box[1] = s[3] / a.w, box[2] = s[4], box[3] = s[5] / a.w;
    }
    s[0] = 0, s[1] = 0, s[2] = INT_MAX, s[3] = INT_MAX, s[4] = -1, s[5] = -1;  // for the next batch
  }
  const unsigned long long ballot = __ballot(pass);
  const int before = __popcll(ballot & ((1ull << lane) - 1));
  if (lane == 0) wave_sum[wave] = __popcll(ballot);
  __syncthreads();
  int offset = 0, total = 0;
  for (int v = 0; v < kPropBatch / 64; ++v) {
    const int n = wave_sum[v];
    offset += v < wave ? n : 0;
    total += n;
  }
  int32_t slot = -1;
  if (pass) {
    const int64_t at = (int64_t)passed_before + offset + before;  // arrival order
    if (at >= 0 && at < a.capacity) {  // (beyond: counted below, stored nowhere)
      slot = (int32_t)at;
      int32_t* row = a.table + (int64_t)slot * kPropRow;
      row[0] = slot, row[1] = __float_as_int(a.iou[t]), row[2] = __float_as_int(stability);
      row[3] = box[0], row[4] = box[1], row[5] = box[2], row[6] = box[3], row[7] = 0;
    }
  }
  if (t < a.nb) a.slots[t] = slot;
  if (t == 0) a.count[0] = passed_before + total;
}

}  // namespace
}  // namespace deva
