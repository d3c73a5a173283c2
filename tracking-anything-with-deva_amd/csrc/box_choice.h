// Rule S1 of deva_box_mask_select (include/deva_hip.h) on the device: one text that box_prompts.hip (libdeva_hip.so) and
// lowres/lowres.hip (libdeva_lowres.so) both compile, in an unnamed namespace like proposal_device.h.
#pragma once
#include <hip/hip_runtime.h>

namespace deva {
namespace {

// numpy's argmax: the first NaN if there is one, else the first maximum (-0.0 == 0.0)
__device__ __forceinline__ int box_choice(const float* s, int n) {
  int best = 0;
  float v = s[0];
  for (int m = 1; m < n; ++m) {
    const float c = s[m];
    if (v == v && (c != c || c > v)) best = m, v = c;
  }
  return best;
}

}  // namespace
}  // namespace deva
