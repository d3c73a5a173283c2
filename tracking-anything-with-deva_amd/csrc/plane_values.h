// How the two DAVIS scorers (pair_metrics/pair_counts.hip, vos_metrics/boundary_counts.hip) read a label plane: the raw
// value of a pixel, the slot of a value in a sorted id table or a look-up table, and a slot's bit.  Header-only device
// text with internal linkage, included as "../plane_values.h".  The encodings are the codes that both public headers
// give (DEVA_PAIR_* and DEVA_VOS_*: 0 .. 3 in this order), which each scorer asserts for its own.
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

namespace plane_values {
namespace {

enum { kU8 = 0, kI32 = 1, kI64 = 2, kIndex16 = 3 };

// the raw value of pixel i of a plane as an int; an int64 outside the int range becomes -1 (non-zero, and in no table)
template <int ENC>
__device__ __forceinline__ int load_value(const void* plane, int64_t i) {
  if constexpr (ENC == kU8) return (int)static_cast<const uint8_t*>(plane)[i];
  else if constexpr (ENC == kI32) return static_cast<const int*>(plane)[i];
  else if constexpr (ENC == kI64) {
    const long long v = static_cast<const long long*>(plane)[i];
    return v < (long long)INT_MIN || v > (long long)INT_MAX ? -1 : (int)v;
  } else return (int)static_cast<const short*>(plane)[i];
}

// the slot of a value in one side's table, -1 for none: by `lut` for kIndex16, else by binary search in the sorted `table`
template <int ENC>
__device__ __forceinline__ int find_slot(int value, const int* table, int n, const uint16_t* lut, int channels) {
  if constexpr (ENC == kIndex16) {
    if (value < 0 || value >= channels) return -1;
    const int e = (int)lut[value];
    return e < n ? e : -1;
  } else {
    if (value < 1) return -1;
    int lo = 0, hi = n;  // the first entry >= value
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (table[mid] < value) lo = mid + 1;
      else hi = mid;
    }
    return lo < n && table[lo] == value ? lo : -1;
  }
}

__device__ __forceinline__ uint64_t bit_of(int slot) { return slot >= 0 ? 1ull << slot : 0ull; }

}  // namespace
}  // namespace plane_values
