// The workgroup scan of the run-length, text and PNG libraries (mask_runs/, rle_text/, rle_overlap/, png/): a shuffle
// scan over each wave, the waves' parts in LDS, two barriers.  Header-only device text with internal linkage, included
// as "../block_scan.h": every library compiles its own copy and no library exports or shares anything from it.
//
// One text serves every operation but for one line, wave_before.  Its general form takes the inclusive value of the
// lane below by one more shuffle; a sum takes `inclusive - v` instead.  The general form was tried for the sums as
// well: the compiler does not see through it, and every sum scan of a step loop then paid a ds_bpermute_b32 and a
// v_cndmask_b32 per 32 bits where it had a v_sub.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

namespace block_scan {
namespace {

struct Sum {
  template <typename V>
  __device__ __forceinline__ static V of(V a, V b) { return a + b; }
};
struct Max {
  template <typename V>
  __device__ __forceinline__ static V of(V a, V b) { return a > b ? a : b; }
};

// inclusive scan over the wave
template <typename Op, typename V>
__device__ __forceinline__ V wave_inclusive(V v, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const V up = __shfl_up(v, d);
    if (lane >= d) v = Op::of(v, up);
  }
  return v;
}

// Op over the lanes before this one in the wave, or `none`
template <typename Op, typename V>
__device__ __forceinline__ V wave_before(V inclusive, V v, V none, int lane) {
  if constexpr (std::is_same<Op, Sum>::value) {
    return inclusive - v;
  } else {
    const V up = __shfl_up(inclusive, 1);
    return lane ? up : none;
  }
}

// -> (Op over the lanes before this one in the workgroup, or `none`; Op over the workgroup).  `wave_parts` is an LDS
// array with one entry per wave of the workgroup, all of whose kWaves * 64 lanes call.
//
// Two barriers.  The first publishes the waves' parts before any wave reads them.  The second keeps a wave that has
// read them from running ahead into the next call on the same array (the next step of a loop, or the next scan that
// reuses it) and storing its new part while a slower wave is still reading the old ones.
template <typename Op, typename V, int kWaves>
__device__ __forceinline__ void block_exclusive(V v, V none, V (&wave_parts)[kWaves], int tid, V& before, V& all) {
  const int lane = tid & 63, wave = tid >> 6;
  const V inclusive = wave_inclusive<Op>(v, lane);
  if (lane == 63) wave_parts[wave] = inclusive;
  before = wave_before<Op>(inclusive, v, none, lane);
  __syncthreads();
  all = none;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) {
    if (w < wave) before = Op::of(before, wave_parts[w]);
    all = Op::of(all, wave_parts[w]);
  }
  __syncthreads();
}

// One workgroup of kWaves * 64 lanes, that many counts a step: base[k] = first + counts[0] + ... + counts[k-1] for
// k < n, in 64 bits; -> first + all of them.
template <int kWaves>
__device__ __forceinline__ long long block_offsets(const int32_t* counts, int n, long long first, int64_t* base,
                                                   long long (&wave_parts)[kWaves], int tid) {
  long long running = first;
  for (int begin = 0; begin < n; begin += kWaves * 64) {
    const int i = begin + tid;
    const long long v = i < n ? (long long)counts[i] : 0ll;
    long long before, all;
    block_exclusive<Sum>(v, 0ll, wave_parts, tid, before, all);
    if (i < n) base[i] = running + before;
    running += all;
  }
  return running;
}

}  // namespace
}  // namespace block_scan
