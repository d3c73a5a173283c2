// The arithmetic of rle_decode.hip that is no HIP: the nearest source index (D3), the search for the run that owns a
// position and the walk to the run that owns a later one (D1), and the shift of a tile row.  The kernel runs these on
// the device; tests/rle_plan_sanitize_main.cpp runs the same functions on the host, on run arrays of exactly their size
// under the address sanitizer, against a decoder written as a loop.
#pragma once
#include <math.h>
#include <stdint.h>

namespace deva_rle {

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RLE_WALK_FN __host__ __device__ __forceinline__
#else
#define RLE_WALK_FN inline
#endif

// D3, as ATen's nearest_neighbor_compute_source_index: scale = in / out in fp32 (rle_plan.cpp)
RLE_WALK_FN int source_index(int dst, float scale, int in) {
  const int src = (int)floorf((float)dst * scale);
  return src < in - 1 ? src : in - 1;
}

// s[0 .. runs]: the starts of a mask, s[0] = 0 <= p < s[runs] = H * W, never descending -> the last run whose start is
// <= p (D1: among runs that share a start the last one owns the pixel).  Reads s[1 .. runs - 1] at most.
RLE_WALK_FN int owner(const int* s, int runs, int p) {
  int lo = 0, hi = runs;   // s[lo] <= p, and hi == runs or s[hi] > p
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (s[mid] <= p)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}

// run owns some position <= p and next == s[run + 1] -> the owner of p, `next` kept in step.  Ends without an end test:
// s[runs] is above every position.
RLE_WALK_FN int advance(const int* s, int run, int& next, int p) {
  while (next <= p) next = s[++run + 1];
  return run;
}

// elements that the pixel `element` (its offset in the output, low word) lies above a 16-byte boundary, for an output
// that begins at the address `out_low` (low word).  Only the low four bits matter, so arithmetic that wraps is exact.
RLE_WALK_FN int row_shift(uint32_t out_low, uint32_t element, uint32_t element_bytes) {
  return (int)(((out_low + element * element_bytes) & 15u) / element_bytes);
}

// a piece of `elements` elements of a shifted row that begins at shifted column u0 -> c0, the tile column of its first
// element, and whether every element is a pixel of the tile's `tw` columns: then the piece leaves as one 16-byte store,
// and its address is 16-byte aligned because u0 is a multiple of `elements`
RLE_WALK_FN bool whole_piece(int u0, int shift, int tw, int elements, int& c0) {
  c0 = u0 - shift;
  return c0 >= 0 && c0 + elements <= tw;
}

}  // namespace deva_rle
