// The arithmetic of rle_overlap.hip that is no HIP: the search for the run of g that owns a position, the bounded walk
// to the owner of a later one, the prefix count P_g, the box test, and a lane's share of the pair pass.  The kernel runs
// these on the device; tests/rle_overlap_plan_sanitize_main.cpp runs the same functions on the host, lane by lane on run
// arrays of exactly their size under the address sanitizer, against an overlap counted pixel by pixel.
#pragma once
#include <stdint.h>

namespace deva_overlap {

#if defined(__HIPCC__) || defined(__CUDACC__)
#define OVERLAP_WALK_FN __host__ __device__ __forceinline__
#else
#define OVERLAP_WALK_FN inline
#endif

constexpr int kWalkSteps = 8;   // starts of g a lane steps over one by one before it searches what is left

// s[0 .. runs]: the starts of a mask, s[0] = 0 <= p < s[runs] = H * W, never descending -> the last run whose start is
// <= p, searched in s[lo .. runs] where s[lo] <= p is known (O1: among runs that share a start the last one owns the
// pixel).  Reads s[lo + 1 .. runs - 1] at most.
template <typename Starts>
OVERLAP_WALK_FN int owner_from(const Starts& s, int lo, int runs, int p) {
  int hi = runs;   // s[lo] <= p, and s[hi] > p
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (s[mid] <= p)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}

// the cursor of a lane in g: run owns some position <= the next p asked for, next == s[run + 1]
struct Cursor {
  int run, next;
};

// -> the owner of p >= every p before, `next` kept in step.  s[runs] is above every position, so run + 1 <= runs.
template <typename Starts>
OVERLAP_WALK_FN void seek(const Starts& s, int runs, Cursor& c, int p) {
  int steps = 0;
  while (c.next <= p) {
    if (++steps > kWalkSteps) {
      c.run = owner_from(s, c.run + 1, runs, p);   // (s[run + 1] == next <= p)
      c.next = s[c.run + 1];
      return;
    }
    c.next = s[++c.run + 1];
  }
}

// ones of g at positions 0 .. p inclusive, for the owner `run` of p
template <typename Starts, typename Ones>
OVERLAP_WALK_FN int ones_through(const Starts& s, const Ones& before, int run, int p) {
  return before[run] + ((run & 1) ? p - s[run] + 1 : 0);
}

// O6: two inclusive boxes share a pixel (an empty mask's -1 box shares none with a box of a mask that has ones)
OVERLAP_WALK_FN bool boxes_meet(const int32_t* a, const int32_t* b) {
  return a[0] <= b[2] && b[0] <= a[2] && a[1] <= b[3] && b[1] <= a[3];
}

// One lane's share of a workgroup's pairs.  first_d: first[d0 .. d0 + nd] of the chunk's detections (indices into
// starts_d, which is the whole side's); live[0 .. nd): the box test; gs[0 .. rg], gob[0 .. rg]: the starts and
// ones_before of g.  The chunk's words [first_d[0], first_d[nd]) are cut into `lanes` contiguous stretches and the lane
// takes the one-runs that BEGIN in its stretch.  add(dd, sum) receives the lane's sum for detection d0 + dd, at most
// once per detection it touches.
template <typename Starts, typename Ones, typename Live, typename Add>
OVERLAP_WALK_FN void lane_pairs(const int32_t* first_d, const int32_t* starts_d, int nd, const Live& live, const Starts& gs, const Ones& gob,
                                int rg, int lane, int lanes, Add add) {
  const int w0 = first_d[0], w1 = first_d[nd];
  const int stretch = (w1 - w0 + lanes - 1) / lanes;
  int i = w0 + lane * stretch;                       // (w1 - w0 <= 2^26 and lane * stretch < w1 - w0 + lanes: no overflow)
  const int end = w1 - i < stretch ? w1 : i + stretch;
  if (i >= end) return;
  int dd = 0;
  while (first_d[dd + 1] <= i) ++dd;                 // (i < w1 = first_d[nd])
  int begin = first_d[dd], stop = first_d[dd + 1];   // the words of detection dd
  bool fresh = true;                                 // no cursor yet in g for this detection: positions begin anew
  Cursor c = {0, 0};
  uint32_t sum = 0;
  for (; i < end; ++i) {
    if (i >= stop) {
      if (sum) add(dd, sum);
      sum = 0;
      do {
        begin = first_d[++dd];
        stop = first_d[dd + 1];
      } while (i >= stop);
      fresh = true;
    }
    if (!((i - begin) & 1) || i + 1 >= stop || !live[dd]) continue;   // a zero-run, the last start, or boxes apart
    const int a = starts_d[i], b = starts_d[i + 1];
    if (a >= b) continue;                                             // a count of zero
    if (fresh) {
      c.run = owner_from(gs, 0, rg, a);
      c.next = gs[c.run + 1];
      fresh = false;
    } else {
      seek(gs, rg, c, a);
    }
    const int upto_a = ones_through(gs, gob, c.run, a) - (c.run & 1);  // ones at 0 .. a - 1
    seek(gs, rg, c, b - 1);
    sum += (uint32_t)(ones_through(gs, gob, c.run, b - 1) - upto_a);
  }
  if (sum) add(dd, sum);
}

}  // namespace deva_overlap
