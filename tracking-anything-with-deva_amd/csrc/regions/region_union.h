// Union-find on an int32 array, by atomic minimum: the one loop every merging stage of regions.hip runs, on LDS and on
// global memory.  No HIP in here: the memory operations come in as a policy, so tests/region_plan_sanitize_main.cpp runs
// the same loops on host threads.
//
// L[i] is 0 for a pixel of the other kind, else 1 + the position of a pixel of the same component at or before i:
// L[i] <= i + 1 always, and L[i] == i + 1 marks a root.  A value is only ever replaced by a smaller one (fetch_min).
//
// Termination.  find_root follows strictly decreasing positions, so it ends after at most i steps whatever other lanes
// do meanwhile, and whether or not a load is fresh: a stale value is a link the component once had.  An iteration of
// unite ends the loop (equal roots, or the minimum took effect on a slot that still was a root) or replaces the larger
// of (a, b) by the value the atomic returned, which is smaller: max(a, b) falls with every iteration, so there are
// at most max(a, b) of them.  No lane waits for a value another lane has yet to write.
//
// Correctness.  When fetch_min(L[a], b + 1) returns old != a + 1, slot a pointed at old - 1 before: whichever of the two
// links the slot keeps, the other pair -- (old - 1, b) -- still has to be united, and the loop goes on with exactly it.
#pragma once

namespace deva_regions {

#if defined(__HIPCC__) || defined(__CUDACC__)
#define REGION_UNION_FN __device__ __forceinline__
#else
#define REGION_UNION_FN inline
#endif

// Mem: static int load(const int* p); static int fetch_min(int* p, int v) -> the value before
template <class Mem>
REGION_UNION_FN int find_root(int* L, int i) {
  int v = Mem::load(L + i);
  while (v != i + 1) {
    i = v - 1;
    v = Mem::load(L + i);
  }
  return i;
}

template <class Mem>
REGION_UNION_FN void unite(int* L, int a, int b) {
  for (;;) {
    a = find_root<Mem>(L, a);
    b = find_root<Mem>(L, b);
    if (a == b) return;
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = Mem::fetch_min(L + a, b + 1) - 1;
    if (old == a) return;
    a = old;
  }
}

}  // namespace deva_regions
