// Stand-alone host program for tests/test_regions_cpu.py: the HIP-free side of the region kernels under the host
// sanitizers.  Two parts:
//  1. csrc/regions/region_plan.cpp (every argument check of deva_regions_label / deva_regions_clean, the scratch layout
//     and the launch decision behind deva_regions_plan) walked over the product of its boundary values.  Addresses are
//     made up: nothing is dereferenced.
//  2. csrc/regions/region_union.h, the one merging loop of the kernels, on host threads that unite the edges of awkward
//     planes in a scrambled order and concurrently, against a sequential flood fill: the loop ends and every pixel's root
//     is its component's first pixel.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <atomic>
#include <initializer_list>
#include <thread>
#include <vector>

#include "deva_regions.h"
#include "region_plan.h"
#include "region_union.h"

static long g_calls = 0, g_refused = 0, g_failed = 0;

static void fail(const char* what, long a, long b, long c, long d) {
  ++g_failed;
  fprintf(stderr, "FAIL %s: %ld %ld %ld %ld (%s)\n", what, a, b, c, d, deva_regions_last_error());
}

static void tally(int e, bool want, const char* entry, const char* what, long a, long b, long c, long d) {
  ++g_calls;
  if (e != 0) ++g_refused;
  if ((e == 0) != want) fail(what, a, b, c, d);
  if (e != 0 && (e != 2 || !strstr(deva_regions_last_error(), entry))) fail("refusal text", a, b, c, d);
  deva_regions::set_error("%s", "");
}

// ------------------------------------------------------------------------------------------ the union loop on threads
struct HostMem {
  static int load(const int* p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }
  static int fetch_min(int* p, int v) {
    int old = __atomic_load_n(p, __ATOMIC_RELAXED);
    while (old > v && !__atomic_compare_exchange_n(p, &old, v, true, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {
    }
    return old;
  }
};

static void union_case(const char* name, int h, int w, const std::vector<uint8_t>& kind, int threads) {
  using namespace deva_regions;
  std::vector<int> L(h * w);
  for (int i = 0; i < h * w; ++i) L[i] = kind[i] ? i + 1 : 0;
  std::vector<std::pair<int, int>> edges;
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) {
      if (!kind[y * w + x]) continue;
      const int dy[4] = {0, -1, -1, -1}, dx[4] = {-1, -1, 0, 1};
      for (int k = 0; k < 4; ++k) {
        const int yy = y + dy[k], xx = x + dx[k];
        if (yy >= 0 && xx >= 0 && xx < w && kind[yy * w + xx]) edges.push_back({y * w + x, yy * w + xx});
      }
    }
  // a fixed scramble, so that late and early merges interleave; the threads take the edges round robin
  uint64_t s = 0x9e3779b97f4a7c15ull;
  for (size_t i = edges.size(); i > 1; --i) {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    std::swap(edges[i - 1], edges[(s >> 33) % i]);
  }
  std::vector<std::thread> pool;
  for (int t = 0; t < threads; ++t)
    pool.emplace_back([&, t] {
      for (size_t i = t; i < edges.size(); i += threads) unite<HostMem>(L.data(), edges[i].first, edges[i].second);
    });
  for (auto& th : pool) th.join();
  // the sequential answer: flood fill in row-major order, so a component is named by its first pixel
  std::vector<int> want(h * w, -1), stack;
  for (int i = 0; i < h * w; ++i) {
    if (!kind[i] || want[i] >= 0) continue;
    want[i] = i;
    stack.push_back(i);
    while (!stack.empty()) {
      const int p = stack.back(), y = p / w, x = p % w;
      stack.pop_back();
      for (int yy = y - 1; yy <= y + 1; ++yy)
        for (int xx = x - 1; xx <= x + 1; ++xx)
          if (yy >= 0 && yy < h && xx >= 0 && xx < w && kind[yy * w + xx] && want[yy * w + xx] < 0) {
            want[yy * w + xx] = i;
            stack.push_back(yy * w + xx);
          }
    }
  }
  long bad = 0;
  for (int i = 0; i < h * w; ++i) {
    ++g_calls;
    if (kind[i] ? find_root<HostMem>(L.data(), i) != want[i] : L[i] != 0) ++bad;
  }
  if (bad) fail(name, h, w, threads, bad);
}

static void union_cases() {
  const int h = 37, w = 67;
  std::vector<uint8_t> serpentine(h * w, 0), comb(h * w, 0), checker(h * w, 0), diagonals(h * w, 0), full(h * w, 1), empty(h * w, 0);
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) {
      const int i = y * w + x;
      serpentine[i] = y % 2 == 0 || x == ((y / 2) % 2 == 0 ? w - 1 : 0);
      comb[i] = x % 2 == 0 || y == h - 1;
      checker[i] = (x + y) % 2 == 0;
      diagonals[i] = (x + y) % 3 == 0;
    }
  for (int threads : {1, 4, 16}) {
    union_case("serpentine", h, w, serpentine, threads);
    union_case("comb", h, w, comb, threads);
    union_case("checkerboard", h, w, checker, threads);
    union_case("diagonals", h, w, diagonals, threads);
    union_case("full", h, w, full, threads);
    union_case("empty", h, w, empty, threads);
  }
}

// ------------------------------------------------------------------------------------------ the plan and the checks
int main() {
  using namespace deva_regions;
  const int sides[] = {-2147483647 - 1, -1, 0, 1, 2, 31, 32, 33, 63, 64, 65, 480, 854, 1920, 32767, 32768, 32769, 46341, 1 << 30,
                       (1 << 30) + 1, 2147483647};
  const int counts[] = {-2147483647 - 1, -1, 0, 1, 2, 5, 64, 65536, 65537, 2147483647};
  const auto at = [](int64_t off) { return reinterpret_cast<const void*>((uintptr_t(1) << 50) + off); };
  const int64_t G = int64_t(1) << 47;
  const void *PL = at(0), *OUT = at(G), *SCR = at(2 * G);

  for (int h : sides)
    for (int w : sides)
      for (int n : counts) {
        const bool ok = h > 0 && w > 0 && (int64_t)h * w <= kMaxPixels && n >= 0 && n <= DEVA_REGIONS_MAX_PLANES;
        int64_t bytes = -1;
        tally(deva_regions_scratch_bytes(h, w, n, &bytes), ok, "deva_regions_scratch_bytes", "scratch", h, w, n, 0);
        if (!ok) {
          struct deva_regions_plan plan;
          tally(deva_regions_plan(h, w, n, 1, &plan), false, "deva_regions_plan", "plan of bad sizes", h, w, n, 0);
          tally(label_check(PL, n, h, w, OUT, nullptr), false, "deva_regions_label", "label of bad sizes", h, w, n, 0);
          tally(clean_check(PL, n, h, w, 5, OUT, SCR, int64_t(1) << 46, nullptr), false, "deva_regions_clean", "clean of bad sizes", h, w, n, 0);
          continue;
        }
        const int64_t pixels = (int64_t)h * w;
        const PlaneLayout lay = plane_layout(pixels);
        if (lay.labels != 0 || lay.areas < 4 * pixels || lay.state < lay.areas + 4 * pixels || lay.bytes < lay.state + 4 * kStateWords ||
            lay.areas % 256 || lay.state % 256 || lay.bytes % 256 || bytes != n * lay.bytes)
          fail("layout", h, w, n, bytes);
        const int64_t budgets[] = {0, 1, lay.bytes - 1, lay.bytes, lay.bytes + 1, 2 * lay.bytes, 5 * lay.bytes - 1, n * lay.bytes, int64_t(1) << 62};
        for (int64_t budget : budgets) {
          struct deva_regions_plan plan;
          memset(&plan, 0xff, sizeof(plan));
          const bool fits = n == 0 || budget >= lay.bytes;
          const int e = deva_regions_plan(h, w, n, budget, &plan);
          tally(e, fits, "deva_regions_plan", "plan", h, w, n, budget);
          if (e != 0) {
            char need[32];
            snprintf(need, sizeof(need), "%lld are needed", (long long)lay.bytes);
            if (!strstr(deva_regions_last_error(), need)) {
              // (tally cleared the text: ask again)
              deva_regions_plan(h, w, n, budget, &plan);
              if (!strstr(deva_regions_last_error(), need)) fail("bytes needed in the text", h, w, n, budget);
            }
            continue;
          }
          const int64_t tx = ((int64_t)w + kTile - 1) / kTile, ty = ((int64_t)h + kTile - 1) / kTile;
          const int64_t per = plan.planes_per_pass, seam = (tx - 1) * h + (ty - 1) * w, chunks = (pixels + kBlock - 1) / kBlock;
          if (plan.tile != kTile || plan.block != kBlock || plan.tiles_x != tx || plan.tiles_y != ty || plan.plane_bytes != lay.bytes ||
              plan.reserved != 0)
            fail("plan fields", h, w, n, budget);
          if (n == 0 ? (per != 0 || plan.passes != 0 || plan.scratch_bytes != 0)
                     : (per < 1 || per > n || per * lay.bytes > budget || (per < n && (per + 1) * lay.bytes <= budget) ||
                        (int64_t)plan.passes * per < n || (int64_t)(plan.passes - 1) * per >= n || plan.scratch_bytes != per * lay.bytes))
            fail("passes", h, w, n, budget);
          // a workgroup per tile, a lane per seam pixel and per pixel up to the grid cap, never an idle workgroup
          const int64_t want_local = per * tx * ty, want_border = (per * seam + kBlock - 1) / kBlock, want_pixel = per * chunks;
          if (plan.local_grid != (want_local < kMaxGrid ? want_local : kMaxGrid) || plan.border_grid != (want_border < kMaxGrid ? want_border : kMaxGrid) ||
              plan.pixel_grid != (want_pixel < kMaxGrid ? want_pixel : kMaxGrid) || (n > 0 && (plan.local_grid < 1 || plan.pixel_grid < 1)))
            fail("grid", h, w, n, budget);
          if (n == 0 || budget > (int64_t(1) << 46)) continue;
          struct deva_regions_plan again;
          memset(&again, 0xff, sizeof(again));
          tally(clean_check(PL, n, h, w, 7, OUT, SCR, budget, &again), true, "deva_regions_clean", "check", h, w, n, budget);
          if (memcmp(&again, &plan, sizeof(plan)) != 0) fail("two plans", h, w, n, budget);
        }
      }
  tally(deva_regions_plan(8, 8, 1, 1 << 20, nullptr), false, "deva_regions_plan", "null plan", 0, 0, 0, 0);
  {
    struct deva_regions_plan plan;
    tally(deva_regions_plan(8, 8, 1, -1, &plan), false, "deva_regions_plan", "negative budget", 0, 0, 0, 0);
  }
  tally(deva_regions_scratch_bytes(8, 8, 1, nullptr), false, "deva_regions_scratch_bytes", "null bytes", 0, 0, 0, 0);

  // the pointers, one at a time on an otherwise good call: 5 planes of 29 x 53
  const int n = 5, h = 29, w = 53;
  const int64_t pixels = (int64_t)n * h * w, one = plane_layout(h * w).bytes;
  struct Case { const void *pl, *rec, *scr; int64_t bytes; int min_area; bool ok; };
  const Case good = {PL, OUT, SCR, 5 * one, 12, true};
  const auto with = [&](auto edit, bool ok) { Case c = good; edit(c); c.ok = ok; return c; };
  const Case cases[] = {
      good,
      with([&](Case& c) { c.pl = nullptr; }, false), with([&](Case& c) { c.pl = at(1); }, true),       // byte planes: any alignment
      with([&](Case& c) { c.rec = nullptr; }, false), with([&](Case& c) { c.rec = at(G + 2); }, false), with([&](Case& c) { c.rec = at(G + 4); }, true),
      with([&](Case& c) { c.scr = nullptr; }, false), with([&](Case& c) { c.scr = at(2 * G + 8); }, false), with([&](Case& c) { c.scr = at(2 * G + 16); }, true),
      with([&](Case& c) { c.bytes = one - 1; }, false), with([&](Case& c) { c.bytes = one; }, true), with([&](Case& c) { c.bytes = -1; }, false),
      with([&](Case& c) { c.bytes = 0; }, false), with([&](Case& c) { c.bytes = 2 * one; }, true),
      with([&](Case& c) { c.min_area = 0; }, false), with([&](Case& c) { c.min_area = -3; }, false), with([&](Case& c) { c.min_area = 1; }, true),
      with([&](Case& c) { c.min_area = 2147483647; }, true),
      // records is 4 * 8 * 5 = 160 bytes
      with([&](Case& c) { c.rec = at(pixels - 4); }, false), with([&](Case& c) { c.rec = at(pixels + 3 & ~3); }, true),
      with([&](Case& c) { c.pl = at(G + 159); }, false), with([&](Case& c) { c.pl = at(G + 160); }, true),
      with([&](Case& c) { c.rec = at(2 * G + 5 * one - 4); }, false), with([&](Case& c) { c.rec = at(2 * G + 5 * one); }, true),
      with([&](Case& c) { c.rec = at(2 * G + one); c.bytes = one; }, true),                             // beyond the part of the scratch that is used
      with([&](Case& c) { c.scr = at(pixels - 1 & ~15); }, false), with([&](Case& c) { c.scr = at(pixels + 15 & ~15); }, true),
      with([&](Case& c) { c.pl = at(2 * G + 5 * one - 1); }, false), with([&](Case& c) { c.pl = at(2 * G + 5 * one); }, true)};
  long k = 0;
  for (const Case& c : cases)
    tally(clean_check(c.pl, n, h, w, c.min_area, c.rec, c.scr, c.bytes, nullptr), c.ok, "deva_regions_clean", "single", k++, 0, 0, 0);
  // the labels: int32 [5][29][53]
  struct LCase { const void *pl, *out; bool ok; };
  const LCase lcases[] = {{PL, OUT, true}, {nullptr, OUT, false}, {PL, nullptr, false}, {PL, at(G + 2), false}, {at(3), OUT, true},
                          {PL, at(pixels - 4 & ~3), false}, {PL, at(pixels + 3 & ~3), true}, {at(G + 4 * pixels - 1), OUT, false},
                          {at(G + 4 * pixels), OUT, true}};
  k = 0;
  for (const LCase& c : lcases) tally(label_check(c.pl, n, h, w, c.out, nullptr), c.ok, "deva_regions_label", "label single", k++, 0, 0, 0);
  tally(label_check(nullptr, 0, h, w, nullptr, nullptr), true, "deva_regions_label", "no planes", 0, 0, 0, 0);
  tally(clean_check(nullptr, 0, h, w, 5, nullptr, nullptr, 0, nullptr), true, "deva_regions_clean", "no planes", 0, 0, 0, 0);
  tally(clean_check(nullptr, 0, h, w, 0, nullptr, nullptr, 0, nullptr), false, "deva_regions_clean", "no planes, no area", 0, 0, 0, 0);

  union_cases();
  printf("%ld checks (%ld refused), %ld failures\n", g_calls, g_refused, g_failed);
  return g_failed ? 1 : 0;
}
