// csrc/rle_overlap/rle_overlap_plan.cpp and the host half of csrc/rle_overlap/overlap_walk.h under the host sanitizers,
// in a program of its own (tests/test_rle_overlap_cpu.py builds it with -fsanitize=address,undefined and runs it; nothing
// is loaded into Python and no GPU is involved).
//
// It sweeps the launch decision over mask numbers and word counts around the limits, sends every argument check of
// deva_overlap_intersections and rule O2 through their refusals (run arrays of exactly their size, made-up device
// addresses), and runs the pair pass as the kernel does, lane by lane with `lane_pairs` on random masks with zero counts,
// for several lane counts, against an overlap counted pixel by pixel.  Prints "<checks> <refused> <failures>".
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "overlap_walk.h"
#include "rle_overlap_plan.h"

using namespace deva_overlap;

static long long g_checks = 0, g_refused = 0, g_failures = 0;

#define EXPECT(cond)                                                   \
  do {                                                                 \
    ++g_checks;                                                        \
    if (!(cond)) {                                                     \
      ++g_failures;                                                    \
      fprintf(stderr, "line %d: %s [%s]\n", __LINE__, #cond, last_error()); \
    }                                                                  \
  } while (0)

static bool refused(int rc, const char* word) {
  ++g_refused;
  return rc == 2 && strstr(last_error(), word) != nullptr;
}

static uint64_t g_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() {
  g_state ^= g_state << 13;
  g_state ^= g_state >> 7;
  g_state ^= g_state << 17;
  return (uint32_t)(g_state >> 16);
}

static void sweep_plans() {
  const int masks[] = {0, 1, 2, 7, 8, 9, 63, 64, 65, 8191, 8192, 8193, 65535, 65536, 65537};
  const int64_t extra[] = {0, 1, 2, 4096, 1 << 20, (int64_t)DEVA_OVERLAP_MAX_WORDS};
  for (int d : masks)
    for (int g : masks)
      for (int64_t e : extra) {
        const int64_t words = (int64_t)g + 1 + e;
        struct deva_overlap_plan p;
        memset(&p, 0x5a, sizeof(p));
        const int rc = pair_plan("sweep", d, g, words, &p);
        if (d > DEVA_OVERLAP_MAX_MASKS || g > DEVA_OVERLAP_MAX_MASKS) {
          EXPECT(refused(rc, "masks a call"));
          continue;
        }
        if (words > DEVA_OVERLAP_MAX_WORDS) {
          EXPECT(refused(rc, "a run array of"));
          EXPECT(deva_overlap_scratch(words, g) == -1);
          continue;
        }
        EXPECT(rc == 0);
        const int64_t chunks = ((int64_t)d + kChunkD - 1) / kChunkD;
        EXPECT(p.d_chunks == chunks && p.scratch_bytes == 4 * e && p.lds_bytes == kLdsBytes && kLdsBytes <= 16 * 1024 + 64);
        EXPECT(p.scan_grid == (uint32_t)((int64_t)d + g < kMaxGrid ? d + g : kMaxGrid));
        EXPECT(p.pair_grid == (uint32_t)(chunks * g < kMaxGrid ? chunks * g : kMaxGrid));
        EXPECT(deva_overlap_scratch(words, g) == 4 * e);
      }
  struct deva_overlap_plan p;
  EXPECT(refused(pair_plan("sweep", 1, 1, 1, &p), "a run array of"));
  EXPECT(refused(pair_plan("sweep", 1, 1, 4, nullptr), "null plan"));
  EXPECT(refused(pair_plan("sweep", -1, 1, 4, &p), "dt: 0 to"));
  EXPECT(refused(pair_plan("sweep", 1, -1, 4, &p), "gt: 0 to"));
}

// a side of n masks over `total` positions: first[0 .. n], then the starts; exactly its size
static std::vector<int32_t> run_array(const std::vector<std::vector<int32_t>>& starts) {
  const int n = (int)starts.size();
  std::vector<int32_t> out(n + 1, 0);
  for (int k = 0; k < n; ++k) out[k + 1] = out[k] + (int32_t)starts[k].size();
  for (const auto& s : starts) out.insert(out.end(), s.begin(), s.end());
  return out;
}

static std::vector<int32_t> random_starts(int total, int kind) {
  std::vector<int32_t> s = {0};
  if (kind == 0) {                       // empty
  } else if (kind == 1) {                // full
    s.push_back(0);
  } else if (kind == 2) {                // every count 1
    for (int p = 1; p < total; ++p) s.push_back(p);
  } else {
    const int step = kind == 3 ? 3 : (kind == 4 ? total / 3 + 2 : 17);
    int p = 0;
    while (p < total) {
      const uint32_t r = rnd();
      const int c = (r & 7) == 0 ? 0 : (int)(r % (uint32_t)step);   // zero counts anywhere, several in a row too
      p = p + c < total ? p + c : total;
      if (p < total) s.push_back(p);
    }
    if (rnd() & 1) s.push_back(total);   // a zero count last
  }
  s.push_back(total);
  return s;
}

static std::vector<uint8_t> pixels(const std::vector<int32_t>& s, int total) {
  std::vector<uint8_t> out(total, 0);
  for (size_t k = 1; k + 1 < s.size(); k += 2)
    for (int p = s[k]; p < s[k + 1]; ++p) out[p] = 1;
  return out;
}

static std::vector<int32_t> ones_before(const std::vector<int32_t>& s) {
  std::vector<int32_t> out(s.size(), 0);
  for (size_t k = 0; k + 1 < s.size(); ++k) out[k + 1] = out[k] + ((k & 1) ? s[k + 1] - s[k] : 0);
  return out;
}

static void sweep_walk() {
  const int totals[] = {1, 2, 4, 9, 64, 257, 1500};
  const int lane_counts[] = {1, 3, 64, 256};
  for (int total : totals)
    for (int round = 0; round < 6; ++round) {
      const int d = 1 + (int)(rnd() % 11), g = 1 + (int)(rnd() % 4);
      std::vector<std::vector<int32_t>> sd, sg;
      for (int k = 0; k < d; ++k) sd.push_back(random_starts(total, (int)(rnd() % 6)));
      for (int k = 0; k < g; ++k) sg.push_back(random_starts(total, (int)(rnd() % 6)));
      const std::vector<int32_t> dt = run_array(sd), gt = run_array(sg);
      EXPECT(runs_check("walk", DEVA_OVERLAP_DT, dt.data(), (int64_t)dt.size(), d, 1, total) == 0);
      EXPECT(runs_check("walk", DEVA_OVERLAP_GT, gt.data(), (int64_t)gt.size(), g, total, 1) == 0);
      const int32_t* starts_d = dt.data() + d + 1;
      for (int j = 0; j < g; ++j) {
        const std::vector<int32_t> before = ones_before(sg[j]);   // exactly rg + 1 words each: a read past them is caught
        const std::vector<uint8_t> pg = pixels(sg[j], total);
        const int rg = (int)sg[j].size() - 1;
        for (int lanes : lane_counts)
          for (int d0 = 0; d0 < d; d0 += kChunkD) {
            const int nd = d - d0 < kChunkD ? d - d0 : kChunkD;
            std::vector<uint32_t> sums(nd, 0);
            std::vector<int> live(nd, 1), calls(nd * lanes, 0);
            if (round & 1) live[rnd() % nd] = 0;                  // a pair the box test dropped: 0, its runs unread
            for (int lane = 0; lane < lanes; ++lane)
              lane_pairs(dt.data() + d0, starts_d, nd, live, sg[j], before, rg, lane, lanes, [&](int dd, uint32_t v) {
                sums[dd] += v;
                ++calls[dd * lanes + lane];
              });
            for (int dd = 0; dd < nd; ++dd) {
              const std::vector<uint8_t> pd = pixels(sd[d0 + dd], total);
              uint32_t want = 0;
              for (int p = 0; p < total; ++p) want += pd[p] & pg[p];
              EXPECT(sums[dd] == (live[dd] ? want : 0u));
              for (int lane = 0; lane < lanes; ++lane) EXPECT(calls[dd * lanes + lane] <= 1);
            }
          }
      }
    }
  // the walk's two regimes: a 2-run mask against one of many runs, in both orders (steps, then the search of the rest)
  const int total = 4 * (kWalkSteps + 40);
  std::vector<std::vector<int32_t>> few = {{0, total / 2, total}}, many = {random_starts(total, 2)};
  for (int order = 0; order < 2; ++order) {
    const auto& sd = order ? many : few;
    const auto& sg = order ? few : many;
    const std::vector<int32_t> dt = run_array(sd), before = ones_before(sg[0]);
    uint32_t sum = 0;
    const std::vector<int> live = {1};
    for (int lane = 0; lane < 4; ++lane)
      lane_pairs(dt.data(), dt.data() + 2, 1, live, sg[0], before, (int)sg[0].size() - 1, lane, 4, [&](int, uint32_t v) { sum += v; });
    EXPECT(sum == (uint32_t)(total / 4));
  }
  const int32_t a[4] = {2, 3, 5, 7}, b[4] = {5, 7, 9, 9}, c[4] = {6, 0, 9, 9}, none[4] = {-1, -1, -1, -1};
  EXPECT(boxes_meet(a, b) && boxes_meet(b, a) && !boxes_meet(a, c) && !boxes_meet(c, a) && !boxes_meet(a, none) && !boxes_meet(none, a));
}

static void sweep_refusals() {
  const std::vector<int32_t> ok = {0, 3, 5, 0, 2, 6, 0, 6};   // two masks of 2 x 3: [2, 4] and [6]
  const int32_t* dev = reinterpret_cast<const int32_t*>(1ll << 40);
  auto at = [](int k) { return reinterpret_cast<uint32_t*>((1ll << 41) + ((int64_t)k << 30)); };
  auto call = [&](const std::vector<int32_t>& dt, const std::vector<int32_t>& gt, int d, int g, int h, int w, const int32_t* dd,
                  const int32_t* gd, const int32_t* bd, const int32_t* bg, void* scratch, int64_t bytes, uint32_t* inter, int64_t pitch,
                  uint32_t* ad, uint32_t* ag) {
    return intersections_check(dt.data(), dd, (int64_t)dt.size(), d, gt.data(), gd, (int64_t)gt.size(), g, h, w, bd, bg, scratch, bytes, inter,
                               pitch, ad, ag, nullptr);
  };
  const int32_t* gdev = dev + 64;
  EXPECT(call(ok, ok, 2, 2, 2, 3, dev, gdev, nullptr, nullptr, at(0), 20, at(1), 2, at(2), at(3)) == 0);
  EXPECT(call(ok, ok, 0, 2, 2, 3, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, 0, nullptr, nullptr) == 0);   // O7
  EXPECT(call(ok, ok, 2, 0, 2, 3, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, 0, nullptr, nullptr) == 0);
  EXPECT(refused(call(ok, ok, 2, 2, 0, 3, dev, gdev, nullptr, nullptr, at(0), 20, at(1), 2, at(2), at(3)), "bad size 0 x 3"));
  EXPECT(refused(call(ok, ok, 2, 2, 46341, 46341, dev, gdev, nullptr, nullptr, at(0), 20, at(1), 2, at(2), at(3)), "bad size"));
  EXPECT(refused(call(ok, ok, -1, 2, 2, 3, dev, gdev, nullptr, nullptr, at(0), 20, at(1), 2, at(2), at(3)), "dt: 0 to 65536 masks"));
  EXPECT(refused(call(ok, ok, 2, 65537, 2, 3, dev, gdev, nullptr, nullptr, at(0), 20, at(1), 2, at(2), at(3)), "gt: 0 to 65536 masks"));
  EXPECT(refused(call(ok, ok, 2, 2, 2, 3, nullptr, gdev, nullptr, nullptr, at(0), 20, at(1), 2, at(2), at(3)), "dt: null or misaligned"));
  EXPECT(refused(call(ok, ok, 2, 2, 2, 3, dev, reinterpret_cast<const int32_t*>((1ll << 40) + 2), nullptr, nullptr, at(0), 20, at(1), 2, at(2), at(3)),
                 "gt: null or misaligned"));
  EXPECT(refused(call(ok, ok, 2, 2, 2, 3, dev, gdev, dev + 32, nullptr, at(0), 20, at(1), 2, at(2), at(3)), "give both sides' or neither"));
  EXPECT(refused(call(ok, ok, 2, 2, 2, 3, dev, gdev, nullptr, nullptr, nullptr, 20, at(1), 2, at(2), at(3)), "scratch: null"));
  EXPECT(refused(call(ok, ok, 2, 2, 2, 3, dev, gdev, nullptr, nullptr, at(0), 19, at(1), 2, at(2), at(3)), "scratch_bytes: 19 given, deva_overlap_scratch asks for 20"));
  EXPECT(refused(call(ok, ok, 2, 2, 2, 3, dev, gdev, nullptr, nullptr, at(0), 20, nullptr, 2, at(2), at(3)), "inter: null"));
  EXPECT(refused(call(ok, ok, 2, 2, 2, 3, dev, gdev, nullptr, nullptr, at(0), 20, at(1), 1, at(2), at(3)), "pitch: 1 elements for rows of 2"));
  EXPECT(refused(call(ok, ok, 2, 2, 2, 3, dev, gdev, nullptr, nullptr, at(0), 20, at(1), 2, nullptr, at(3)), "area_d: null"));
  EXPECT(refused(call(ok, ok, 2, 2, 2, 3, dev, gdev, nullptr, nullptr, at(0), 20, at(1), 2, at(2), nullptr), "area_g: null"));
  EXPECT(refused(call(ok, ok, 2, 2, 2, 3, dev, gdev, nullptr, nullptr, at(0), 20, at(1), 2, at(2), at(2) + 1), "area_d overlaps area_g"));
  EXPECT(refused(call(ok, ok, 2, 2, 2, 3, dev, gdev, nullptr, nullptr, at(0), 20, at(1), 5, at(2), at(1) + 6), "inter overlaps area_g"));
  EXPECT(call(ok, ok, 2, 2, 2, 3, dev, gdev, nullptr, nullptr, at(0), 20, at(1), 5, at(2), at(1) + 7) == 0);   // right behind the block
  EXPECT(refused(call(ok, ok, 2, 2, 2, 3, dev, gdev, nullptr, nullptr, (void*)(dev + 7), 20, at(1), 2, at(2), at(3)), "scratch overlaps the dt run array"));
  EXPECT(refused(call(ok, ok, 2, 2, 2, 3, dev, gdev, dev + 32, dev + 48, at(0), 20, (uint32_t*)(dev + 55), 2, at(2), at(3)), "inter overlaps box_g"));
  // O2, on arrays of exactly their size
  struct Bad { std::vector<int32_t> runs; const char* word; };
  const Bad bad[] = {{{1, 3, 5, 0, 2, 6, 0, 6}, "first[0] must be 0"},       {{0, 1, 5, 0, 2, 6, 0, 6}, "mask 0: no counts"},
                     {{0, 3, 9, 0, 2, 6, 0, 6}, "mask 1: its starts end"},   {{0, 3, 4, 0, 2, 6, 0, 6}, "mask 1: no counts"},
                     {{0, 3, 5, 1, 2, 6, 0, 6}, "mask 0: the first start"},  {{0, 3, 5, 0, 4, 3, 0, 6}, "mask 0: count 1 is negative (-1)"},
                     {{0, 3, 5, 0, 2, 5, 0, 6}, "mask 0: the counts sum to 5"}, {{0, 3, 5, 0, 2, 6, 0, 7}, "mask 1: the counts sum to 7"},
                     {{0, 3, 5, 0, 2, 6, 0, 6, 6}, "holds 6 starts, the masks take 5"}};
  for (const Bad& b : bad) {
    EXPECT(refused(runs_check("o2", DEVA_OVERLAP_GT, b.runs.data(), (int64_t)b.runs.size(), 2, 2, 3), b.word));
    EXPECT(strstr(last_error(), "gt") != nullptr);
    EXPECT(refused(call(b.runs, ok, 2, 2, 2, 3, dev, gdev, nullptr, nullptr, at(0), 20, at(1), 2, at(2), at(3)), b.word));
    EXPECT(strstr(last_error(), "dt") != nullptr);
    EXPECT(refused(call(ok, b.runs, 2, 2, 2, 3, dev, gdev, nullptr, nullptr, at(0), 24, at(1), 2, at(2), at(3)), b.word));
    EXPECT(strstr(last_error(), "gt") != nullptr);
  }
  EXPECT(refused(runs_check("o2", 2, ok.data(), 8, 2, 2, 3), "side must be"));
  EXPECT(refused(runs_check("o2", DEVA_OVERLAP_DT, nullptr, 8, 2, 2, 3), "null run array"));
  EXPECT(refused(runs_check("o2", DEVA_OVERLAP_DT, ok.data(), 2, 2, 2, 3), "a run array of 3 to"));
  const int32_t none[1] = {0};
  EXPECT(runs_check("o2", DEVA_OVERLAP_DT, none, 1, 0, 2, 3) == 0);
  struct deva_overlap_limits limits;
  EXPECT(deva_overlap_limits(&limits) == 0 && limits.d_chunk == kChunkD && limits.lds_runs == kLdsRuns && limits.block == kBlock);
  EXPECT(refused(deva_overlap_limits(nullptr), "null limits"));
  EXPECT(deva_overlap_version() == DEVA_OVERLAP_ABI_VERSION);
}

int main() {
  sweep_plans();
  sweep_walk();
  sweep_refusals();
  printf("%lld %lld %lld\n", g_checks, g_refused, g_failures);
  return g_failures ? 1 : 0;
}
