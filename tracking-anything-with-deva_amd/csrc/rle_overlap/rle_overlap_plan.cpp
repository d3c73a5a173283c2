// The argument checks, rule O2 and the launch decision of the run-length overlap (see rle_overlap_plan.h), and the
// library's host-only entry points.
#include "rle_overlap_plan.h"

namespace deva_overlap {

HOST_ARGS_DEFINE_ERROR_TEXT()
const char* last_error() { return g_err; }

static int64_t capped(int64_t groups) { return groups < kMaxGrid ? groups : kMaxGrid; }

static int check_masks(const char* what, const char* side, int n) {
  DEVA_OVERLAP_REQUIRE(n >= 0 && n <= DEVA_OVERLAP_MAX_MASKS, "%s: %s: 0 to %d masks a call (got %d)", what, side, DEVA_OVERLAP_MAX_MASKS, n);
  return 0;
}

static int check_words(const char* what, const char* side, int64_t words, int n) {
  DEVA_OVERLAP_REQUIRE(words >= (int64_t)n + 1 && words <= DEVA_OVERLAP_MAX_WORDS, "%s: %s: a run array of %lld to %d words (got %lld)", what,
                       side, (long long)n + 1, DEVA_OVERLAP_MAX_WORDS, (long long)words);
  return 0;
}

int pair_plan(const char* what, int d, int g, int64_t words_g, struct deva_overlap_plan* plan) {
  DEVA_OVERLAP_REQUIRE(plan, "%s: null plan", what);
  if (int rc = check_masks(what, "dt", d)) return rc;
  if (int rc = check_masks(what, "gt", g)) return rc;
  if (int rc = check_words(what, "gt", words_g, g)) return rc;
  const int64_t d_chunks = ((int64_t)d + kChunkD - 1) / kChunkD;
  plan->scan_grid = (uint32_t)capped((int64_t)d + g);
  plan->pair_grid = (uint32_t)capped(d_chunks * g);
  plan->d_chunks = (int32_t)d_chunks;
  plan->lds_bytes = kLdsBytes;
  plan->scratch_bytes = 4 * (words_g - g - 1);   // one int32 per start of the ground-truth side
  return 0;
}

int runs_check(const char* what, int side, const int32_t* runs, int64_t words, int n, int height, int width) {
  const char* name = side_name(side);
  DEVA_OVERLAP_REQUIRE(side == DEVA_OVERLAP_DT || side == DEVA_OVERLAP_GT, "%s: side must be DEVA_OVERLAP_DT or DEVA_OVERLAP_GT (got %d)", what,
                       side);
  DEVA_OVERLAP_REQUIRE(height > 0 && width > 0 && (int64_t)height * width <= kMaxPixels, "%s: bad size %d x %d (1 <= H * W < 2^31)", what,
                       height, width);
  if (int rc = check_masks(what, name, n)) return rc;
  DEVA_OVERLAP_REQUIRE(runs, "%s: %s: null run array", what, name);
  if (int rc = check_words(what, name, words, n)) return rc;
  const int32_t* first = runs;
  const int32_t* starts = runs + n + 1;
  const int64_t held = words - n - 1, total = (int64_t)height * width;
  DEVA_OVERLAP_REQUIRE(first[0] == 0, "%s: %s: first[0] must be 0 (got %d)", what, name, first[0]);
  for (int k = 0; k < n; ++k) {   // the index first: nothing below reads outside the array
    DEVA_OVERLAP_REQUIRE(first[k + 1] >= first[k] && first[k + 1] <= held, "%s: %s mask %d: its starts end at word %d of %lld", what, name, k,
                         first[k + 1], (long long)held);
    DEVA_OVERLAP_REQUIRE(first[k + 1] - first[k] >= 2, "%s: %s mask %d: no counts (the counts of a mask sum to H * W = %lld)", what, name, k,
                         (long long)total);
  }
  DEVA_OVERLAP_REQUIRE(first[n] == held, "%s: %s: the run array holds %lld starts, the masks take %d", what, name, (long long)held, first[n]);
  for (int k = 0; k < n; ++k) {
    const int32_t* s = starts + first[k];
    const int runs_k = first[k + 1] - first[k] - 1;
    DEVA_OVERLAP_REQUIRE(s[0] == 0, "%s: %s mask %d: the first start must be 0 (got %d)", what, name, k, s[0]);
    for (int r = 0; r < runs_k; ++r)
      DEVA_OVERLAP_REQUIRE(s[r + 1] >= s[r], "%s: %s mask %d: count %d is negative (%lld)", what, name, k, r, (long long)s[r + 1] - s[r]);
    DEVA_OVERLAP_REQUIRE(s[runs_k] == total, "%s: %s mask %d: the counts sum to %d, H * W is %lld", what, name, k, s[runs_k], (long long)total);
  }
  return 0;
}

int intersections_check(const int32_t* dt_host, const int32_t* dt_device, int64_t dt_words, int d, const int32_t* gt_host,
                        const int32_t* gt_device, int64_t gt_words, int g, int height, int width, const int32_t* box_d,
                        const int32_t* box_g, const void* scratch, int64_t scratch_bytes, const uint32_t* inter, int64_t pitch,
                        const uint32_t* area_d, const uint32_t* area_g, struct deva_overlap_plan* plan) {
  const char* what = "deva_overlap_intersections";
  struct deva_overlap_plan local;
  if (!plan) plan = &local;
  DEVA_OVERLAP_REQUIRE(height > 0 && width > 0 && (int64_t)height * width <= kMaxPixels, "%s: bad size %d x %d (1 <= H * W < 2^31)", what,
                       height, width);
  if (int rc = check_masks(what, "dt", d)) return rc;
  if (int rc = check_masks(what, "gt", g)) return rc;
  if (d == 0 || g == 0) return 0;   // O7
  if (int rc = runs_check(what, DEVA_OVERLAP_DT, dt_host, dt_words, d, height, width)) return rc;
  if (int rc = runs_check(what, DEVA_OVERLAP_GT, gt_host, gt_words, g, height, width)) return rc;
  if (int rc = pair_plan(what, d, g, gt_words, plan)) return rc;
  DEVA_OVERLAP_REQUIRE(dt_device && aligned(dt_device, 4), "%s: dt: null or misaligned run array on the device", what);
  DEVA_OVERLAP_REQUIRE(gt_device && aligned(gt_device, 4), "%s: gt: null or misaligned run array on the device", what);
  DEVA_OVERLAP_REQUIRE((box_d == nullptr) == (box_g == nullptr), "%s: boxes: give both sides' or neither", what);
  DEVA_OVERLAP_REQUIRE(aligned(box_d, 4) && aligned(box_g, 4), "%s: boxes: misaligned", what);
  DEVA_OVERLAP_REQUIRE(scratch && aligned(scratch, 4), "%s: scratch: null or not 4-byte aligned", what);
  DEVA_OVERLAP_REQUIRE(scratch_bytes >= plan->scratch_bytes, "%s: scratch_bytes: %lld given, deva_overlap_scratch asks for %lld", what,
                       (long long)scratch_bytes, (long long)plan->scratch_bytes);
  DEVA_OVERLAP_REQUIRE(inter && aligned(inter, 4), "%s: inter: null or misaligned", what);
  DEVA_OVERLAP_REQUIRE(pitch >= g && pitch <= (1ll << 40), "%s: pitch: %lld elements for rows of %d", what, (long long)pitch, g);
  DEVA_OVERLAP_REQUIRE(area_d && aligned(area_d, 4), "%s: area_d: null or misaligned", what);
  DEVA_OVERLAP_REQUIRE(area_g && aligned(area_g, 4), "%s: area_g: null or misaligned", what);
  const struct { const char* name; const void* p; int64_t bytes; } outs[] = {{"scratch", scratch, plan->scratch_bytes},
                                                                             {"inter", inter, 4 * ((d - 1) * pitch + g)},
                                                                             {"area_d", area_d, 4ll * d},
                                                                             {"area_g", area_g, 4ll * g}};
  const struct { const char* name; const void* p; int64_t bytes; } ins[] = {
      {"the dt run array", dt_device, 4 * dt_words}, {"the gt run array", gt_device, 4 * gt_words}, {"box_d", box_d, 16ll * d}, {"box_g", box_g, 16ll * g}};
  for (const auto& o : outs) {
    for (const auto& i : ins) DEVA_OVERLAP_REQUIRE(!overlaps(o.p, o.bytes, i.p, i.bytes), "%s: %s overlaps %s", what, o.name, i.name);
    for (const auto& q : outs)
      DEVA_OVERLAP_REQUIRE(&o == &q || !overlaps(o.p, o.bytes, q.p, q.bytes), "%s: %s overlaps %s", what, o.name, q.name);
  }
  return 0;
}

}  // namespace deva_overlap

extern "C" int deva_overlap_version(void) { return DEVA_OVERLAP_ABI_VERSION; }
extern "C" const char* deva_overlap_last_error(void) { return deva_overlap::last_error(); }
extern "C" int deva_overlap_limits(struct deva_overlap_limits* limits) {
  DEVA_OVERLAP_REQUIRE(limits, "deva_overlap_limits: null limits");
  limits->max_masks = DEVA_OVERLAP_MAX_MASKS;
  limits->max_words = DEVA_OVERLAP_MAX_WORDS;
  limits->block = deva_overlap::kBlock;
  limits->d_chunk = DEVA_OVERLAP_D_CHUNK;
  limits->lds_runs = DEVA_OVERLAP_LDS_RUNS;
  limits->scan_chunk = DEVA_OVERLAP_SCAN_CHUNK;
  return 0;
}
extern "C" int deva_overlap_plan(int d, int g, int64_t words_g, struct deva_overlap_plan* plan) {
  return deva_overlap::pair_plan("deva_overlap_plan", d, g, words_g, plan);
}
extern "C" int64_t deva_overlap_scratch(int64_t words_g, int g) {
  struct deva_overlap_plan plan;
  return deva_overlap::pair_plan("deva_overlap_scratch", 0, g, words_g, &plan) ? -1 : plan.scratch_bytes;
}
extern "C" int deva_overlap_check(const int32_t* runs, int64_t words, int n, int height, int width, int side) {
  return deva_overlap::runs_check("deva_overlap_check", side, runs, words, n, height, width);
}
