// The argument checks and launch decision of the pair counts (see pair_plan.h), and the library's host-only entry points.
#include "pair_plan.h"

namespace deva_pair {

HOST_ARGS_DEFINE_ERROR_TEXT()
const char* last_error() { return g_err; }

int encoding_bytes(int encoding) {
  switch (encoding) {
    case DEVA_PAIR_U8: return 1;
    case DEVA_PAIR_I32: return 4;
    case DEVA_PAIR_I64: return 8;
    case DEVA_PAIR_INDEX16: return 2;
    default: return 0;
  }
}

static int check_size(const char* what, int height, int width) {
  DEVA_PAIR_REQUIRE(height > 0 && width > 0 && (int64_t)height * width <= kMaxPixels, "%s: bad plane size %d x %d", what, height,
                    width);
  return 0;
}

int pair_plan(const char* what, int height, int width, int n_gt, int n_pred, int radius, struct deva_pair_plan* plan) {
  DEVA_PAIR_REQUIRE(plan, "%s: null plan", what);
  DEVA_PAIR_REQUIRE(n_gt >= 1 && n_gt <= DEVA_PAIR_MAX_OBJECTS, "%s: 1 to %d ground-truth objects (got %d)", what,
                    DEVA_PAIR_MAX_OBJECTS, n_gt);
  DEVA_PAIR_REQUIRE(n_pred >= 1 && n_pred <= DEVA_PAIR_MAX_OBJECTS, "%s: 1 to %d proposals (got %d)", what, DEVA_PAIR_MAX_OBJECTS,
                    n_pred);
  DEVA_PAIR_REQUIRE(radius >= 0 && radius <= DEVA_PAIR_MAX_RADIUS, "%s: radius 0 to %d (got %d)", what, DEVA_PAIR_MAX_RADIUS, radius);
  if (int rc = check_size(what, height, width)) return rc;
  const int64_t pixels = (int64_t)height * width;
  const int64_t strips = (int64_t)height * (((int64_t)width + DEVA_PAIR_STRIP - 1) / DEVA_PAIR_STRIP);
  const int64_t label_groups = (strips + kBlock - 1) / kBlock;
  const int64_t chunks = (pixels + kWave - 1) / kWave;
  const int64_t match_groups = (chunks + kBlock / kWave - 1) / (kBlock / kWave);
  const uint32_t slots = (uint32_t)(n_gt + n_pred), cells = (uint32_t)n_gt * (uint32_t)n_pred;
  plan->label_grid = (uint32_t)(label_groups < kMaxGrid ? label_groups : kMaxGrid);
  plan->match_grid = (uint32_t)(match_groups < kMaxMatchGrid ? match_groups : kMaxMatchGrid);
  plan->block = kBlock;
  plan->label_lds_bytes = 4u * (2u * slots + cells);                         // both id tables, the areas, the joint counts
  plan->match_lds_bytes = 4u * (2u * DEVA_PAIR_MAX_OBJECTS + 2u * cells);    // boundary pixels per slot, the two match tables
  plan->inner_radius = radius < DEVA_PAIR_INNER_RADIUS ? radius : DEVA_PAIR_INNER_RADIUS;
  plan->wave_search = radius > DEVA_PAIR_INNER_RADIUS ? 1 : 0;
  plan->radius = radius;
  plan->scratch_bytes = pixels * kWordBytes;
  return 0;
}

int pair_counts_check(const void* gt, int gt_encoding, const void* gt_ids, int n_gt, const void* pred, int pred_encoding,
                      const void* pred_ids, int n_pred, const void* pred_lut, int channels, int height, int width, int radius,
                      const void* scratch, int64_t scratch_bytes, const void* singles, const void* pairs,
                      struct deva_pair_plan* plan) {
  const char* what = "deva_pair_counts";
  DEVA_PAIR_REQUIRE(gt_encoding == DEVA_PAIR_U8 || gt_encoding == DEVA_PAIR_I32,
                    "%s: the ground truth is U8 (0) or I32 (1); there is no binary form (got encoding %d)", what, gt_encoding);
  DEVA_PAIR_REQUIRE(pred_encoding >= DEVA_PAIR_U8 && pred_encoding <= DEVA_PAIR_INDEX16,
                    "%s: unknown encoding %d of the prediction (there is no binary form)", what, pred_encoding);
  struct deva_pair_plan local;
  if (!plan) plan = &local;
  if (int rc = pair_plan(what, height, width, n_gt, n_pred, radius, plan)) return rc;
  const bool fast = pred_encoding == DEVA_PAIR_INDEX16;
  DEVA_PAIR_REQUIRE(gt && aligned(gt, 16), "%s: null or misaligned ground-truth plane", what);
  DEVA_PAIR_REQUIRE(pred && aligned(pred, 16), "%s: null or misaligned predicted plane", what);
  DEVA_PAIR_REQUIRE(gt_ids && aligned(gt_ids, 4), "%s: null or misaligned ground-truth id table", what);
  if (fast) {
    DEVA_PAIR_REQUIRE(channels >= 1 && channels <= 32767, "%s: 1 to 32767 channels (got %d)", what, channels);
    DEVA_PAIR_REQUIRE(pred_lut && aligned(pred_lut, 2), "%s: null or misaligned channel table", what);
    pred_ids = nullptr;  // not read
  } else {
    DEVA_PAIR_REQUIRE(pred_ids && aligned(pred_ids, 4), "%s: null or misaligned proposal id table", what);
  }
  DEVA_PAIR_REQUIRE(scratch && aligned(scratch, 16), "%s: null or misaligned scratch", what);
  DEVA_PAIR_REQUIRE(scratch_bytes >= plan->scratch_bytes, "%s: the scratch holds %lld bytes, %lld are needed", what,
                    (long long)scratch_bytes, (long long)plan->scratch_bytes);
  DEVA_PAIR_REQUIRE(singles && aligned(singles, 4), "%s: null or misaligned singles", what);
  DEVA_PAIR_REQUIRE(pairs && aligned(pairs, 4), "%s: null or misaligned pairs", what);
  const int64_t pixels = (int64_t)height * width;
  const int64_t singles_bytes = 4ll * DEVA_PAIR_SINGLE_FIELDS * (n_gt + n_pred);
  const int64_t pairs_bytes = 4ll * DEVA_PAIR_FIELDS * n_gt * n_pred;
  const auto meets_input = [&](const void* p, int64_t bytes) {
    return overlaps(p, bytes, gt, pixels * encoding_bytes(gt_encoding)) ||
           overlaps(p, bytes, pred, pixels * encoding_bytes(pred_encoding)) || overlaps(p, bytes, gt_ids, 4ll * n_gt) ||
           overlaps(p, bytes, pred_ids, 4ll * n_pred) || (fast && overlaps(p, bytes, pred_lut, 2ll * channels));
  };
  DEVA_PAIR_REQUIRE(!meets_input(singles, singles_bytes) && !overlaps(singles, singles_bytes, scratch, plan->scratch_bytes),
                    "%s: singles overlaps an input", what);
  DEVA_PAIR_REQUIRE(!meets_input(pairs, pairs_bytes) && !overlaps(pairs, pairs_bytes, scratch, plan->scratch_bytes),
                    "%s: pairs overlaps an input", what);
  DEVA_PAIR_REQUIRE(!overlaps(singles, singles_bytes, pairs, pairs_bytes), "%s: singles and pairs overlap", what);
  DEVA_PAIR_REQUIRE(!meets_input(scratch, plan->scratch_bytes), "%s: the scratch overlaps an input", what);
  return 0;
}

}  // namespace deva_pair

extern "C" int deva_pair_version(void) { return DEVA_PAIR_ABI_VERSION; }
extern "C" const char* deva_pair_last_error(void) { return deva_pair::last_error(); }
extern "C" int deva_pair_scratch_bytes(int height, int width, int64_t* bytes) {
  const char* what = "deva_pair_scratch_bytes";
  DEVA_PAIR_REQUIRE(bytes, "%s: null bytes", what);
  struct deva_pair_plan plan;
  if (int rc = deva_pair::pair_plan(what, height, width, 1, 1, 0, &plan)) return rc;
  *bytes = plan.scratch_bytes;
  return 0;
}
extern "C" int deva_pair_plan(int height, int width, int n_gt, int n_pred, int radius, struct deva_pair_plan* plan) {
  return deva_pair::pair_plan("deva_pair_plan", height, width, n_gt, n_pred, radius, plan);
}
