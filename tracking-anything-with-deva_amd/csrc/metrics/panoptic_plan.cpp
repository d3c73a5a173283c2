// Argument checks and launch decision of the joint count (see panoptic_plan.h), and the library's host-only entry points.
#include "panoptic_plan.h"

namespace deva_metrics {

HOST_ARGS_DEFINE_ERROR_TEXT()
const char* last_error() { return g_err; }

int encoding_bytes(int encoding) {
  switch (encoding) {
    case DEVA_METRICS_RGB8: return 3;
    case DEVA_METRICS_I32: return 4;
    case DEVA_METRICS_I64: return 8;
    case DEVA_METRICS_INDEX16: return 2;
    default: return 0;
  }
}

int panoptic_plan(const char* what, int height, int width, int n_gt, int n_pred, deva_metrics_plan* plan) {
  DEVA_METRICS_REQUIRE(plan, "%s: null plan", what);
  DEVA_METRICS_REQUIRE(n_gt >= 0 && n_gt <= DEVA_METRICS_MAX_IDS, "%s: 0 to %d ground-truth ids (got %d)", what,
                       DEVA_METRICS_MAX_IDS, n_gt);
  DEVA_METRICS_REQUIRE(n_pred >= 0 && n_pred <= DEVA_METRICS_MAX_IDS, "%s: 0 to %d predicted ids (got %d)", what,
                       DEVA_METRICS_MAX_IDS, n_pred);
  DEVA_METRICS_REQUIRE(height > 0 && width > 0 && (int64_t)height * width <= kMaxPixels, "%s: bad plane size %d x %d", what,
                       height, width);
  const int64_t bins = (int64_t)(n_gt + 2) * (n_pred + 2);
  const int64_t tables = 4ll * (n_gt + n_pred);
  const int64_t strips = ((int64_t)height * width + DEVA_METRICS_STRIP - 1) / DEVA_METRICS_STRIP;
  const int64_t groups = (strips + kBlock - 1) / kBlock;
  plan->path = 4 * bins + tables <= DEVA_METRICS_LDS_LIMIT ? DEVA_METRICS_PATH_LDS : DEVA_METRICS_PATH_GLOBAL;
  plan->grid = (uint32_t)(groups < kMaxGrid ? groups : kMaxGrid);
  plan->block = kBlock;
  plan->lds_bytes = (uint32_t)(tables + (plan->path == DEVA_METRICS_PATH_LDS ? 4 * bins : 0));
  return 0;
}

int panoptic_counts_check(const void* gt, int gt_encoding, const void* gt_ids, int n_gt, const void* pred, int pred_encoding,
                          const void* pred_ids, int n_pred, const void* pred_lut, int channels, int height, int width,
                          const void* counts, deva_metrics_plan* plan) {
  const char* what = "deva_metrics_panoptic_counts";
  DEVA_METRICS_REQUIRE(gt_encoding == DEVA_METRICS_RGB8 || gt_encoding == DEVA_METRICS_I32,
                       "%s: the ground truth is RGB8 (0) or I32 (1) (got encoding %d)", what, gt_encoding);
  DEVA_METRICS_REQUIRE(pred_encoding >= DEVA_METRICS_RGB8 && pred_encoding <= DEVA_METRICS_INDEX16,
                       "%s: unknown encoding %d of the prediction", what, pred_encoding);
  deva_metrics_plan local;
  if (int rc = panoptic_plan(what, height, width, n_gt, n_pred, plan ? plan : &local)) return rc;
  const bool fast = pred_encoding == DEVA_METRICS_INDEX16;
  DEVA_METRICS_REQUIRE(gt && aligned(gt, 16), "%s: null or misaligned ground-truth plane", what);
  DEVA_METRICS_REQUIRE(pred && aligned(pred, 16), "%s: null or misaligned predicted plane", what);
  DEVA_METRICS_REQUIRE((gt_ids || n_gt == 0) && aligned(gt_ids, 4),
                       "%s: null or misaligned ground-truth id table", what);
  DEVA_METRICS_REQUIRE(fast || ((pred_ids || n_pred == 0) && aligned(pred_ids, 4)),
                       "%s: null or misaligned predicted id table", what);
  if (fast) {
    DEVA_METRICS_REQUIRE(channels >= 1 && channels <= 32767, "%s: 1 to 32767 channels (got %d)", what, channels);
    DEVA_METRICS_REQUIRE(pred_lut && aligned(pred_lut, 2), "%s: null or misaligned channel table", what);
  }
  DEVA_METRICS_REQUIRE(counts && aligned(counts, 4), "%s: null or misaligned counts", what);
  const int64_t pixels = (int64_t)height * width;
  const int64_t out_bytes = 4ll * (n_gt + 2) * (n_pred + 2);
  const bool clash = overlaps(counts, out_bytes, gt, pixels * encoding_bytes(gt_encoding)) ||
                     overlaps(counts, out_bytes, pred, pixels * encoding_bytes(pred_encoding)) ||
                     overlaps(counts, out_bytes, gt_ids, 4ll * n_gt) ||
                     (!fast && overlaps(counts, out_bytes, pred_ids, 4ll * n_pred)) ||
                     (fast && overlaps(counts, out_bytes, pred_lut, 2ll * channels));
  DEVA_METRICS_REQUIRE(!clash, "%s: counts overlaps an input", what);
  return 0;
}

}  // namespace deva_metrics

extern "C" int deva_metrics_version(void) { return DEVA_METRICS_ABI_VERSION; }
extern "C" const char* deva_metrics_last_error(void) { return deva_metrics::last_error(); }
extern "C" int deva_metrics_panoptic_plan(int height, int width, int n_gt, int n_pred, deva_metrics_plan* plan) {
  return deva_metrics::panoptic_plan("deva_metrics_panoptic_plan", height, width, n_gt, n_pred, plan);
}
