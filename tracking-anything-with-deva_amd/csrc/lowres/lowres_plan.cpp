// The argument checks (rule L7), the launch decision and the host-only entry points of the low-resolution filter (see
// lowres_plan.h).
#include "lowres_plan.h"

#include <math.h>

namespace deva_lowres {

HOST_ARGS_DEFINE_ERROR_TEXT()
const char* last_error() { return g_err; }

int geometry_check(const char* what, const struct deva_lowres_geometry* g) {
  DEVA_LOWRES_REQUIRE(g, "%s: null geometry", what);
  DEVA_LOWRES_REQUIRE(g->low_h >= 1 && g->low_h <= DEVA_LOWRES_MAX_SIDE && g->low_w >= 1 && g->low_w <= DEVA_LOWRES_MAX_SIDE,
                      "%s: low-resolution planes of 1 to %d rows and columns (got %d x %d)", what, DEVA_LOWRES_MAX_SIDE, g->low_h,
                      g->low_w);
  DEVA_LOWRES_REQUIRE(g->model_size >= 1 && g->model_size <= DEVA_LOWRES_MAX_SIDE, "%s: a model_size of 1 to %d (got %d)", what,
                      DEVA_LOWRES_MAX_SIDE, g->model_size);
  DEVA_LOWRES_REQUIRE(g->in_h >= 1 && g->in_h <= g->model_size && g->in_w >= 1 && g->in_w <= g->model_size,
                      "%s: an input size within 1 .. model_size = %d (got %d x %d)", what, g->model_size, g->in_h, g->in_w);
  DEVA_LOWRES_REQUIRE(g->out_h >= 1 && g->out_w >= 1 && (int64_t)g->out_h * g->out_w <= DEVA_LOWRES_MAX_PIXELS,
                      "%s: bad output size %d x %d (1 <= OH * OW <= 2^30)", what, g->out_h, g->out_w);
  DEVA_LOWRES_REQUIRE(g->reserved == 0, "%s: geometry.reserved must be 0", what);
  return 0;
}

int lowres_plan(const char* what, const struct deva_lowres_geometry* g, struct deva_lowres_plan* plan) {
  if (int rc = geometry_check(what, g)) return rc;
  DEVA_LOWRES_REQUIRE(plan, "%s: null plan", what);
  const int oh = g->out_h, ow = g->out_w;
  // the rows below a band that the last 16-byte piece it owns may reach into
  const int reach = (kPiece - 1 + ow - 1) / ow;
  int rows = kBandPixels / ow;
  if (rows > DEVA_LOWRES_MAX_TILE_ROWS) rows = DEVA_LOWRES_MAX_TILE_ROWS;
  if (rows > oh) rows = oh;
  if (rows < 1) rows = 1;
  plan->path = DEVA_LOWRES_PATH_POINT;
  plan->tile_rows = rows;
  plan->mid_rows = plan->low_rows = plan->lds_bytes = 0;
  for (int r = rows; r >= 1; --r) {  // the tallest band whose patch fits the budget
    const int64_t cover = r + reach < oh ? r + reach : oh;
    const int mid_rows = rows_touched((int)cover, g->in_h, oh);
    const int low_rows = rows_touched(mid_rows, g->low_h, g->model_size);
    const int64_t lds = 4 * ((int64_t)mid_rows * g->in_w + (int64_t)low_rows * g->low_w);
    if (lds > DEVA_LOWRES_LDS_BUDGET) continue;
    if ((int64_t)mid_rows * g->in_w <= (int64_t)kMidPerOutMax * r * ow) {
      plan->path = DEVA_LOWRES_PATH_TILE;
      plan->tile_rows = r, plan->mid_rows = mid_rows, plan->low_rows = low_rows, plan->lds_bytes = (int32_t)lds;
    }
    break;
  }
  plan->tile_cols = ow;
  const int64_t cover = plan->tile_rows + reach < oh ? plan->tile_rows + reach : oh;
  plan->cover_rows = (int32_t)cover;
  plan->block = kBlock;
  plan->grid_x = (uint32_t)((oh + plan->tile_rows - 1) / plan->tile_rows);
  plan->grid_y_max = kMaxGridY;
  plan->out_values = (int64_t)plan->tile_rows * ow;
  plan->mid_values = plan->path == DEVA_LOWRES_PATH_TILE ? (int64_t)plan->mid_rows * g->in_w : 4 * plan->out_values;
  return 0;
}

int upsample_check(const void* low, int batch, const struct deva_lowres_geometry* g, const void* out, struct deva_lowres_plan* plan) {
  const char* what = "deva_lowres_upsample";
  if (int rc = lowres_plan(what, g, plan)) return rc;
  DEVA_LOWRES_REQUIRE(batch >= 0, "%s: negative batch (%d)", what, batch);
  if (batch == 0) return 0;  // (nothing is read or written)
  DEVA_LOWRES_REQUIRE(low && aligned(low, 4), "%s: null or misaligned low-resolution logits", what);
  DEVA_LOWRES_REQUIRE(out && aligned(out, 4), "%s: null or misaligned output", what);
  return 0;
}

int select_check(const void* low, const void* scores, int batch, int per_box, const struct deva_lowres_geometry* g,
                 double mask_threshold, const void* out, const void* chosen, struct deva_lowres_plan* plan) {
  const char* what = "deva_lowres_select";
  if (int rc = lowres_plan(what, g, plan)) return rc;
  DEVA_LOWRES_REQUIRE(batch >= 0, "%s: negative batch (%d)", what, batch);
  DEVA_LOWRES_REQUIRE(per_box >= 1 && per_box <= DEVA_LOWRES_MAX_PER_BOX, "%s: 1 to %d planes per box (got %d)", what,
                      DEVA_LOWRES_MAX_PER_BOX, per_box);
  DEVA_LOWRES_REQUIRE((int64_t)batch * per_box <= kMaxPlanes, "%s: at most 2^30 planes a call (got %d x %d)", what, batch, per_box);
  DEVA_LOWRES_REQUIRE(!isnan(mask_threshold), "%s: the mask threshold is not a number", what);
  DEVA_LOWRES_REQUIRE(aligned(chosen, 4), "%s: misaligned choices", what);
  if (batch == 0) return 0;  // (nothing is read or written)
  DEVA_LOWRES_REQUIRE(scores || per_box == 1, "%s: null scores with %d planes per box", what, per_box);
  DEVA_LOWRES_REQUIRE(low && aligned(low, 4), "%s: null or misaligned low-resolution logits", what);
  DEVA_LOWRES_REQUIRE(aligned(scores, 4), "%s: misaligned scores", what);
  DEVA_LOWRES_REQUIRE(out, "%s: null output", what);
  return 0;
}

int proposal_check(const void* low, const void* iou_preds, int batch, const struct deva_lowres_geometry* g, double pred_iou_thresh,
                   double stability_score_thresh, double stability_score_offset, double mask_threshold, const void* arena,
                   int capacity, const void* scratch, int64_t scratch_bytes, struct deva_lowres_plan* plan) {
  const char* what = "deva_lowres_proposal_batch";
  if (int rc = lowres_plan(what, g, plan)) return rc;
  DEVA_LOWRES_REQUIRE(batch >= 0, "%s: negative batch (%d)", what, batch);
  DEVA_LOWRES_REQUIRE(!isnan(pred_iou_thresh) && !isnan(stability_score_thresh) && !isnan(stability_score_offset) &&
                          !isnan(mask_threshold),
                      "%s: a threshold is not a number", what);
  DEVA_LOWRES_REQUIRE(capacity >= 1 && capacity <= deva::kPropMaxMasks, "%s: a capacity of 1 to %d masks (got %d)", what,
                      deva::kPropMaxMasks, capacity);
  const int64_t need = deva::proposal_plan(capacity).bytes;
  DEVA_LOWRES_REQUIRE(scratch_ok(scratch, scratch_bytes, need),
                      "%s: scratch of %lld bytes (16-byte aligned), deva_proposal_scratch asks for %lld", what,
                      (long long)(scratch ? scratch_bytes : 0), (long long)need);
  DEVA_LOWRES_REQUIRE(arena, "%s: null arena", what);
  if (batch == 0) return 0;  // (nothing else is read)
  DEVA_LOWRES_REQUIRE(low && aligned(low, 4), "%s: null or misaligned low-resolution logits", what);
  DEVA_LOWRES_REQUIRE(iou_preds && aligned(iou_preds, 4), "%s: null or misaligned predicted IoUs", what);
  return 0;
}

}  // namespace deva_lowres

extern "C" int deva_lowres_version(void) { return DEVA_LOWRES_ABI_VERSION; }
extern "C" const char* deva_lowres_last_error(void) { return deva_lowres::last_error(); }
extern "C" int deva_lowres_limits(struct deva_lowres_limits* limits) {
  DEVA_LOWRES_REQUIRE(limits, "deva_lowres_limits: null limits");
  limits->max_side = DEVA_LOWRES_MAX_SIDE;
  limits->max_pixels = DEVA_LOWRES_MAX_PIXELS;
  limits->max_per_box = DEVA_LOWRES_MAX_PER_BOX;
  limits->block = deva_lowres::kBlock;
  limits->lds_budget = DEVA_LOWRES_LDS_BUDGET;
  limits->max_tile_rows = DEVA_LOWRES_MAX_TILE_ROWS;
  return 0;
}
extern "C" int deva_lowres_plan(const struct deva_lowres_geometry* geometry, struct deva_lowres_plan* plan) {
  return deva_lowres::lowres_plan("deva_lowres_plan", geometry, plan);
}
