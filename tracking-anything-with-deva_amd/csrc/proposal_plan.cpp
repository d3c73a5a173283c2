// Argument checks and scratch layout of the proposal filter (see proposal_plan.h); deva_proposal_scratch.
#include "proposal_plan.h"

#include <math.h>

#include "deva_hip.h"
#include "host_error.h"

namespace deva {

bool proposal_capacity_ok(int capacity) { return capacity >= 1 && capacity <= kPropMaxMasks; }

int proposal_chunks(int height, int width) {
  return (int)(((int64_t)height * width + 15 + kPropChunk - 1) / kPropChunk);
}

static int scratch_check(const char* what, int capacity, const void* scratch, int64_t scratch_bytes) {
  DEVA_REQUIRE(capacity >= 1, "%s: a capacity of at least one mask (got %d)", what, capacity);
  DEVA_REQUIRE(capacity <= kPropMaxMasks, "%s: at most %d masks (got %d)", what, kPropMaxMasks, capacity);
  const int64_t need = proposal_plan(capacity).bytes;
  DEVA_REQUIRE(scratch_ok(scratch, scratch_bytes, need),
               "%s: scratch of %lld bytes (16-byte aligned), deva_proposal_scratch asks for %lld", what,
               (long long)(scratch ? scratch_bytes : 0), (long long)need);
  return 0;
}

static int plane_check(const char* what, int height, int width) {
  DEVA_REQUIRE(height > 0 && width > 0 && (int64_t)height * width <= kPropMaxPixels, "%s: bad plane size %d x %d", what,
               height, width);
  return 0;
}

int proposal_begin_check(int capacity, const void* scratch, int64_t scratch_bytes) {
  return scratch_check("deva_proposal_begin", capacity, scratch, scratch_bytes);
}

int proposal_batch_check(const void* logits, const void* iou_preds, int batch, int height, int width, double pred_iou_thresh,
                         double stability_score_thresh, double stability_score_offset, double mask_threshold,
                         const void* arena, int capacity, const void* scratch, int64_t scratch_bytes) {
  const char* what = "deva_proposal_batch";
  DEVA_REQUIRE(batch >= 0, "%s: negative batch (%d)", what, batch);
  if (int e = plane_check(what, height, width)) return e;
  DEVA_REQUIRE(!isnan(pred_iou_thresh) && !isnan(stability_score_thresh) && !isnan(stability_score_offset) &&
                   !isnan(mask_threshold),
               "%s: a threshold is not a number", what);
  if (int e = scratch_check(what, capacity, scratch, scratch_bytes)) return e;
  DEVA_REQUIRE(arena, "%s: null arena", what);
  if (batch == 0) return 0;  // (nothing else is read)
  DEVA_REQUIRE(logits && aligned(logits, 4), "%s: null or misaligned logits", what);
  DEVA_REQUIRE(iou_preds, "%s: null predicted IoUs", what);
  return 0;
}

int proposal_finish_check(int capacity, double box_nms_thresh, const void* scratch, int64_t scratch_bytes, const void* result) {
  const char* what = "deva_proposal_finish";
  if (int e = scratch_check(what, capacity, scratch, scratch_bytes)) return e;
  DEVA_REQUIRE(!isnan(box_nms_thresh), "%s: the NMS threshold is not a number", what);
  DEVA_REQUIRE(result && aligned(result, 4), "%s: null or misaligned result table", what);
  return 0;
}

int proposal_gather_check(const void* arena, int capacity, int height, int width, const void* scratch, int64_t scratch_bytes,
                          int n_kept, const void* out) {
  const char* what = "deva_proposal_gather";
  if (int e = plane_check(what, height, width)) return e;
  if (int e = scratch_check(what, capacity, scratch, scratch_bytes)) return e;
  DEVA_REQUIRE(n_kept >= 0 && n_kept <= capacity, "%s: %d kept masks of a capacity of %d", what, n_kept, capacity);
  if (n_kept == 0) return 0;
  DEVA_REQUIRE(arena, "%s: null arena", what);
  DEVA_REQUIRE(out, "%s: null output", what);
  return 0;
}

int box_nms_check(const void* boxes, const void* scores, int m, double box_nms_thresh, const void* scratch,
                  int64_t scratch_bytes, const void* keep, const void* n_keep) {
  const char* what = "deva_box_nms";
  DEVA_REQUIRE(m >= 0, "%s: negative number of boxes (%d)", what, m);
  DEVA_REQUIRE(m <= kPropMaxMasks, "%s: at most %d boxes (got %d)", what, kPropMaxMasks, m);
  DEVA_REQUIRE(!isnan(box_nms_thresh), "%s: the NMS threshold is not a number", what);
  DEVA_REQUIRE(n_keep && aligned(n_keep, 4), "%s: null or misaligned keep count", what);
  if (m == 0) return 0;  // (a count of 0: nothing else is touched)
  DEVA_REQUIRE(boxes && aligned(boxes, 4), "%s: null or misaligned boxes", what);
  DEVA_REQUIRE(scores && aligned(scores, 4), "%s: null or misaligned scores", what);
  DEVA_REQUIRE(keep && aligned(keep, 4), "%s: null or misaligned keep list", what);
  return scratch_check(what, m, scratch, scratch_bytes);
}

}  // namespace deva

extern "C" int64_t deva_proposal_scratch(int capacity) {
  if (!deva::proposal_capacity_ok(capacity)) return -1;
  return deva::proposal_plan(capacity).bytes;
}
