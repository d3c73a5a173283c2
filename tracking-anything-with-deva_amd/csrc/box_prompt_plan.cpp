// Argument checks of the box prompts (see box_prompt_plan.h).
#include "box_prompt_plan.h"

#include <math.h>

#include "deva_hip.h"
#include "host_error.h"
#include "proposal_plan.h"

namespace deva {

int box_select_chunks(int height, int width) { return (int)(((int64_t)height * width + 3 + kBoxChunk - 1) / kBoxChunk); }

int box_nms_xyxy_check(const void* boxes, const void* scores, int n, double thresh, const void* scratch, int64_t scratch_bytes,
                       const void* keep, const void* n_keep) {
  const char* what = "deva_box_nms_xyxy";
  DEVA_REQUIRE(n >= 0, "%s: negative number of boxes (%d)", what, n);
  DEVA_REQUIRE(n <= kPropMaxMasks, "%s: at most %d boxes (got %d)", what, kPropMaxMasks, n);
  DEVA_REQUIRE(!isnan(thresh), "%s: the NMS threshold is not a number", what);
  DEVA_REQUIRE(n_keep && aligned(n_keep, 4), "%s: null or misaligned keep count", what);
  if (n == 0) return 0;  // (a count of 0: nothing else is touched)
  DEVA_REQUIRE(boxes && aligned(boxes, 4), "%s: null or misaligned boxes", what);
  DEVA_REQUIRE(scores && aligned(scores, 4), "%s: null or misaligned scores", what);
  DEVA_REQUIRE(keep && aligned(keep, 4), "%s: null or misaligned keep list", what);
  const int64_t need = proposal_plan(n).bytes;
  DEVA_REQUIRE(scratch_ok(scratch, scratch_bytes, need),
               "%s: scratch of %lld bytes (16-byte aligned), deva_proposal_scratch asks for %lld", what,
               (long long)(scratch ? scratch_bytes : 0), (long long)need);
  return 0;
}

int box_mask_select_check(const void* logits, const void* scores, int batch, int per_box, int height, int width,
                          double mask_threshold, const void* out, const void* chosen) {
  const char* what = "deva_box_mask_select";
  DEVA_REQUIRE(batch >= 0, "%s: negative batch (%d)", what, batch);
  DEVA_REQUIRE(per_box >= 1 && per_box <= kBoxMaxPerBox, "%s: 1 to %d planes per box (got %d)", what, kBoxMaxPerBox, per_box);
  DEVA_REQUIRE(height > 0 && width > 0 && (int64_t)height * width <= kBoxMaxPixels, "%s: bad plane size %d x %d", what,
               height, width);
  DEVA_REQUIRE(!isnan(mask_threshold), "%s: the mask threshold is not a number", what);
  DEVA_REQUIRE(aligned(chosen, 4), "%s: misaligned choice list", what);
  if (batch == 0) return 0;  // (nothing else is read or written)
  // batch * per_box * pixels * 4 bytes stays below 2^63: 2^31 * 2^4 * 2^30 * 2^2 does not
  DEVA_REQUIRE((int64_t)batch * per_box <= (int64_t)1 << 30, "%s: %d boxes of %d planes are more than 2^30 planes", what, batch,
               per_box);
  DEVA_REQUIRE(logits && aligned(logits, 4), "%s: null or misaligned logits", what);
  DEVA_REQUIRE(scores && aligned(scores, 4), "%s: null or misaligned scores", what);
  DEVA_REQUIRE(out, "%s: null output", what);
  return 0;
}

}  // namespace deva
