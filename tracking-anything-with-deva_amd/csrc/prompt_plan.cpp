// Argument checks and scratch layout of the prompt-point choice (see prompt_plan.h); deva_prompt_scratch.
#include "prompt_plan.h"

#include <math.h>

#include "deva_hip.h"
#include "host_error.h"

namespace deva {

bool prompt_size_ok(int height, int width) {
  return height >= kPromptScale && width >= kPromptScale && height <= kPromptMaxSide && width <= kPromptMaxSide &&
         (int64_t)height * width <= kPromptMaxPixels;
}

bool prompt_points_ok(int points) { return points >= 1 && points <= kPromptMaxPoints; }

PromptPlan prompt_plan(int height, int width) {
  PromptPlan p;
  p.low_h = height / kPromptScale, p.low_w = width / kPromptScale;
  ScratchLayout s;
  p.off_rows = s.take((int64_t)height * p.low_w * 4);
  p.off_low = s.take((int64_t)p.low_h * p.low_w * 4);
  p.bytes = s.at;
  return p;
}

int prompt_points_check(const void* mask, int mask_elem_bytes, int height, int width, const void* points_xy, int points,
                        double threshold, const void* scratch, int64_t scratch_bytes, const void* out_points,
                        const void* out_labels, const void* out_count) {
  const char* what = "deva_prompt_points";
  DEVA_REQUIRE(mask_elem_bytes == 1 || mask_elem_bytes == 8, "%s: a mask of 1-byte or 8-byte elements (got %d)", what,
               mask_elem_bytes);
  DEVA_REQUIRE(height >= kPromptScale && width >= kPromptScale,
               "%s: a mask of at least %d x %d (got %d x %d): the map of a smaller one is empty", what, kPromptScale,
               kPromptScale, height, width);
  DEVA_REQUIRE(prompt_size_ok(height, width), "%s: bad mask size %d x %d", what, height, width);
  DEVA_REQUIRE(points >= 1, "%s: at least one point (got %d)", what, points);
  DEVA_REQUIRE(points <= kPromptMaxPoints, "%s: at most %d points (got %d)", what, kPromptMaxPoints, points);
  DEVA_REQUIRE(!isnan(threshold), "%s: the threshold is not a number", what);
  DEVA_REQUIRE(mask && aligned(mask, mask_elem_bytes), "%s: null or misaligned mask", what);
  DEVA_REQUIRE(points_xy && aligned(points_xy, 4), "%s: null or misaligned points", what);
  DEVA_REQUIRE(out_points && aligned(out_points, 4), "%s: null or misaligned kept points", what);
  DEVA_REQUIRE(out_labels && aligned(out_labels, 4), "%s: null or misaligned labels", what);
  DEVA_REQUIRE(out_count && aligned(out_count, 4), "%s: null or misaligned count", what);
  const int64_t need = prompt_plan(height, width).bytes;
  DEVA_REQUIRE(scratch_ok(scratch, scratch_bytes, need),
               "%s: scratch of %lld bytes (16-byte aligned), deva_prompt_scratch asks for %lld", what,
               (long long)(scratch ? scratch_bytes : 0), (long long)need);
  return 0;
}

}  // namespace deva

extern "C" int64_t deva_prompt_scratch(int height, int width, int points) {
  if (!deva::prompt_size_ok(height, width) || !deva::prompt_points_ok(points)) return -1;
  return deva::prompt_plan(height, width).bytes;
}
