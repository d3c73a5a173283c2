// The argument checks, the segment geometry and the sizes of the PNG deflate coder (see png_plan.h), and the library's
// host-only entry points.
#include "png_plan.h"

namespace deva_png {

HOST_ARGS_DEFINE_ERROR_TEXT()
const char* last_error() { return g_err; }

int png_plan(const char* what, int height, int width, int bpp, struct deva_png_plan* plan) {
  DEVA_PNG_REQUIRE(plan, "%s: null plan", what);
  DEVA_PNG_REQUIRE(bpp == 1 || bpp == 3, "%s: bpp: 1 ([H,W]) or 3 ([H,W,3]) bytes a pixel (got %d)", what, bpp);
  DEVA_PNG_REQUIRE(height >= 1 && width >= 1 && height <= DEVA_PNG_MAX_SIDE && width <= DEVA_PNG_MAX_SIDE,
                   "%s: bad height x width %d x %d (1 to %d each)", what, height, width, DEVA_PNG_MAX_SIDE);
  const int64_t row_bytes = (int64_t)width * bpp;
  DEVA_PNG_REQUIRE(row_bytes * height <= DEVA_PNG_MAX_BYTES, "%s: a plane of %d x %d x %d bytes, a call takes %d", what, height, width, bpp,
                   DEVA_PNG_MAX_BYTES);
  const int rows = DEVA_PNG_ROWS_PER_SEGMENT;
  plan->rows_per_segment = rows;
  plan->segments = (height + rows - 1) / rows;
  plan->row_bytes = (int32_t)row_bytes;
  plan->steps_per_row = (int32_t)((row_bytes + 1 + DEVA_PNG_STEP - 1) / DEVA_PNG_STEP);
  plan->block = kBlock;
  plan->reserved = 0;
  plan->slot_bytes = (segment_worst(rows, row_bytes) + 15) / 16 * 16;
  int64_t at[4];
  plan->scratch_bytes = scratch_layout(plan->segments, plan->slot_bytes, at);
  const int last_rows = height - (plan->segments - 1) * rows;
  plan->worst_case = 2 + (plan->segments - 1) * segment_worst(rows, row_bytes) + segment_worst(last_rows, row_bytes) + 2 + 4;
  return 0;
}

int place_check(const char* what, int height, int width, int bpp, const void* scratch, int64_t scratch_bytes, const uint8_t* out,
                int64_t capacity, const int64_t* info, struct deva_png_plan* plan) {
  struct deva_png_plan local;
  if (!plan) plan = &local;
  if (int rc = png_plan(what, height, width, bpp, plan)) return rc;
  DEVA_PNG_REQUIRE(capacity >= 0 && capacity <= (1ll << 40), "%s: capacity: 0 to 2^40 (got %lld)", what, (long long)capacity);
  DEVA_PNG_REQUIRE(out || capacity == 0, "%s: out: null", what);
  DEVA_PNG_REQUIRE(scratch && aligned(scratch, 16), "%s: scratch: null or not 16-byte aligned", what);
  DEVA_PNG_REQUIRE(scratch_bytes >= plan->scratch_bytes, "%s: scratch_bytes: %lld given, deva_png_plan asks for %lld", what,
                   (long long)scratch_bytes, (long long)plan->scratch_bytes);
  DEVA_PNG_REQUIRE(info && aligned(info, 8), "%s: info: null or misaligned", what);
  DEVA_PNG_REQUIRE(!overlaps(out, capacity, scratch, plan->scratch_bytes), "%s: out overlaps scratch", what);
  DEVA_PNG_REQUIRE(!overlaps(info, 32, scratch, plan->scratch_bytes), "%s: info overlaps scratch", what);
  DEVA_PNG_REQUIRE(!overlaps(info, 32, out, capacity), "%s: info overlaps out", what);
  return 0;
}

int deflate_check(const uint8_t* plane, int height, int width, int bpp, const void* scratch, int64_t scratch_bytes, const uint8_t* out,
                  int64_t capacity, const int64_t* info, struct deva_png_plan* plan) {
  const char* what = "deva_png_deflate";
  struct deva_png_plan local;
  if (!plan) plan = &local;
  if (int rc = place_check(what, height, width, bpp, scratch, scratch_bytes, out, capacity, info, plan)) return rc;
  DEVA_PNG_REQUIRE(plane, "%s: plane: null", what);
  const int64_t bytes = (int64_t)plan->row_bytes * height;
  DEVA_PNG_REQUIRE(!overlaps(plane, bytes, scratch, plan->scratch_bytes), "%s: plane overlaps scratch", what);
  DEVA_PNG_REQUIRE(!overlaps(plane, bytes, out, capacity), "%s: plane overlaps out", what);
  DEVA_PNG_REQUIRE(!overlaps(plane, bytes, info, 32), "%s: plane overlaps info", what);
  return 0;
}

}  // namespace deva_png

extern "C" int deva_png_version(void) { return DEVA_PNG_ABI_VERSION; }
extern "C" const char* deva_png_last_error(void) { return deva_png::last_error(); }
extern "C" int deva_png_limits(struct deva_png_limits* limits) {
  DEVA_PNG_REQUIRE(limits, "deva_png_limits: null limits");
  limits->max_side = DEVA_PNG_MAX_SIDE;
  limits->max_bytes = DEVA_PNG_MAX_BYTES;
  limits->rows_per_segment = DEVA_PNG_ROWS_PER_SEGMENT;
  limits->step = DEVA_PNG_STEP;
  limits->block = deva_png::kBlock;
  limits->lds_bytes = deva_png::kLdsBytes;
  return 0;
}
extern "C" int deva_png_plan(int height, int width, int bpp, struct deva_png_plan* plan) {
  return deva_png::png_plan("deva_png_plan", height, width, bpp, plan);
}
