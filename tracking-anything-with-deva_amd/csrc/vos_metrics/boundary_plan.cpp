// The radius rule, argument checks and launch decision of the DAVIS counts (see boundary_plan.h), and the library's
// host-only entry points.
#include "boundary_plan.h"

#include <math.h>

namespace deva_vos {

HOST_ARGS_DEFINE_ERROR_TEXT()
const char* last_error() { return g_err; }

int encoding_bytes(int encoding) {
  switch (encoding & ~DEVA_VOS_BINARY) {
    case DEVA_VOS_U8: return 1;
    case DEVA_VOS_I32: return 4;
    case DEVA_VOS_I64: return 8;
    case DEVA_VOS_INDEX16: return 2;
    default: return 0;
  }
}

static int check_size(const char* what, int height, int width) {
  DEVA_VOS_REQUIRE(height > 0 && width > 0 && (int64_t)height * width <= kMaxPixels, "%s: bad plane size %d x %d", what, height,
                   width);
  return 0;
}

int boundary_radius(const char* what, int height, int width, double bound_th, int* radius) {
  DEVA_VOS_REQUIRE(radius, "%s: null radius", what);
  if (int rc = check_size(what, height, width)) return rc;
  DEVA_VOS_REQUIRE(isfinite(bound_th) && bound_th >= 0.0, "%s: bound_th must be finite and not negative (got %g)", what, bound_th);
  double r;
  if (bound_th >= 1.0) {  // R3: a radius in pixels
    DEVA_VOS_REQUIRE(bound_th == floor(bound_th), "%s: a bound_th of 1 or more is a radius in pixels, an integer (got %g)", what,
                     bound_th);
    r = bound_th;
  } else {
    const int64_t h = height, w = width;
    r = ceil(bound_th * sqrt((double)(h * h + w * w)));
  }
  DEVA_VOS_REQUIRE(r <= (double)DEVA_VOS_MAX_RADIUS, "%s: radius 0 to %d (bound_th %g gives %.0f at %d x %d)", what,
                   DEVA_VOS_MAX_RADIUS, bound_th, r, height, width);
  *radius = (int)r;
  return 0;
}

int boundary_plan(const char* what, int height, int width, int n_objects, int radius, deva_vos_plan* plan) {
  DEVA_VOS_REQUIRE(plan, "%s: null plan", what);
  DEVA_VOS_REQUIRE(n_objects >= 1 && n_objects <= DEVA_VOS_MAX_OBJECTS, "%s: 1 to %d objects (got %d)", what, DEVA_VOS_MAX_OBJECTS,
                   n_objects);
  DEVA_VOS_REQUIRE(radius >= 0 && radius <= DEVA_VOS_MAX_RADIUS, "%s: radius 0 to %d (got %d)", what, DEVA_VOS_MAX_RADIUS, radius);
  if (int rc = check_size(what, height, width)) return rc;
  const int64_t pixels = (int64_t)height * width;
  const int64_t strips = (int64_t)height * (((int64_t)width + DEVA_VOS_STRIP - 1) / DEVA_VOS_STRIP);
  const int64_t label_groups = (strips + kBlock - 1) / kBlock;
  const int64_t chunks = (pixels + kWave - 1) / kWave;
  const int64_t match_groups = (chunks + kBlock / kWave - 1) / (kBlock / kWave);
  plan->label_grid = (uint32_t)(label_groups < kMaxGrid ? label_groups : kMaxGrid);
  plan->match_grid = (uint32_t)(match_groups < kMaxMatchGrid ? match_groups : kMaxMatchGrid);
  plan->block = kBlock;
  plan->lds_bytes = 4u * (uint32_t)n_objects * 4u;  // the id table and fields 0 - 2 of every object
  plan->inner_radius = radius < DEVA_VOS_INNER_RADIUS ? radius : DEVA_VOS_INNER_RADIUS;
  plan->radius = radius;
  plan->scratch_bytes = pixels * kWordBytes;
  return 0;
}

int boundary_counts_check(const void* gt, int gt_encoding, const void* pred, int pred_encoding, const void* ids, int n_objects,
                          const void* pred_lut, int channels, int height, int width, int radius, const void* scratch,
                          int64_t scratch_bytes, const void* counts, deva_vos_plan* plan) {
  const char* what = "deva_vos_boundary_counts";
  const int gt_plain = gt_encoding & ~DEVA_VOS_BINARY, pred_plain = pred_encoding & ~DEVA_VOS_BINARY;
  DEVA_VOS_REQUIRE(gt_encoding >= 0 && (gt_plain == DEVA_VOS_U8 || gt_plain == DEVA_VOS_I32),
                   "%s: the ground truth is U8 (0) or I32 (1), with or without BINARY (256) (got encoding %d)", what, gt_encoding);
  DEVA_VOS_REQUIRE(pred_encoding >= 0 && pred_plain >= DEVA_VOS_U8 && pred_plain <= DEVA_VOS_INDEX16,
                   "%s: unknown encoding %d of the prediction", what, pred_encoding);
  deva_vos_plan local;
  if (!plan) plan = &local;
  if (int rc = boundary_plan(what, height, width, n_objects, radius, plan)) return rc;
  const bool binary = ((gt_encoding | pred_encoding) & DEVA_VOS_BINARY) != 0;
  DEVA_VOS_REQUIRE(!binary || n_objects == 1, "%s: BINARY planes hold one object (got %d)", what, n_objects);
  const bool fast = pred_plain == DEVA_VOS_INDEX16;
  DEVA_VOS_REQUIRE(gt && aligned(gt, 16), "%s: null or misaligned ground-truth plane", what);
  DEVA_VOS_REQUIRE(pred && aligned(pred, 16), "%s: null or misaligned predicted plane", what);
  DEVA_VOS_REQUIRE(ids && aligned(ids, 4), "%s: null or misaligned id table", what);
  if (fast) {
    DEVA_VOS_REQUIRE(channels >= 1 && channels <= 32767, "%s: 1 to 32767 channels (got %d)", what, channels);
    DEVA_VOS_REQUIRE(pred_lut && aligned(pred_lut, 2), "%s: null or misaligned channel table", what);
  }
  DEVA_VOS_REQUIRE(scratch && aligned(scratch, 16), "%s: null or misaligned scratch", what);
  DEVA_VOS_REQUIRE(scratch_bytes >= plan->scratch_bytes, "%s: the scratch holds %lld bytes, %lld are needed", what,
                   (long long)scratch_bytes, (long long)plan->scratch_bytes);
  DEVA_VOS_REQUIRE(counts && aligned(counts, 4), "%s: null or misaligned counts", what);
  const int64_t pixels = (int64_t)height * width;
  const int64_t out_bytes = 4ll * DEVA_VOS_FIELDS * n_objects;
  const bool clash = overlaps(counts, out_bytes, gt, pixels * encoding_bytes(gt_encoding)) ||
                     overlaps(counts, out_bytes, pred, pixels * encoding_bytes(pred_encoding)) ||
                     overlaps(counts, out_bytes, ids, 4ll * n_objects) ||
                     (fast && overlaps(counts, out_bytes, pred_lut, 2ll * channels)) ||
                     overlaps(counts, out_bytes, scratch, plan->scratch_bytes);
  DEVA_VOS_REQUIRE(!clash, "%s: counts overlaps an input", what);
  const bool scribble = overlaps(scratch, plan->scratch_bytes, gt, pixels * encoding_bytes(gt_encoding)) ||
                        overlaps(scratch, plan->scratch_bytes, pred, pixels * encoding_bytes(pred_encoding)) ||
                        overlaps(scratch, plan->scratch_bytes, ids, 4ll * n_objects) ||
                        (fast && overlaps(scratch, plan->scratch_bytes, pred_lut, 2ll * channels));
  DEVA_VOS_REQUIRE(!scribble, "%s: the scratch overlaps an input", what);
  return 0;
}

}  // namespace deva_vos

extern "C" int deva_vos_version(void) { return DEVA_VOS_ABI_VERSION; }
extern "C" const char* deva_vos_last_error(void) { return deva_vos::last_error(); }
extern "C" int deva_vos_boundary_radius(int height, int width, double bound_th, int* radius) {
  return deva_vos::boundary_radius("deva_vos_boundary_radius", height, width, bound_th, radius);
}
extern "C" int deva_vos_boundary_scratch_bytes(int height, int width, int64_t* bytes) {
  const char* what = "deva_vos_boundary_scratch_bytes";
  DEVA_VOS_REQUIRE(bytes, "%s: null bytes", what);
  deva_vos_plan plan;
  if (int rc = deva_vos::boundary_plan(what, height, width, 1, 0, &plan)) return rc;
  *bytes = plan.scratch_bytes;
  return 0;
}
extern "C" int deva_vos_boundary_plan(int height, int width, int n_objects, int radius, deva_vos_plan* plan) {
  return deva_vos::boundary_plan("deva_vos_boundary_plan", height, width, n_objects, radius, plan);
}
