// Argument checks and scratch layout of deva_detection_assemble (see detection_plan.h); deva_detection_scratch.
#include "detection_plan.h"

#include <math.h>

#include "deva_hip.h"
#include "host_error.h"

namespace deva {

bool detection_sizes_ok(int n, int h0, int w0, int oh, int ow) {
  return n >= 0 && n <= kDetMaxMasks && h0 > 0 && w0 > 0 && oh > 0 && ow > 0 && (int64_t)h0 * w0 < (1ll << 31) &&
         (int64_t)oh * ow < (1ll << 31);
}

DetectionPlan detection_plan(int n, int h0, int w0, int oh, int ow) {
  DetectionPlan p;
  const int64_t src = (int64_t)h0 * w0, dst = (int64_t)oh * ow;
  const int64_t most = src > dst ? src : dst;
  p.chunks = (int)((most + kDetChunk - 1) / kDetChunk);
  const int64_t part = (int64_t)n * p.chunks * 4, per_mask = (int64_t)n * 4;
  ScratchLayout s;
  p.off_part_area = s.take(part);
  p.off_part_orig = s.take(part);
  p.off_part_src = s.take(part);
  p.off_area = s.take(per_mask);
  p.off_orig = s.take(per_mask);
  p.off_src = s.take(per_mask);
  p.off_mult = s.take(per_mask);
  p.off_stats = s.take((int64_t)(n + 1) * 8);
  p.off_lut = s.take((int64_t)(n + 1) * 4);
  p.off_plane = s.take(dst * 2);
  p.bytes = s.at;
  return p;
}

int detection_check(const void* masks, int n, int h0, int w0, int oh, int ow, int policy, double overlap_threshold,
                    const void* scratch, int64_t scratch_bytes, const void* out, const void* records) {
  const char* what = "deva_detection_assemble";
  DEVA_REQUIRE(n >= 0, "%s: negative number of masks (%d)", what, n);
  DEVA_REQUIRE(n <= kDetMaxMasks, "%s: at most %d masks (got %d)", what, kDetMaxMasks, n);
  DEVA_REQUIRE(oh > 0 && ow > 0, "%s: bad output size %d x %d", what, oh, ow);
  DEVA_REQUIRE((int64_t)oh * ow < (1ll << 31), "%s: output of 2^31 pixels or more", what);
  DEVA_REQUIRE(policy == DET_SUPPRESS_SMALL || policy == DET_PREFER_SMALL || policy == DET_TEXT,
               "%s: unknown policy %d (0 suppress small masks, 1 prefer small masks, 2 text-prompted)", what, policy);
  DEVA_REQUIRE(out, "%s: null output mask", what);
  if (n == 0) return 0;  // (an all-zero mask: nothing else is read)
  DEVA_REQUIRE(masks, "%s: null masks", what);
  DEVA_REQUIRE(h0 > 0 && w0 > 0 && (int64_t)h0 * w0 < (1ll << 31), "%s: bad mask size %d x %d", what, h0, w0);
  DEVA_REQUIRE(records, "%s: null record table", what);
  DEVA_REQUIRE(policy != DET_SUPPRESS_SMALL || !isnan(overlap_threshold), "%s: the overlap threshold is not a number", what);
  const int64_t need = detection_plan(n, h0, w0, oh, ow).bytes;
  DEVA_REQUIRE(scratch_ok(scratch, scratch_bytes, need),
               "%s: scratch of %lld bytes (16-byte aligned), deva_detection_scratch asks for %lld", what,
               (long long)(scratch ? scratch_bytes : 0), (long long)need);
  return 0;
}

}  // namespace deva

extern "C" int64_t deva_detection_scratch(int n_masks, int height, int width, int out_height, int out_width) {
  if (!deva::detection_sizes_ok(n_masks, height, width, out_height, out_width)) return -1;
  if (n_masks == 0) return 0;
  return deva::detection_plan(n_masks, height, width, out_height, out_width).bytes;
}
