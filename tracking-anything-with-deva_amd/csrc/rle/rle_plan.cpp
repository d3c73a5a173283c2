// The argument checks, rule D2 and the launch decision of the run-length decoder (see rle_plan.h), and the library's
// host-only entry points.
#include "rle_plan.h"

namespace deva_rle {

HOST_ARGS_DEFINE_ERROR_TEXT()
const char* last_error() { return g_err; }

static int check_size(const char* what, const char* which, int height, int width) {
  DEVA_RLE_REQUIRE(height > 0 && width > 0 && (int64_t)height * width <= kMaxPixels, "%s: bad %s size %d x %d (1 <= H * W < 2^31)", what,
                   which, height, width);
  return 0;
}

int decode_plan(const char* what, int n, int height, int width, int out_height, int out_width, int dtype, struct deva_rle_plan* plan) {
  DEVA_RLE_REQUIRE(plan, "%s: null plan", what);
  if (int rc = check_size(what, "source", height, width)) return rc;
  if (int rc = check_size(what, "output", out_height, out_width)) return rc;
  DEVA_RLE_REQUIRE(n >= 0 && n <= DEVA_RLE_MAX_MASKS, "%s: 0 to %d masks a call (got %d)", what, DEVA_RLE_MAX_MASKS, n);
  DEVA_RLE_REQUIRE(dtype == DEVA_RLE_U8 || dtype == DEVA_RLE_F32, "%s: dtype must be DEVA_RLE_U8 or DEVA_RLE_F32 (got %d)", what, dtype);
  const int64_t tiles_x = ((int64_t)out_width + kTile - 1) / kTile, tiles_y = ((int64_t)out_height + kTile - 1) / kTile;
  const int64_t tiles = n * tiles_x * tiles_y;
  plan->tiles_x = (int32_t)tiles_x;
  plan->tiles_y = (int32_t)tiles_y;
  plan->grid = (uint32_t)(tiles < kMaxGrid ? tiles : kMaxGrid);
  plan->lds_bytes = kTile * kPitch;
  plan->scale_y = (float)height / (float)out_height;   // ATen's compute_scales_value<float> without a scale factor
  plan->scale_x = (float)width / (float)out_width;
  plan->out_bytes = (int64_t)n * out_height * out_width * element_bytes(dtype);
  return 0;
}

int runs_check(const char* what, const int32_t* runs, int64_t words, int n, int height, int width) {
  if (int rc = check_size(what, "source", height, width)) return rc;
  DEVA_RLE_REQUIRE(n >= 0 && n <= DEVA_RLE_MAX_MASKS, "%s: 0 to %d masks a call (got %d)", what, DEVA_RLE_MAX_MASKS, n);
  DEVA_RLE_REQUIRE(runs, "%s: null run array", what);
  DEVA_RLE_REQUIRE(words >= (int64_t)n + 1 && words <= DEVA_RLE_MAX_WORDS, "%s: a run array of %lld to %d words (got %lld)", what,
                   (long long)n + 1, DEVA_RLE_MAX_WORDS, (long long)words);
  const int32_t* first = runs;
  const int32_t* starts = runs + n + 1;
  const int64_t held = words - n - 1, total = (int64_t)height * width;
  DEVA_RLE_REQUIRE(first[0] == 0, "%s: first[0] must be 0 (got %d)", what, first[0]);
  for (int k = 0; k < n; ++k) {   // the index first: nothing below reads outside the array
    DEVA_RLE_REQUIRE(first[k + 1] >= first[k] && first[k + 1] <= held, "%s: mask %d: its starts end at word %d of %lld", what, k,
                     first[k + 1], (long long)held);
    DEVA_RLE_REQUIRE(first[k + 1] - first[k] >= 2, "%s: mask %d: no counts (the counts of a mask sum to H * W = %lld)", what, k,
                     (long long)total);
  }
  DEVA_RLE_REQUIRE(first[n] == held, "%s: the run array holds %lld starts, the masks take %d", what, (long long)held, first[n]);
  for (int k = 0; k < n; ++k) {
    const int32_t* s = starts + first[k];
    const int runs_k = first[k + 1] - first[k] - 1;
    DEVA_RLE_REQUIRE(s[0] == 0, "%s: mask %d: the first start must be 0 (got %d)", what, k, s[0]);
    for (int r = 0; r < runs_k; ++r)
      DEVA_RLE_REQUIRE(s[r + 1] >= s[r], "%s: mask %d: count %d is negative (%lld)", what, k, r, (long long)s[r + 1] - s[r]);
    DEVA_RLE_REQUIRE(s[runs_k] == total, "%s: mask %d: the counts sum to %d, H * W is %lld", what, k, s[runs_k], (long long)total);
  }
  return 0;
}

int decode_check(const int32_t* runs_host, const int32_t* runs_device, int64_t words, int n, int height, int width, int out_height,
                 int out_width, int dtype, const void* out, struct deva_rle_plan* plan) {
  const char* what = "deva_rle_decode";
  struct deva_rle_plan local;
  if (!plan) plan = &local;
  if (int rc = decode_plan(what, n, height, width, out_height, out_width, dtype, plan)) return rc;
  if (n == 0) return 0;
  if (int rc = runs_check(what, runs_host, words, n, height, width)) return rc;
  DEVA_RLE_REQUIRE(runs_device && aligned(runs_device, 4), "%s: null or misaligned run array on the device", what);
  DEVA_RLE_REQUIRE(out && aligned(out, element_bytes(dtype)), "%s: null or misaligned out", what);
  DEVA_RLE_REQUIRE(!overlaps(out, plan->out_bytes, runs_device, 4 * words), "%s: out overlaps the run array", what);
  return 0;
}

}  // namespace deva_rle

extern "C" int deva_rle_version(void) { return DEVA_RLE_ABI_VERSION; }
extern "C" const char* deva_rle_last_error(void) { return deva_rle::last_error(); }
extern "C" int deva_rle_limits(struct deva_rle_limits* limits) {
  DEVA_RLE_REQUIRE(limits, "deva_rle_limits: null limits");
  limits->max_masks = DEVA_RLE_MAX_MASKS;
  limits->max_words = DEVA_RLE_MAX_WORDS;
  limits->tile = deva_rle::kTile;
  limits->block = deva_rle::kBlock;
  return 0;
}
extern "C" int deva_rle_plan(int n, int height, int width, int out_height, int out_width, int dtype, struct deva_rle_plan* plan) {
  return deva_rle::decode_plan("deva_rle_plan", n, height, width, out_height, out_width, dtype, plan);
}
extern "C" int deva_rle_check(const int32_t* runs, int64_t words, int n, int height, int width) {
  return deva_rle::runs_check("deva_rle_check", runs, words, n, height, width);
}
