// The argument checks, scratch layout and launch decision of the region kernels (see region_plan.h), and the library's
// host-only entry points.
#include "region_plan.h"

namespace deva_regions {

HOST_ARGS_DEFINE_ERROR_TEXT()
const char* last_error() { return g_err; }

static int check_size(const char* what, int height, int width, int n) {
  DEVA_REGIONS_REQUIRE(height > 0 && width > 0 && (int64_t)height * width <= kMaxPixels, "%s: bad plane size %d x %d", what, height,
                       width);
  DEVA_REGIONS_REQUIRE(n >= 0 && n <= DEVA_REGIONS_MAX_PLANES, "%s: 0 to %d planes (got %d)", what, DEVA_REGIONS_MAX_PLANES, n);
  return 0;
}

PlaneLayout plane_layout(int64_t pixels) {
  ScratchLayout s;
  PlaneLayout p;
  p.labels = s.take(4 * pixels);
  p.areas = s.take(4 * pixels);
  p.state = s.take(4 * kStateWords);
  p.bytes = s.at;
  return p;
}

static uint32_t capped(int64_t groups) { return (uint32_t)(groups < kMaxGrid ? groups : kMaxGrid); }

int region_plan(const char* what, int height, int width, int n, int64_t budget_bytes, struct deva_regions_plan* plan) {
  DEVA_REGIONS_REQUIRE(plan, "%s: null plan", what);
  if (int rc = check_size(what, height, width, n)) return rc;
  const int64_t pixels = (int64_t)height * width;
  const int64_t plane_bytes = plane_layout(pixels).bytes;
  int64_t together = n;
  if (budget_bytes >= 0 && n > 0) {
    DEVA_REGIONS_REQUIRE(budget_bytes >= plane_bytes, "%s: the scratch holds %lld bytes, %lld are needed for one plane", what,
                         (long long)budget_bytes, (long long)plane_bytes);
    const int64_t fit = budget_bytes / plane_bytes;
    together = fit < n ? fit : n;
  }
  const int64_t tiles_x = ((int64_t)width + kTile - 1) / kTile, tiles_y = ((int64_t)height + kTile - 1) / kTile;
  const int64_t seam_pixels = (tiles_x - 1) * height + (tiles_y - 1) * width;   // beside a tile edge, per plane
  plan->tile = kTile;
  plan->block = kBlock;
  plan->tiles_x = (int32_t)tiles_x;
  plan->tiles_y = (int32_t)tiles_y;
  plan->planes_per_pass = (int32_t)together;
  plan->passes = together ? (int32_t)((n + together - 1) / together) : 0;
  plan->local_grid = capped(together * tiles_x * tiles_y);
  plan->border_grid = capped((together * seam_pixels + kBlock - 1) / kBlock);
  plan->pixel_grid = capped(together * ((pixels + kBlock - 1) / kBlock));
  plan->reserved = 0;
  plan->plane_bytes = plane_bytes;
  plan->scratch_bytes = together * plane_bytes;
  return 0;
}

int label_check(const void* planes, int n, int height, int width, const void* labels, struct deva_regions_plan* plan) {
  const char* what = "deva_regions_label";
  struct deva_regions_plan local;
  if (!plan) plan = &local;
  if (int rc = region_plan(what, height, width, n, -1, plan)) return rc;
  if (n == 0) return 0;
  DEVA_REGIONS_REQUIRE(planes, "%s: null planes", what);
  DEVA_REGIONS_REQUIRE(labels && aligned(labels, 4), "%s: null or misaligned labels", what);
  const int64_t pixels = (int64_t)n * height * width;
  DEVA_REGIONS_REQUIRE(!overlaps(labels, 4 * pixels, planes, pixels), "%s: labels overlaps an input", what);
  return 0;
}

int clean_check(const void* planes, int n, int height, int width, int min_area, const void* records, const void* scratch,
                int64_t scratch_bytes, struct deva_regions_plan* plan) {
  const char* what = "deva_regions_clean";
  struct deva_regions_plan local;
  if (!plan) plan = &local;
  DEVA_REGIONS_REQUIRE(min_area > 0, "%s: min_area must be positive (got %d)", what, min_area);
  if (int rc = region_plan(what, height, width, n, -1, plan)) return rc;   // the sizes first: their text, not the budget's
  if (n == 0) return 0;
  DEVA_REGIONS_REQUIRE(planes, "%s: null planes", what);
  DEVA_REGIONS_REQUIRE(records && aligned(records, 4), "%s: null or misaligned records", what);
  DEVA_REGIONS_REQUIRE(scratch && aligned(scratch, 16), "%s: null or misaligned scratch", what);
  if (int rc = region_plan(what, height, width, n, scratch_bytes < 0 ? 0 : scratch_bytes, plan)) return rc;
  const int64_t pixels = (int64_t)n * height * width, record_bytes = 4ll * DEVA_REGIONS_FIELDS * n;
  DEVA_REGIONS_REQUIRE(!overlaps(records, record_bytes, planes, pixels) && !overlaps(records, record_bytes, scratch, plan->scratch_bytes),
                       "%s: records overlaps an input", what);
  DEVA_REGIONS_REQUIRE(!overlaps(scratch, plan->scratch_bytes, planes, pixels), "%s: the scratch overlaps an input", what);
  return 0;
}

}  // namespace deva_regions

extern "C" int deva_regions_version(void) { return DEVA_REGIONS_ABI_VERSION; }
extern "C" const char* deva_regions_last_error(void) { return deva_regions::last_error(); }
extern "C" int deva_regions_scratch_bytes(int height, int width, int n, int64_t* bytes) {
  const char* what = "deva_regions_scratch_bytes";
  DEVA_REGIONS_REQUIRE(bytes, "%s: null bytes", what);
  struct deva_regions_plan plan;
  if (int rc = deva_regions::region_plan(what, height, width, n, -1, &plan)) return rc;
  *bytes = plan.scratch_bytes;
  return 0;
}
extern "C" int deva_regions_plan(int height, int width, int n, int64_t budget_bytes, struct deva_regions_plan* plan) {
  const char* what = "deva_regions_plan";
  DEVA_REGIONS_REQUIRE(budget_bytes >= 0, "%s: a scratch budget of 0 bytes or more (got %lld)", what, (long long)budget_bytes);
  return deva_regions::region_plan(what, height, width, n, budget_bytes, plan);
}
