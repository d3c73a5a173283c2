// The argument checks, rule E6 and the launch decision of the run-length encoder (see mask_runs_plan.h), and the
// library's host-only entry points.
#include "mask_runs_plan.h"

namespace deva_runs {

HOST_ARGS_DEFINE_ERROR_TEXT()
const char* last_error() { return g_err; }

static int64_t capped(int64_t groups) { return groups < kMaxGrid ? groups : kMaxGrid; }

int runs_plan(const char* what, int n, int height, int width, struct deva_runs_plan* plan) {
  DEVA_RUNS_REQUIRE(plan, "%s: null plan", what);
  DEVA_RUNS_REQUIRE(height > 0 && width > 0 && (int64_t)height * width <= kMaxPixels, "%s: bad height x width %d x %d (1 <= H * W < 2^31)",
                    what, height, width);
  DEVA_RUNS_REQUIRE(n >= 0 && n <= DEVA_RUNS_MAX_MASKS, "%s: n: 0 to %d masks a call (got %d)", what, DEVA_RUNS_MAX_MASKS, n);
  const int64_t tiles_x = ((int64_t)width + kTile - 1) / kTile, tiles_y = ((int64_t)height + kTile - 1) / kTile;
  const int64_t segments = (int64_t)width * tiles_y;           // <= H * W < 2^31
  const int64_t bytes = (int64_t)n * segments * kSegmentBytes;
  DEVA_RUNS_REQUIRE(bytes <= DEVA_RUNS_MAX_SCRATCH, "%s: n: %d masks of %d x %d need %lld bytes of scratch, a call takes %d", what, n, height,
                    width, (long long)bytes, DEVA_RUNS_MAX_SCRATCH);
  plan->tiles_x = (int32_t)tiles_x;
  plan->tiles_y = (int32_t)tiles_y;
  plan->segments = (int32_t)segments;
  plan->scan_chunks = (int32_t)((segments + DEVA_RUNS_SCAN_CHUNK - 1) / DEVA_RUNS_SCAN_CHUNK);
  plan->mask_chunks = (n + DEVA_RUNS_MASK_CHUNK - 1) / DEVA_RUNS_MASK_CHUNK;
  plan->count_grid = (uint32_t)capped(n * tiles_x * tiles_y);
  plan->write_grid = (uint32_t)capped(n * ((segments + kBlock - 1) / kBlock));
  plan->reserved = 0;
  plan->scratch_bytes = bytes;
  return 0;
}

static int scratch_check(const char* what, const void* scratch, int64_t scratch_bytes, const struct deva_runs_plan& plan) {
  DEVA_RUNS_REQUIRE(scratch && aligned(scratch, 4), "%s: scratch: null or not 4-byte aligned", what);
  DEVA_RUNS_REQUIRE(scratch_bytes >= plan.scratch_bytes, "%s: scratch_bytes: %lld given, deva_runs_scratch asks for %lld", what,
                    (long long)scratch_bytes, (long long)plan.scratch_bytes);
  return 0;
}

int count_check(const void* planes, int dtype, int n, int height, int width, const void* scratch, int64_t scratch_bytes,
                const int32_t* n_out, const int64_t* base, const int64_t* total, const int64_t* first, const int32_t* stats,
                struct deva_runs_plan* plan) {
  const char* what = "deva_runs_count";
  struct deva_runs_plan local;
  if (!plan) plan = &local;
  DEVA_RUNS_REQUIRE(dtype == DEVA_RUNS_U8 || dtype == DEVA_RUNS_F32, "%s: dtype must be DEVA_RUNS_U8 or DEVA_RUNS_F32 (got %d)", what, dtype);
  if (int rc = runs_plan(what, n, height, width, plan)) return rc;
  if (n == 0) return 0;
  const int64_t plane_bytes = (int64_t)n * height * width * element_bytes(dtype);
  DEVA_RUNS_REQUIRE(planes && aligned(planes, element_bytes(dtype)), "%s: planes: null or misaligned", what);
  if (int rc = scratch_check(what, scratch, scratch_bytes, *plan)) return rc;
  DEVA_RUNS_REQUIRE(n_out && aligned(n_out, 4), "%s: n_out: null or misaligned", what);
  DEVA_RUNS_REQUIRE(base && aligned(base, 8), "%s: base: null or misaligned", what);
  DEVA_RUNS_REQUIRE(total && aligned(total, 8), "%s: total: null or misaligned", what);
  DEVA_RUNS_REQUIRE(aligned(first, 8), "%s: first: misaligned", what);
  DEVA_RUNS_REQUIRE(aligned(stats, 4), "%s: stats: misaligned", what);
  DEVA_RUNS_REQUIRE(first != total, "%s: first: it must not be `total` itself", what);
  const struct { const char* name; const void* p; int64_t bytes; } outs[] = {
      {"scratch", scratch, plan->scratch_bytes}, {"n_out", n_out, 4ll * n}, {"base", base, 8ll * n},
      {"total", total, 8},                       {"stats", stats, 20ll * n}};
  for (const auto& o : outs) {
    DEVA_RUNS_REQUIRE(!overlaps(o.p, o.bytes, planes, plane_bytes), "%s: %s overlaps the planes", what, o.name);
    DEVA_RUNS_REQUIRE(!overlaps(o.p, o.bytes, first, 8), "%s: %s overlaps first", what, o.name);
    for (const auto& q : outs)
      DEVA_RUNS_REQUIRE(&o == &q || !overlaps(o.p, o.bytes, q.p, q.bytes), "%s: %s overlaps %s", what, o.name, q.name);
  }
  return 0;
}

int write_check(int n, int height, int width, const void* scratch, int64_t scratch_bytes, const int64_t* base, const int32_t* bounds,
                int64_t capacity, struct deva_runs_plan* plan) {
  const char* what = "deva_runs_write";
  struct deva_runs_plan local;
  if (!plan) plan = &local;
  if (int rc = runs_plan(what, n, height, width, plan)) return rc;
  DEVA_RUNS_REQUIRE(capacity >= 0, "%s: capacity: negative (%lld)", what, (long long)capacity);
  if (n == 0) return 0;
  if (int rc = scratch_check(what, scratch, scratch_bytes, *plan)) return rc;
  DEVA_RUNS_REQUIRE(base && aligned(base, 8), "%s: base: null or misaligned", what);
  DEVA_RUNS_REQUIRE((bounds || capacity == 0) && aligned(bounds, 4), "%s: bounds: null or misaligned", what);
  DEVA_RUNS_REQUIRE(capacity <= (1ll << 60), "%s: capacity: above 2^60 (%lld)", what, (long long)capacity);
  DEVA_RUNS_REQUIRE(!overlaps(bounds, 4 * capacity, scratch, plan->scratch_bytes), "%s: bounds overlaps scratch", what);
  DEVA_RUNS_REQUIRE(!overlaps(bounds, 4 * capacity, base, 8ll * n), "%s: bounds overlaps base", what);
  return 0;
}

}  // namespace deva_runs

extern "C" int deva_runs_version(void) { return DEVA_RUNS_ABI_VERSION; }
extern "C" const char* deva_runs_last_error(void) { return deva_runs::last_error(); }
extern "C" int deva_runs_limits(struct deva_runs_limits* limits) {
  DEVA_RUNS_REQUIRE(limits, "deva_runs_limits: null limits");
  limits->max_masks = DEVA_RUNS_MAX_MASKS;
  limits->tile = deva_runs::kTile;
  limits->block = deva_runs::kBlock;
  limits->scan_chunk = DEVA_RUNS_SCAN_CHUNK;
  limits->mask_chunk = DEVA_RUNS_MASK_CHUNK;
  limits->reserved = 0;
  limits->max_scratch = DEVA_RUNS_MAX_SCRATCH;
  return 0;
}
extern "C" int deva_runs_plan(int n, int height, int width, struct deva_runs_plan* plan) {
  return deva_runs::runs_plan("deva_runs_plan", n, height, width, plan);
}
extern "C" int64_t deva_runs_scratch(int n, int height, int width) {
  struct deva_runs_plan plan;
  return deva_runs::runs_plan("deva_runs_scratch", n, height, width, &plan) ? -1 : plan.scratch_bytes;
}
