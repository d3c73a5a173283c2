// Stand-alone host program for tests/test_plan_sanitize_cpu.py: the HIP-free side of the joint count
// (csrc/metrics/panoptic_plan.cpp: every argument check of deva_metrics_panoptic_counts and the launch decision behind
// deva_metrics_panoptic_plan) walked over the product of its boundary values under the host sanitizers.  Addresses are
// made up: nothing is dereferenced.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <initializer_list>

#include "deva_metrics.h"
#include "panoptic_plan.h"

static long g_calls = 0, g_refused = 0, g_failed = 0;

static void fail(const char* what, long a, long b, long c, long d) {
  ++g_failed;
  fprintf(stderr, "FAIL %s: %ld %ld %ld %ld (%s)\n", what, a, b, c, d, deva_metrics_last_error());
}

static void tally(int e, bool want, const char* entry, const char* what, long a, long b, long c, long d) {
  ++g_calls;
  if (e != 0) ++g_refused;
  if ((e == 0) != want) fail(what, a, b, c, d);
  if (e != 0 && (e != 2 || !strstr(deva_metrics_last_error(), entry))) fail("refusal text", a, b, c, d);
  deva_metrics::set_error("%s", "");
}

int main() {
  using namespace deva_metrics;
  const int sides[] = {-2147483647 - 1, -1, 0, 1, 2, 3, 7, 13, 15, 16, 17, 47, 255, 256, 257, 720, 1080, 1280, 1920, 4095,
                       4096, 4097, 32767, 32768, 32769, 46341, 65536, 1 << 30, (1 << 30) + 1, 2147483647};
  const int ids[] = {-2147483647 - 1, -1, 0, 1, 2, 40, 100, 125, 126, 127, 253, 254, 255, 510, 1021, 1022, 1023, 2147483647};
  const auto at = [](int64_t off) { return reinterpret_cast<const void*>((uintptr_t(1) << 40) + off); };
  const void *GT = at(0), *GI = at(int64_t(1) << 36), *PR = at(int64_t(2) << 36), *PI = at(int64_t(3) << 36),
             *LUT = at(int64_t(4) << 36), *OUT = at(int64_t(5) << 36);

  // the plan: sizes x table lengths
  for (int h : sides)
    for (int w : sides) {
      const bool size_ok = h > 0 && w > 0 && (int64_t)h * w <= kMaxPixels;
      for (int ng : ids)
        for (int np : ids) {
          const bool n_ok = ng >= 0 && ng <= DEVA_METRICS_MAX_IDS && np >= 0 && np <= DEVA_METRICS_MAX_IDS;
          deva_metrics_plan plan = {-1, 0, 0, 0};
          const int e = deva_metrics_panoptic_plan(h, w, ng, np, &plan);
          tally(e, size_ok && n_ok, "deva_metrics_panoptic_plan", "plan", h, w, ng, np);
          if (e != 0) continue;
          const int64_t pixels = (int64_t)h * w, strips = (pixels + DEVA_METRICS_STRIP - 1) / DEVA_METRICS_STRIP;
          const int64_t bins = (int64_t)(ng + 2) * (np + 2), tables = 4ll * (ng + np);
          const bool lds = 4 * bins + tables <= DEVA_METRICS_LDS_LIMIT;
          // one lane per strip up to the grid cap, never an idle workgroup, the LDS of the launch inside the limit
          if (plan.block != (uint32_t)kBlock || plan.grid < 1 || plan.grid > (uint32_t)kMaxGrid) fail("grid", h, w, plan.grid, plan.block);
          if ((int64_t)(plan.grid - 1) * kBlock >= strips) fail("idle workgroup", h, w, plan.grid, strips);
          if (plan.grid < (uint32_t)kMaxGrid && (int64_t)plan.grid * kBlock < strips) fail("uncovered", h, w, plan.grid, strips);
          if (plan.path != (lds ? DEVA_METRICS_PATH_LDS : DEVA_METRICS_PATH_GLOBAL)) fail("path", ng, np, plan.path, 0);
          if (plan.lds_bytes != (uint64_t)(tables + (lds ? 4 * bins : 0)) || plan.lds_bytes > DEVA_METRICS_LDS_LIMIT)
            fail("lds", ng, np, plan.lds_bytes, 0);
          // the same decision through the checks of the launch, for every pair of encodings
          for (int ge : {-1, 0, 1, 2, 3, 4})
            for (int pe : {-1, 0, 1, 2, 3, 4}) {
              deva_metrics_plan again = {-1, 0, 0, 0};
              const bool enc_ok = (ge == 0 || ge == 1) && pe >= 0 && pe <= 3;
              const int e2 = panoptic_counts_check(GT, ge, GI, ng, PR, pe, PI, np, LUT, 9, h, w, OUT, &again);
              tally(e2, enc_ok, "deva_metrics_panoptic_counts", "check", h, w, ge, pe);
              if (e2 == 0 && memcmp(&again, &plan, sizeof(plan)) != 0) fail("two plans", h, w, ng, np);
            }
        }
    }
  tally(deva_metrics_panoptic_plan(8, 8, 1, 1, nullptr), false, "deva_metrics_panoptic_plan", "null plan", 0, 0, 0, 0);

  // the pointers, one at a time on an otherwise good call: null, alignment, overlap with the output
  struct { const void *gt, *gi; int ng; const void *pr; int pe; const void *pi; int np; const void* lut; int ch; const void* out; bool ok; } one[] = {
      {GT, GI, 3, PR, 0, PI, 4, nullptr, 0, OUT, true},    {nullptr, GI, 3, PR, 0, PI, 4, nullptr, 0, OUT, false},
      {at(4), GI, 3, PR, 0, PI, 4, nullptr, 0, OUT, false}, {at(16), GI, 3, PR, 0, PI, 4, nullptr, 0, OUT, true},
      {GT, nullptr, 3, PR, 0, PI, 4, nullptr, 0, OUT, false}, {GT, nullptr, 0, PR, 0, PI, 4, nullptr, 0, OUT, true},
      {GT, at(2), 3, PR, 0, PI, 4, nullptr, 0, OUT, false}, {GT, GI, 3, nullptr, 0, PI, 4, nullptr, 0, OUT, false},
      {GT, GI, 3, at((int64_t(2) << 36) + 8), 2, PI, 4, nullptr, 0, OUT, false}, {GT, GI, 3, PR, 2, nullptr, 4, nullptr, 0, OUT, false},
      {GT, GI, 3, PR, 2, nullptr, 0, nullptr, 0, OUT, true}, {GT, GI, 3, PR, 1, at((int64_t(3) << 36) + 1), 4, nullptr, 0, OUT, false},
      {GT, GI, 3, PR, 3, nullptr, 4, LUT, 9, OUT, true},   {GT, GI, 3, PR, 3, nullptr, 4, nullptr, 9, OUT, false},
      {GT, GI, 3, PR, 3, nullptr, 4, at((int64_t(4) << 36) + 1), 9, OUT, false}, {GT, GI, 3, PR, 3, nullptr, 4, LUT, 0, OUT, false},
      {GT, GI, 3, PR, 3, nullptr, 4, LUT, 32767, OUT, true}, {GT, GI, 3, PR, 3, nullptr, 4, LUT, 32768, OUT, false},
      {GT, GI, 3, PR, 3, PI, 4, LUT, -1, OUT, false},      {GT, GI, 3, PR, 0, PI, 4, nullptr, 0, nullptr, false},
      {GT, GI, 3, PR, 0, PI, 4, nullptr, 0, at((int64_t(5) << 36) + 2), false}, {GT, GI, 3, PR, 0, PI, 4, nullptr, 0, at(29 * 53 * 3 - 7), false},
      {GT, GI, 3, PR, 0, PI, 4, nullptr, 0, at(29 * 53 * 3 + 1), true}, {GT, GI, 3, PR, 0, PI, 4, nullptr, 0, at((int64_t(1) << 36) + 8), false},
      {GT, GI, 3, PR, 0, PI, 4, nullptr, 0, at((int64_t(1) << 36) + 12), true}, {GT, GI, 3, PR, 0, PI, 4, nullptr, 0, at((int64_t(3) << 36) - 120), true},
      {GT, GI, 3, PR, 0, PI, 4, nullptr, 0, at((int64_t(3) << 36) - 116), false}, {GT, GI, 3, PR, 3, PI, 4, LUT, 9, at((int64_t(3) << 36) + 4), true},
      {GT, GI, 3, PR, 3, nullptr, 4, LUT, 9, at((int64_t(4) << 36) + 16), false}, {GT, GI, 3, OUT, 2, PI, 4, nullptr, 0, OUT, false}};
  long k = 0;
  for (const auto& c : one)
    tally(panoptic_counts_check(c.gt, 0, c.gi, c.ng, c.pr, c.pe, c.pi, c.np, c.lut, c.ch, 29, 53, c.out, nullptr), c.ok,
          "deva_metrics_panoptic_counts", "single", k++, 0, 0, 0);
  printf("%ld checks (%ld refused), %ld failures\n", g_calls, g_refused, g_failed);
  return g_failed ? 1 : 0;
}
