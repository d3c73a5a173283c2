// Stand-alone host program for tests/test_vos_quality_cpu.py: the HIP-free side of the DAVIS counts
// (csrc/vos_metrics/boundary_plan.cpp: the radius rule, every argument check of deva_vos_boundary_counts and the launch
// decision behind deva_vos_boundary_plan) walked over the product of its boundary values under the host sanitizers.
// Addresses are made up: nothing is dereferenced.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <initializer_list>
#include <limits>

#include "boundary_plan.h"
#include "deva_vos_metrics.h"

static long g_calls = 0, g_refused = 0, g_failed = 0;

static void fail(const char* what, long a, long b, long c, long d) {
  ++g_failed;
  fprintf(stderr, "FAIL %s: %ld %ld %ld %ld (%s)\n", what, a, b, c, d, deva_vos_last_error());
}

static void tally(int e, bool want, const char* entry, const char* what, long a, long b, long c, long d) {
  ++g_calls;
  if (e != 0) ++g_refused;
  if ((e == 0) != want) fail(what, a, b, c, d);
  if (e != 0 && (e != 2 || !strstr(deva_vos_last_error(), entry))) fail("refusal text", a, b, c, d);
  deva_vos::set_error("%s", "");
}

int main() {
  using namespace deva_vos;
  const int sides[] = {-2147483647 - 1, -1, 0, 1, 2, 3, 7, 8, 9, 63, 64, 65, 255, 256, 257, 480, 854, 1080, 1920, 4095,
                       4096, 32767, 32768, 32769, 46341, 65536, 1 << 30, (1 << 30) + 1, 2147483647};
  const int objects[] = {-2147483647 - 1, -1, 0, 1, 2, 5, 63, 64, 65, 2147483647};
  const int radii[] = {-2147483647 - 1, -1, 0, 1, 2, 3, 4, 8, 36, 127, 128, 129, 2147483647};
  const auto at = [](int64_t off) { return reinterpret_cast<const void*>((uintptr_t(1) << 44) + off); };
  const void *GT = at(0), *PR = at(int64_t(1) << 40), *IDS = at(int64_t(2) << 40), *LUT = at(int64_t(3) << 40),
             *SCR = at(int64_t(4) << 40), *OUT = at(int64_t(6) << 40);

  // the plan: sizes x objects x radii, and the same decision through the checks of the launch for every pair of encodings
  for (int h : sides)
    for (int w : sides) {
      const bool size_ok = h > 0 && w > 0 && (int64_t)h * w <= kMaxPixels;
      int64_t bytes = -1;
      tally(deva_vos_boundary_scratch_bytes(h, w, &bytes), size_ok, "deva_vos_boundary_scratch_bytes", "scratch", h, w, 0, 0);
      if (size_ok && bytes != (int64_t)h * w * kWordBytes) fail("scratch bytes", h, w, bytes, 0);
      for (int n : objects)
        for (int r : radii) {
          const bool ok = size_ok && n >= 1 && n <= DEVA_VOS_MAX_OBJECTS && r >= 0 && r <= DEVA_VOS_MAX_RADIUS;
          deva_vos_plan plan;
          memset(&plan, 0xff, sizeof(plan));
          const int e = deva_vos_boundary_plan(h, w, n, r, &plan);
          tally(e, ok, "deva_vos_boundary_plan", "plan", h, w, n, r);
          if (e != 0) continue;
          const int64_t pixels = (int64_t)h * w, strips = (int64_t)h * (((int64_t)w + DEVA_VOS_STRIP - 1) / DEVA_VOS_STRIP);
          const int64_t chunks = (pixels + kWave - 1) / kWave, per = kBlock / kWave;
          // a lane per strip and a wave per 64 pixels up to the grid cap, never an idle workgroup
          if (plan.block != (uint32_t)kBlock || plan.label_grid < 1 || plan.label_grid > (uint32_t)kMaxGrid || plan.match_grid < 1 ||
              plan.match_grid > (uint32_t)kMaxMatchGrid)
            fail("grid", h, w, plan.label_grid, plan.match_grid);
          if ((int64_t)(plan.label_grid - 1) * kBlock >= strips || (int64_t)(plan.match_grid - 1) * per >= chunks)
            fail("idle workgroup", h, w, plan.label_grid, plan.match_grid);
          if ((plan.label_grid < (uint32_t)kMaxGrid && (int64_t)plan.label_grid * kBlock < strips) ||
              (plan.match_grid < (uint32_t)kMaxMatchGrid && (int64_t)plan.match_grid * per < chunks))
            fail("uncovered", h, w, plan.label_grid, plan.match_grid);
          if (plan.lds_bytes != 16u * (uint32_t)n || plan.radius != r || plan.inner_radius != (r < DEVA_VOS_INNER_RADIUS ? r : DEVA_VOS_INNER_RADIUS) ||
              plan.scratch_bytes != pixels * kWordBytes)
            fail("plan fields", h, w, n, r);
          if (r != 8) continue;
          for (int ge : {-1, 0, 1, 2, 3, 4, 256, 257, 258, 512})
            for (int pe : {-1, 0, 1, 2, 3, 4, 256, 259, 260, 512}) {
              deva_vos_plan again;
              memset(&again, 0xff, sizeof(again));
              const bool enc_ok = (ge == 0 || ge == 1 || ge == 256 || ge == 257) && ((pe >= 0 && pe <= 3) || pe == 256 || pe == 259);
              const bool binary_ok = (ge < 256 && pe < 256) || n == 1;
              const int e2 = boundary_counts_check(GT, ge, PR, pe, IDS, n, LUT, 9, h, w, r, SCR, plan.scratch_bytes, OUT, &again);
              tally(e2, enc_ok && binary_ok, "deva_vos_boundary_counts", "check", h, w, ge, pe);
              if (e2 == 0 && memcmp(&again, &plan, sizeof(plan)) != 0) fail("two plans", h, w, n, r);
            }
        }
    }
  tally(deva_vos_boundary_plan(8, 8, 1, 1, nullptr), false, "deva_vos_boundary_plan", "null plan", 0, 0, 0, 0);
  tally(deva_vos_boundary_scratch_bytes(8, 8, nullptr), false, "deva_vos_boundary_scratch_bytes", "null bytes", 0, 0, 0, 0);

  // R3: the radius over sizes x thresholds, against the rule written out again
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  const double ths[] = {-inf, -1.0, -1e-300, 0.0, 1e-300, 0.001, 0.008, 0.5, 0.999999, 1.0, 1.5, 2.0, 8.0, 128.0, 128.5, 129.0, 1e18, inf, nan};
  for (int h : sides)
    for (int w : sides)
      for (int t = 0; t < (int)(sizeof(ths) / sizeof(ths[0])); ++t) {
        const double th = ths[t];
        const bool size_ok = h > 0 && w > 0 && (int64_t)h * w <= kMaxPixels;
        bool ok = size_ok && th >= 0.0 && th <= 1e300;
        double want = 0.0;
        if (ok) {
          if (th >= 1.0) ok = th == floor(th), want = th;
          else want = ceil(th * sqrt((double)((int64_t)h * h + (int64_t)w * w)));
          ok = ok && want <= 128.0;
        }
        int r = -7;
        tally(deva_vos_boundary_radius(h, w, th, &r), ok, "deva_vos_boundary_radius", "radius", h, w, t, 0);
        if (ok && r != (int)want) fail("radius value", h, w, r, (long)want);
        if (!ok && r != -7) fail("radius written on refusal", h, w, r, 0);
      }
  tally(deva_vos_boundary_radius(8, 8, 0.008, nullptr), false, "deva_vos_boundary_radius", "null radius", 0, 0, 0, 0);

  // the pointers, one at a time on an otherwise good call (29 x 53, 3 objects): null, alignment, size, overlap
  const int64_t need = 29 * 53 * 16;
  struct { const void *gt, *pr; int pe; const void* ids; const void* lut; int ch; const void* scr; int64_t bytes; const void* out; bool ok; } one[] = {
      {GT, PR, 0, IDS, nullptr, 0, SCR, need, OUT, true},          {nullptr, PR, 0, IDS, nullptr, 0, SCR, need, OUT, false},
      {at(4), PR, 0, IDS, nullptr, 0, SCR, need, OUT, false},      {at(16), PR, 0, IDS, nullptr, 0, SCR, need, OUT, true},
      {GT, nullptr, 0, IDS, nullptr, 0, SCR, need, OUT, false},    {GT, at((int64_t(1) << 40) + 8), 2, IDS, nullptr, 0, SCR, need, OUT, false},
      {GT, PR, 0, nullptr, nullptr, 0, SCR, need, OUT, false},     {GT, PR, 0, at((int64_t(2) << 40) + 2), nullptr, 0, SCR, need, OUT, false},
      {GT, PR, 3, IDS, LUT, 9, SCR, need, OUT, true},              {GT, PR, 3, IDS, nullptr, 9, SCR, need, OUT, false},
      {GT, PR, 3, IDS, at((int64_t(3) << 40) + 1), 9, SCR, need, OUT, false}, {GT, PR, 3, IDS, LUT, 0, SCR, need, OUT, false},
      {GT, PR, 3, IDS, LUT, 32767, SCR, need, OUT, true},          {GT, PR, 3, IDS, LUT, 32768, SCR, need, OUT, false},
      {GT, PR, 3, IDS, LUT, -1, SCR, need, OUT, false},            {GT, PR, 0, IDS, nullptr, 0, nullptr, need, OUT, false},
      {GT, PR, 0, IDS, nullptr, 0, at((int64_t(4) << 40) + 8), need, OUT, false}, {GT, PR, 0, IDS, nullptr, 0, SCR, need - 1, OUT, false},
      {GT, PR, 0, IDS, nullptr, 0, SCR, need + 1, OUT, true},      {GT, PR, 0, IDS, nullptr, 0, SCR, -1, OUT, false},
      {GT, PR, 0, IDS, nullptr, 0, SCR, need, nullptr, false},     {GT, PR, 0, IDS, nullptr, 0, SCR, need, at((int64_t(6) << 40) + 2), false},
      {GT, PR, 0, IDS, nullptr, 0, SCR, need, at(29 * 53 - 1), false}, {GT, PR, 0, IDS, nullptr, 0, SCR, need, at(29 * 53 + 3), true},
      {GT, PR, 0, IDS, nullptr, 0, SCR, need, at((int64_t(2) << 40) + 8), false}, {GT, PR, 0, IDS, nullptr, 0, SCR, need, at((int64_t(2) << 40) + 12), true},
      {GT, PR, 0, IDS, nullptr, 0, SCR, need, at((int64_t(1) << 40) - 96), true}, {GT, PR, 0, IDS, nullptr, 0, SCR, need, at((int64_t(1) << 40) - 92), false},
      {GT, PR, 3, IDS, LUT, 9, SCR, need, at((int64_t(3) << 40) + 16), false}, {GT, PR, 0, IDS, nullptr, 0, SCR, need, at((int64_t(3) << 40) + 16), true},
      {GT, PR, 0, IDS, nullptr, 0, SCR, need, at((int64_t(4) << 40) + need - 4), false}, {GT, PR, 0, IDS, nullptr, 0, SCR, need, at((int64_t(4) << 40) + need), true},
      {GT, OUT, 2, IDS, nullptr, 0, SCR, need, OUT, false},        {GT, PR, 0, IDS, nullptr, 0, at(1536), need, OUT, false},
      {GT, PR, 0, IDS, nullptr, 0, at(1552), need, OUT, true}};
  long k = 0;
  for (const auto& c : one)
    tally(boundary_counts_check(c.gt, 0, c.pr, c.pe, c.ids, 3, c.lut, c.ch, 29, 53, 8, c.scr, c.bytes, c.out, nullptr), c.ok,
          "deva_vos_boundary_counts", "single", k++, 0, 0, 0);
  printf("%ld checks (%ld refused), %ld failures\n", g_calls, g_refused, g_failed);
  return g_failed ? 1 : 0;
}
