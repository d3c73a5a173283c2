// Stand-alone host program for tests/test_unsup_quality_cpu.py: the HIP-free side of the pair counts
// (csrc/pair_metrics/pair_plan.cpp: every argument check of deva_pair_counts and the launch decision behind
// deva_pair_plan) walked over the product of its boundary values under the host sanitizers.
// Addresses are made up: nothing is dereferenced.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <initializer_list>

#include "deva_pair_metrics.h"
#include "pair_plan.h"

static long g_calls = 0, g_refused = 0, g_failed = 0;

static void fail(const char* what, long a, long b, long c, long d) {
  ++g_failed;
  fprintf(stderr, "FAIL %s: %ld %ld %ld %ld (%s)\n", what, a, b, c, d, deva_pair_last_error());
}

static void tally(int e, bool want, const char* entry, const char* what, long a, long b, long c, long d) {
  ++g_calls;
  if (e != 0) ++g_refused;
  if ((e == 0) != want) fail(what, a, b, c, d);
  if (e != 0 && (e != 2 || !strstr(deva_pair_last_error(), entry))) fail("refusal text", a, b, c, d);
  deva_pair::set_error("%s", "");
}

int main() {
  using namespace deva_pair;
  const int sides[] = {-2147483647 - 1, -1, 0, 1, 2, 7, 8, 9, 63, 64, 65, 257, 480, 854, 1920, 4096, 32767, 32768, 32769,
                       46341, 65536, 1 << 30, (1 << 30) + 1, 2147483647};
  const int objects[] = {-2147483647 - 1, -1, 0, 1, 2, 5, 20, 63, 64, 65, 2147483647};
  const int radii[] = {-2147483647 - 1, -1, 0, 1, 3, 4, 8, 36, 128, 129, 2147483647};
  const auto at = [](int64_t off) { return reinterpret_cast<const void*>((uintptr_t(1) << 44) + off); };
  const void *GT = at(0), *PR = at(int64_t(1) << 40), *GIDS = at(int64_t(2) << 40), *PIDS = at((int64_t(2) << 40) + (1 << 20)),
             *LUT = at(int64_t(3) << 40), *SCR = at(int64_t(4) << 40), *ONE = at(int64_t(6) << 40), *TWO = at(int64_t(7) << 40);

  // the plan: sizes x tables x radii, and the same decision through the checks of the launch for every pair of encodings
  for (int h : sides)
    for (int w : sides) {
      const bool size_ok = h > 0 && w > 0 && (int64_t)h * w <= kMaxPixels;
      int64_t bytes = -1;
      tally(deva_pair_scratch_bytes(h, w, &bytes), size_ok, "deva_pair_scratch_bytes", "scratch", h, w, 0, 0);
      if (size_ok && bytes != (int64_t)h * w * kWordBytes) fail("scratch bytes", h, w, bytes, 0);
      for (int ng : objects)
        for (int np : objects)
          for (int r : radii) {
            const bool ok = size_ok && ng >= 1 && ng <= DEVA_PAIR_MAX_OBJECTS && np >= 1 && np <= DEVA_PAIR_MAX_OBJECTS && r >= 0 &&
                            r <= DEVA_PAIR_MAX_RADIUS;
            struct deva_pair_plan plan;
            memset(&plan, 0xff, sizeof(plan));
            const int e = deva_pair_plan(h, w, ng, np, r, &plan);
            tally(e, ok, "deva_pair_plan", "plan", h, w, (long)ng * 1000 + np, r);
            if (e != 0) continue;
            const int64_t pixels = (int64_t)h * w, strips = (int64_t)h * (((int64_t)w + DEVA_PAIR_STRIP - 1) / DEVA_PAIR_STRIP);
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
            if (plan.label_lds_bytes != 4u * (2u * (uint32_t)(ng + np) + (uint32_t)ng * (uint32_t)np) ||
                plan.match_lds_bytes != 4u * (128u + 2u * (uint32_t)ng * (uint32_t)np) || plan.match_lds_bytes > 160u * 1024u || plan.radius != r ||
                plan.inner_radius != (r < DEVA_PAIR_INNER_RADIUS ? r : DEVA_PAIR_INNER_RADIUS) ||
                plan.wave_search != (r > DEVA_PAIR_INNER_RADIUS ? 1 : 0) || plan.scratch_bytes != pixels * kWordBytes)
              fail("plan fields", h, w, (long)ng * 1000 + np, r);
            if (r != 8 || ng > 5) continue;
            for (int ge : {-1, 0, 1, 2, 3, 4, 256, 257, 512})
              for (int pe : {-1, 0, 1, 2, 3, 4, 256, 259, 512}) {
                struct deva_pair_plan again;
                memset(&again, 0xff, sizeof(again));
                const bool enc_ok = (ge == 0 || ge == 1) && pe >= 0 && pe <= 3;   // no binary form
                const int e2 = pair_counts_check(GT, ge, GIDS, ng, PR, pe, PIDS, np, LUT, 9, h, w, r, SCR, plan.scratch_bytes, ONE, TWO, &again);
                tally(e2, enc_ok, "deva_pair_counts", "check", h, w, ge, pe);
                if (e2 == 0 && memcmp(&again, &plan, sizeof(plan)) != 0) fail("two plans", h, w, ng, np);
              }
          }
    }
  tally(deva_pair_plan(8, 8, 1, 1, 1, nullptr), false, "deva_pair_plan", "null plan", 0, 0, 0, 0);
  tally(deva_pair_scratch_bytes(8, 8, nullptr), false, "deva_pair_scratch_bytes", "null bytes", 0, 0, 0, 0);

  // the pointers, one at a time on an otherwise good call (29 x 53, 3 objects, 5 proposals): null, alignment, size, overlap
  const int64_t need = 29 * 53 * 16, G = int64_t(1) << 40;
  struct Case { const void *gt, *pr; int pe; const void *gids, *pids, *lut; int ch; const void* scr; int64_t bytes; const void *one, *two; bool ok; };
  const Case good = {GT, PR, 0, GIDS, PIDS, nullptr, 0, SCR, need, ONE, TWO, true};
  const auto with = [&](auto edit, bool ok) { Case c = good; edit(c); c.ok = ok; return c; };
  const Case one[] = {
      good,
      with([&](Case& c) { c.gt = nullptr; }, false), with([&](Case& c) { c.gt = at(4); }, false), with([&](Case& c) { c.gt = at(16); }, true),
      with([&](Case& c) { c.pr = nullptr; }, false), with([&](Case& c) { c.pr = at(G + 8); c.pe = 2; }, false),
      with([&](Case& c) { c.gids = nullptr; }, false), with([&](Case& c) { c.gids = at(2 * G + 2); }, false),
      with([&](Case& c) { c.pids = nullptr; }, false), with([&](Case& c) { c.pids = at(2 * G + (1 << 20) + 2); }, false),
      with([&](Case& c) { c.pe = 3; c.lut = LUT; c.ch = 9; }, true),
      with([&](Case& c) { c.pe = 3; c.lut = LUT; c.ch = 9; c.pids = nullptr; }, true),      // pred_ids is not read with the channel plane
      with([&](Case& c) { c.pe = 3; c.lut = nullptr; c.ch = 9; }, false), with([&](Case& c) { c.pe = 3; c.lut = at(3 * G + 1); c.ch = 9; }, false),
      with([&](Case& c) { c.pe = 3; c.lut = LUT; c.ch = 0; }, false), with([&](Case& c) { c.pe = 3; c.lut = LUT; c.ch = 32767; }, true),
      with([&](Case& c) { c.pe = 3; c.lut = LUT; c.ch = 32768; }, false), with([&](Case& c) { c.pe = 3; c.lut = LUT; c.ch = -1; }, false),
      with([&](Case& c) { c.scr = nullptr; }, false), with([&](Case& c) { c.scr = at(4 * G + 8); }, false),
      with([&](Case& c) { c.bytes = need - 1; }, false), with([&](Case& c) { c.bytes = need + 1; }, true), with([&](Case& c) { c.bytes = -1; }, false),
      with([&](Case& c) { c.one = nullptr; }, false), with([&](Case& c) { c.one = at(6 * G + 2); }, false),
      with([&](Case& c) { c.two = nullptr; }, false), with([&](Case& c) { c.two = at(7 * G + 2); }, false),
      // singles is 4 * 2 * 8 = 64 bytes, pairs 4 * 4 * 15 = 240
      with([&](Case& c) { c.one = at(1536); }, false), with([&](Case& c) { c.one = at(1540); }, true),
      with([&](Case& c) { c.two = at(1536); }, false),
      with([&](Case& c) { c.one = at(2 * G + 8); }, false), with([&](Case& c) { c.one = at(2 * G + 12); }, true),
      with([&](Case& c) { c.two = at(2 * G + (1 << 20) + 16); }, false), with([&](Case& c) { c.two = at(2 * G + (1 << 20) + 20); }, true),
      with([&](Case& c) { c.pe = 3; c.lut = LUT; c.ch = 9; c.two = at(2 * G + (1 << 20) + 16); }, true),   // the unread table may be anywhere
      with([&](Case& c) { c.one = at(G - 64); }, true), with([&](Case& c) { c.one = at(G - 60); }, false),
      with([&](Case& c) { c.pe = 3; c.lut = LUT; c.ch = 9; c.one = at(3 * G + 16); }, false), with([&](Case& c) { c.one = at(3 * G + 16); }, true),
      with([&](Case& c) { c.one = at(4 * G + need - 4); }, false), with([&](Case& c) { c.one = at(4 * G + need); }, true),
      with([&](Case& c) { c.two = at(4 * G + need - 4); }, false), with([&](Case& c) { c.two = at(4 * G + need); }, true),
      with([&](Case& c) { c.two = at(6 * G + 60); }, false), with([&](Case& c) { c.two = at(6 * G + 64); }, true),
      with([&](Case& c) { c.one = at(7 * G + 236); }, false), with([&](Case& c) { c.one = at(7 * G + 240); }, true),
      with([&](Case& c) { c.pr = ONE; c.pe = 2; }, false), with([&](Case& c) { c.scr = at(1536); }, false), with([&](Case& c) { c.scr = at(1552); }, true)};
  long k = 0;
  for (const Case& c : one)
    tally(pair_counts_check(c.gt, 0, c.gids, 3, c.pr, c.pe, c.pids, 5, c.lut, c.ch, 29, 53, 8, c.scr, c.bytes, c.one, c.two, nullptr), c.ok,
          "deva_pair_counts", "single", k++, 0, 0, 0);
  printf("%ld checks (%ld refused), %ld failures\n", g_calls, g_refused, g_failed);
  return g_failed ? 1 : 0;
}
