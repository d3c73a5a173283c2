// Stand-alone host program for tests/test_plan_sanitize_cpu.py: the HIP-free side of the prompt-point choice
// (csrc/prompt_plan.cpp: the argument checks of deva_prompt_points, the scratch layout and deva_prompt_scratch) walked
// over the product of its boundary values under the host sanitizers.  Addresses are made up: nothing is dereferenced.
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <initializer_list>

#include "deva_hip.h"
#include "prompt_plan.h"

namespace deva {
static char g_err[512];
void set_error(const char* fmt, ...) {  // (the library's lives in runtime.hip)
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
}  // namespace deva

static long g_calls = 0, g_refused = 0, g_failed = 0;

static void fail(const char* what, int h, int w, int n, int elem) {
  ++g_failed;
  fprintf(stderr, "FAIL %s: %dx%d points=%d elem=%d (%s)\n", what, h, w, n, elem, deva::g_err);
}

static void tally(int e, bool want, const char* what, int h, int w, int n, int elem) {
  ++g_calls;
  if (e != 0) ++g_refused;
  if ((e == 0) != want) fail(what, h, w, n, elem);
  if (e != 0 && (e != 2 || !strstr(deva::g_err, "deva_prompt_points"))) fail("refusal text", h, w, n, elem);
  deva::g_err[0] = 0;
}

int main() {
  using namespace deva;
  const int sides[] = {-2147483647 - 1, -1, 0, 1, 15, 16, 17, 31, 32, 33, 96, 853, 1080, 1920, 16384, 32768, 32769,
                       46341, 65535, 65536, 65537, 1 << 30, 2147483647};
  const int counts[] = {-2147483647 - 1, -1, 0, 1, 9, 63, 64, 65, 1023, 1024, 1025, 16383, 16384, 16385, 1 << 30, 2147483647};
  const int elems[] = {-8, -1, 0, 1, 2, 4, 7, 8, 9, 16, 2147483647};
  const void* P = reinterpret_cast<const void*>(uintptr_t(1) << 40);
  const double nan = 0.0 / 0.0;
  for (int h : sides)
    for (int w : sides) {
      const bool size_ok = h >= 16 && w >= 16 && h <= kPromptMaxSide && w <= kPromptMaxSide && (int64_t)h * w <= kPromptMaxPixels;
      if (prompt_size_ok(h, w) != size_ok) fail("size_ok", h, w, 0, 0);
      int64_t bytes = -1;
      if (size_ok) {
        const PromptPlan p = prompt_plan(h, w);
        bytes = p.bytes;
        const bool ok = p.low_h == h / 16 && p.low_w == w / 16 && p.low_h >= 1 && p.low_w >= 1 && p.off_rows == 0 &&
                        p.off_low % 256 == 0 && p.bytes % 256 == 0 && p.off_low - p.off_rows >= (int64_t)h * p.low_w * 4 &&
                        p.bytes - p.off_low >= (int64_t)p.low_h * p.low_w * 4 &&
                        p.bytes < (int64_t)(h + p.low_h) * p.low_w * 4 + 512;
        if (!ok) fail("layout", h, w, 0, 0);
      }
      for (int n : counts) {
        const bool n_ok = n >= 1 && n <= kPromptMaxPoints;
        if (prompt_points_ok(n) != n_ok) fail("points_ok", h, w, n, 0);
        const int64_t asked = deva_prompt_scratch(h, w, n);
        if (asked != (size_ok && n_ok ? bytes : -1)) fail("deva_prompt_scratch", h, w, n, 0);
        for (int elem : elems)
          for (int64_t given : {bytes - 1, bytes, (int64_t)0, (int64_t)1 << 40}) {
            const bool room = size_ok && given >= bytes;
            tally(prompt_points_check(P, elem, h, w, P, n, 0.01, P, given, P, P, P), (elem == 1 || elem == 8) && n_ok && room,
                  "check", h, w, n, elem);
          }
      }
    }
  // the null pointers, the alignments and the threshold, one at a time on an otherwise good call
  const int64_t need = deva_prompt_scratch(96, 128, 64);
  const auto at = [](int off) { return reinterpret_cast<const void*>((uintptr_t(1) << 40) + off); };
  struct { const void *m; int e; const void *p, *s, *o, *l, *c; double t; bool ok; } single[] = {
      {P, 8, P, P, P, P, P, 0.01, true},        {P, 1, P, P, P, P, P, 0.01, true},
      {nullptr, 8, P, P, P, P, P, 0.01, false}, {at(4), 8, P, P, P, P, P, 0.01, false},
      {at(8), 8, P, P, P, P, P, 0.01, true},    {at(3), 1, P, P, P, P, P, 0.01, true},
      {P, 8, nullptr, P, P, P, P, 0.01, false}, {P, 8, at(2), P, P, P, P, 0.01, false},
      {P, 8, at(4), P, P, P, P, 0.01, true},    {P, 8, P, nullptr, P, P, P, 0.01, false},
      {P, 8, P, at(8), P, P, P, 0.01, false},   {P, 8, P, at(16), P, P, P, 0.01, true},
      {P, 8, P, P, nullptr, P, P, 0.01, false}, {P, 8, P, P, at(1), P, P, 0.01, false},
      {P, 8, P, P, P, nullptr, P, 0.01, false}, {P, 8, P, P, P, at(2), P, 0.01, false},
      {P, 8, P, P, P, P, nullptr, 0.01, false}, {P, 8, P, P, P, P, at(3), 0.01, false},
      {P, 8, P, P, at(4), at(4), at(4), 0.01, true}, {P, 8, P, P, P, P, P, nan, false},
      {P, 8, P, P, P, P, P, -1.0, true},        {P, 8, P, P, P, P, P, 1.0 / 0.0, true},
      {P, 8, P, P, P, P, P, -1.0 / 0.0, true}};
  for (const auto& c : single)
    tally(prompt_points_check(c.m, c.e, 96, 128, c.p, 64, c.t, c.s, need, c.o, c.l, c.c), c.ok, "single", 96, 128, 64, c.e);
  printf("%ld checks (%ld refused), %ld failures\n", g_calls, g_refused, g_failed);
  return g_failed ? 1 : 0;
}
