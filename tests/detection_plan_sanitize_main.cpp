// Stand-alone host program for tests/test_plan_sanitize_cpu.py: the HIP-free side of deva_detection_assemble
// (csrc/detection_plan.cpp: the argument checks and the scratch layout, and deva_detection_scratch) walked over the
// product of its boundary values under the host sanitizers.  Addresses are made up: nothing is dereferenced.
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <initializer_list>

#include "deva_hip.h"
#include "detection_plan.h"

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

static void fail(const char* what, int n, int h, int w, int oh, int ow) {
  ++g_failed;
  fprintf(stderr, "FAIL %s: n=%d %dx%d -> %dx%d (%s)\n", what, n, h, w, oh, ow, deva::g_err);
}

int main() {
  const int counts[] = {-1, 0, 1, 2, 255, 256, 257, 1024, 1025, 4095, 4096, 4097, 1 << 30};
  const int sides[] = {-1, 0, 1, 3, 16, 127, 128, 1080, 1920, 46340, 46341, 65536, 2147483647};
  const int policies[] = {-1, 0, 1, 2, 3};
  const void* P = reinterpret_cast<const void*>(uintptr_t(1) << 40);
  for (int n : counts)
    for (int h : sides)
      for (int w : sides)
        for (int oh : sides)
          for (int ow : {oh, 853, 0}) {
            const int64_t bytes = deva_detection_scratch(n, h, w, oh, ow);
            const bool sizes_ok = deva::detection_sizes_ok(n, h, w, oh, ow);
            if ((bytes >= 0) != sizes_ok) fail("scratch / sizes_ok disagree", n, h, w, oh, ow);
            if (sizes_ok && n > 0) {
              const deva::DetectionPlan p = deva::detection_plan(n, h, w, oh, ow);
              const int64_t offs[] = {p.off_part_area, p.off_part_orig, p.off_part_src, p.off_area, p.off_orig,
                                      p.off_src,       p.off_mult,      p.off_stats,    p.off_lut,  p.off_plane, p.bytes};
              const int64_t most = (int64_t)h * w > (int64_t)oh * ow ? (int64_t)h * w : (int64_t)oh * ow;
              bool ok = p.bytes == bytes && offs[0] == 0 && p.chunks >= 1 && (int64_t)p.chunks * deva::kDetChunk >= most &&
                        (int64_t)(p.chunks - 1) * deva::kDetChunk < most;
              for (int i = 0; i < 10; ++i) ok = ok && offs[i] % 256 == 0 && offs[i] < offs[i + 1];
              ok = ok && p.off_part_orig - p.off_part_area >= (int64_t)n * p.chunks * 4 && p.off_orig - p.off_area >= (int64_t)n * 4 &&
                   p.off_lut - p.off_stats >= (int64_t)(n + 1) * 8 && p.off_plane - p.off_lut >= (int64_t)(n + 1) * 4 &&
                   p.bytes - p.off_plane >= (int64_t)oh * ow * 2;
              if (!ok) fail("layout", n, h, w, oh, ow);
            }
            for (int policy : policies)
              for (int64_t given : {bytes - 1, bytes, (int64_t)0}) {
                ++g_calls;
                deva::g_err[0] = 0;
                const int e = deva::detection_check(P, n, h, w, oh, ow, policy, 0.8, P, given, P, P);
                const bool want = n >= 0 && n <= deva::kDetMaxMasks && oh > 0 && ow > 0 && (int64_t)oh * ow < (1ll << 31) &&
                                  policy >= 0 && policy <= 2 &&
                                  (n == 0 || (h > 0 && w > 0 && (int64_t)h * w < (1ll << 31) && given >= bytes && bytes >= 0));
                if (e != 0) ++g_refused;
                if ((e == 0) != want) fail("check", n, h, w, oh, ow);
                if (e != 0 && (e != 2 || !strstr(deva::g_err, "deva_detection_assemble"))) fail("refusal text", n, h, w, oh, ow);
              }
          }
  // the null pointers and the threshold, one at a time on an otherwise good call
  const int64_t need = deva_detection_scratch(3, 8, 8, 8, 8);
  struct { const void *m, *s, *o, *r; double t; int policy; bool ok; } single[] = {
      {P, P, P, P, 0.8, 0, true},      {nullptr, P, P, P, 0.8, 0, false}, {P, nullptr, P, P, 0.8, 0, false},
      {P, P, nullptr, P, 0.8, 0, false}, {P, P, P, nullptr, 0.8, 0, false}, {P, P, P, P, 0.0 / 0.0, 0, false},
      {P, P, P, P, 0.0 / 0.0, 1, true},  {reinterpret_cast<const void*>(uintptr_t(8)), P, P, P, 0.8, 2, true},
      {P, reinterpret_cast<const void*>(uintptr_t(4104)), P, P, 0.8, 0, false}};
  for (const auto& c : single) {
    ++g_calls;
    const int e = deva::detection_check(c.m, 3, 8, 8, 8, 8, c.policy, c.t, c.s, need, c.o, c.r);
    if (e != 0) ++g_refused;
    if ((e == 0) != c.ok) fail("single", 3, 8, 8, 8, 8);
  }
  printf("%ld checks (%ld refused), %ld failures\n", g_calls, g_refused, g_failed);
  return g_failed ? 1 : 0;
}
