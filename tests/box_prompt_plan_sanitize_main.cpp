// Stand-alone host program for tests/test_plan_sanitize_cpu.py: the HIP-free side of the box prompts
// (csrc/box_prompt_plan.cpp: the argument checks of deva_box_nms_xyxy and deva_box_mask_select and the launch geometry of
// the latter) walked over the product of its boundary values under the host sanitizers.  Addresses are made up: nothing
// is dereferenced.
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <initializer_list>

#include "box_prompt_plan.h"
#include "deva_hip.h"
#include "proposal_plan.h"

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

static void fail(const char* what, long a, long b, long c, long d) {
  ++g_failed;
  fprintf(stderr, "FAIL %s: %ld %ld %ld %ld (%s)\n", what, a, b, c, d, deva::g_err);
}

static void tally(int e, bool want, const char* entry, const char* what, long a, long b, long c, long d) {
  ++g_calls;
  if (e != 0) ++g_refused;
  if ((e == 0) != want) fail(what, a, b, c, d);
  if (e != 0 && (e != 2 || !strstr(deva::g_err, entry))) fail("refusal text", a, b, c, d);
  deva::g_err[0] = 0;
}

int main() {
  using namespace deva;
  const int sides[] = {-2147483647 - 1, -1, 0, 1, 2, 3, 4, 5, 53, 127, 128, 1080, 1920, 16383, 16384, 16385, 32768, 32769,
                       46341, 65536, 1 << 30, (1 << 30) + 1, 2147483647};
  const int batches[] = {-2147483647 - 1, -1, 0, 1, 3, 64, 65, 65535, 65536, 66000, 1 << 26, (1 << 26) + 1, 1 << 30, 2147483647};
  const int per_boxes[] = {-2147483647 - 1, -1, 0, 1, 2, 3, 4, 15, 16, 17, 64, 2147483647};
  const void* P = reinterpret_cast<const void*>(uintptr_t(1) << 40);
  const auto at = [](int off) { return reinterpret_cast<const void*>((uintptr_t(1) << 40) + off); };
  const double nan = 0.0 / 0.0;

  // deva_box_mask_select: sizes x batch x planes per box x the alignment of the output
  for (int h : sides)
    for (int w : sides) {
      const bool size_ok = h > 0 && w > 0 && (int64_t)h * w <= kBoxMaxPixels;
      if (size_ok) {
        const int64_t hw = (int64_t)h * w, chunks = box_select_chunks(h, w);
        // every element of the plane, shifted by up to 3, lies in a chunk; no chunk is empty at shift 0
        if (chunks < 1 || chunks * kBoxChunk < hw + 3 || (chunks - 1) * (int64_t)kBoxChunk >= hw + 3 ||
            chunks * (int64_t)kBoxChunk + kBoxChunk > 2147483647)
          fail("chunks", h, w, chunks, 0);
      }
      for (int b : batches)
        for (int m : per_boxes) {
          const bool m_ok = m >= 1 && m <= kBoxMaxPerBox;
          const bool planes_ok = b == 0 || (b > 0 && (int64_t)b * (m_ok ? m : 1) <= (int64_t)1 << 30);
          for (int off : {0, 1, 5, 13})
            tally(box_mask_select_check(P, P, b, m, h, w, 0.0, at(off), P), b >= 0 && m_ok && size_ok && planes_ok,
                  "deva_box_mask_select", "select", h, w, b, m);
        }
    }
  // the launches of a long batch stay inside it and inside one grid dimension
  for (int b : batches) {
    if (b < 0) continue;
    int64_t covered = 0;
    for (int64_t first = 0; first < b; first += kBoxMaxGridY) {
      const int64_t nb = b - first < kBoxMaxGridY ? b - first : kBoxMaxGridY;
      if (nb < 1 || nb > 65535) fail("launch", b, first, nb, 0);
      covered += nb;
    }
    if (covered != b) fail("launches", b, covered, 0, 0);
  }
  // the null pointers, the alignments and the threshold, one at a time on an otherwise good call
  struct { const void *l, *s; int b; double t; const void *o, *c; bool ok; } select[] = {
      {P, P, 2, 0.0, P, P, true},          {P, P, 2, 0.0, at(7), nullptr, true},  {nullptr, P, 2, 0.0, P, P, false},
      {at(2), P, 2, 0.0, P, P, false},     {at(4), P, 2, 0.0, P, P, true},        {P, nullptr, 2, 0.0, P, P, false},
      {P, at(1), 2, 0.0, P, P, false},     {P, at(4), 2, 0.0, P, P, true},        {P, P, 2, 0.0, nullptr, P, false},
      {P, P, 2, 0.0, P, at(2), false},     {P, P, 2, 0.0, P, at(4), true},        {P, P, 2, nan, P, P, false},
      {P, P, 2, 1.0 / 0.0, P, P, true},    {P, P, 2, -1.0 / 0.0, P, P, true},     {nullptr, nullptr, 0, 0.0, nullptr, nullptr, true},
      {nullptr, nullptr, 0, nan, nullptr, nullptr, false}};
  for (const auto& c : select)
    tally(box_mask_select_check(c.l, c.s, c.b, 3, 29, 53, c.t, c.o, c.c), c.ok, "deva_box_mask_select", "select single", c.b, 0, 0, 0);

  // deva_box_nms_xyxy: the number of boxes x the scratch given
  const int counts[] = {-2147483647 - 1, -1, 0, 1, 63, 64, 65, 130, 1000, 4095, 4096, 4097, 1 << 30, 2147483647};
  for (int n : counts) {
    const bool n_ok = n >= 0 && n <= kPropMaxMasks;
    const int64_t need = n_ok && n > 0 ? proposal_plan(n).bytes : 0;
    if (n_ok && n > 0 && need != deva_proposal_scratch(n)) fail("scratch", n, need, 0, 0);
    for (int64_t given : {need - 1, need, (int64_t)0, (int64_t)1 << 40})
      for (double t : {0.8, 0.0, -1.0, 1.0 / 0.0})
        tally(box_nms_xyxy_check(P, P, n, t, P, given, P, P), n_ok && (n == 0 || given >= need), "deva_box_nms_xyxy", "nms", n,
              given, 0, 0);
  }
  const int64_t need = deva_proposal_scratch(130);
  struct { const void *b, *s; double t; const void *sc, *k, *n; bool ok; } nms[] = {
      {P, P, 0.8, P, P, P, true},          {nullptr, P, 0.8, P, P, P, false},   {at(2), P, 0.8, P, P, P, false},
      {at(4), P, 0.8, P, P, P, true},      {P, nullptr, 0.8, P, P, P, false},   {P, at(3), 0.8, P, P, P, false},
      {P, P, nan, P, P, P, false},         {P, P, 0.8, nullptr, P, P, false},   {P, P, 0.8, at(8), P, P, false},
      {P, P, 0.8, at(16), P, P, true},     {P, P, 0.8, P, nullptr, P, false},   {P, P, 0.8, P, at(2), P, false},
      {P, P, 0.8, P, P, nullptr, false},   {P, P, 0.8, P, P, at(1), false},     {P, P, 0.8, P, at(4), at(4), true}};
  for (const auto& c : nms)
    tally(box_nms_xyxy_check(c.b, c.s, 130, c.t, c.sc, need, c.k, c.n), c.ok, "deva_box_nms_xyxy", "nms single", 130, 0, 0, 0);
  tally(box_nms_xyxy_check(nullptr, nullptr, 0, 0.8, nullptr, 0, nullptr, P), true, "deva_box_nms_xyxy", "nms empty", 0, 0, 0, 0);
  tally(box_nms_xyxy_check(nullptr, nullptr, 0, 0.8, nullptr, 0, nullptr, nullptr), false, "deva_box_nms_xyxy", "nms empty", 0, 0, 0, 0);
  printf("%ld checks (%ld refused), %ld failures\n", g_calls, g_refused, g_failed);
  return g_failed ? 1 : 0;
}
