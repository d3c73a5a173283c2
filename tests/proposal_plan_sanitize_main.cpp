// Stand-alone host program for tests/test_plan_sanitize_cpu.py: the HIP-free side of the proposal filter
// (csrc/proposal_plan.cpp: the argument checks of its five launching entry points, the scratch layout and
// deva_proposal_scratch) walked over the product of its boundary values under the host sanitizers.  Addresses are
// made up: nothing is dereferenced.
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <initializer_list>

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

static void fail(const char* what, int cap, int b, int h, int w) {
  ++g_failed;
  fprintf(stderr, "FAIL %s: capacity=%d batch=%d %dx%d (%s)\n", what, cap, b, h, w, deva::g_err);
}

static void tally(int e, bool want, const char* name, const char* what, int cap, int b, int h, int w) {
  ++g_calls;
  if (e != 0) ++g_refused;
  if ((e == 0) != want) fail(what, cap, b, h, w);
  if (e != 0 && (e != 2 || !strstr(deva::g_err, name))) fail("refusal text", cap, b, h, w);
  deva::g_err[0] = 0;
}

int main() {
  using namespace deva;
  const int caps[] = {-1, 0, 1, 2, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 4095, 4096, 4097, 1 << 30, 2147483647};
  const int batches[] = {-1, 0, 1, 3, 192, 1023, 1024, 1025, 5000, 2147483647};
  const int sides[] = {-1, 0, 1, 3, 29, 53, 1080, 1920, 32768, 32769, 46341, 65536, 2147483647};
  const void* P = reinterpret_cast<const void*>(uintptr_t(1) << 40);
  const double nan = 0.0 / 0.0;
  for (int cap : caps) {
    const int64_t bytes = deva_proposal_scratch(cap);
    const bool cap_ok = cap >= 1 && cap <= kPropMaxMasks;
    if ((bytes >= 0) != cap_ok || proposal_capacity_ok(cap) != cap_ok) fail("scratch / capacity_ok disagree", cap, 0, 0, 0);
    if (cap_ok) {
      const ProposalPlan p = proposal_plan(cap);
      const int64_t offs[] = {p.off_stats, p.off_slots, p.off_count, p.off_table, p.off_order,
                              p.off_keep,  p.off_nkeep, p.off_matrix, p.bytes};
      bool ok = p.bytes == bytes && offs[0] == 0 && p.words >= 1 && p.words <= 64 && (int64_t)p.words * 64 >= cap &&
                (int64_t)(p.words - 1) * 64 < cap;
      for (int i = 0; i < 8; ++i) ok = ok && offs[i] % 256 == 0 && offs[i] < offs[i + 1];
      ok = ok && p.off_slots - p.off_stats >= (int64_t)kPropBatch * kPropStat * 4 && p.off_count - p.off_slots >= kPropBatch * 4 &&
           p.off_table - p.off_count >= 16 && p.off_order - p.off_table >= (int64_t)cap * kPropRow * 4 &&
           p.off_keep - p.off_order >= (int64_t)cap * 4 && p.off_nkeep - p.off_keep >= (int64_t)cap * 4 &&
           p.off_matrix - p.off_nkeep >= 16 && p.bytes - p.off_matrix >= (int64_t)cap * p.words * 8;
      if (!ok) fail("layout", cap, 0, 0, 0);
    }
    for (int64_t given : {bytes - 1, bytes, (int64_t)0}) {
      const bool room = cap_ok && given >= bytes;
      tally(proposal_begin_check(cap, P, given), room, "deva_proposal_begin", "begin", cap, 0, 0, 0);
      tally(proposal_finish_check(cap, 0.7, P, given, P), room, "deva_proposal_finish", "finish", cap, 0, 0, 0);
      for (int h : sides)
        for (int w : sides) {
          const bool plane = h > 0 && w > 0 && (int64_t)h * w <= kPropMaxPixels;
          if (plane) {
            const int chunks = proposal_chunks(h, w);
            if (chunks < 1 || (int64_t)chunks * kPropChunk < (int64_t)h * w + 15 ||
                (int64_t)(chunks - 1) * kPropChunk >= (int64_t)h * w + 15)
              fail("chunks", cap, 0, h, w);
          }
          for (int b : batches)
            tally(proposal_batch_check(P, P, b, h, w, 0.88, 0.95, 1.0, 0.0, P, cap, P, given), b >= 0 && plane && room,
                  "deva_proposal_batch", "batch", cap, b, h, w);
          for (int kept : {-1, 0, 1, cap, cap < 2147483647 ? cap + 1 : cap})
            tally(proposal_gather_check(P, cap, h, w, P, given, kept, P), plane && room && kept >= 0 && kept <= cap,
                  "deva_proposal_gather", "gather", cap, kept, h, w);
        }
      // deva_box_nms takes the number of boxes where the others take the capacity, and 0 boxes need no scratch
      tally(box_nms_check(P, P, cap, 0.7, P, given, P, P), cap == 0 || room, "deva_box_nms", "box_nms", cap, 0, 0, 0);
    }
  }
  // the null pointers, the alignments and the thresholds, one at a time on an otherwise good call
  const int64_t need = deva_proposal_scratch(16);
  const void* odd = reinterpret_cast<const void*>((uintptr_t(1) << 40) + 2);
  const void* off8 = reinterpret_cast<const void*>((uintptr_t(1) << 40) + 8);
  struct { const void *l, *i, *a, *s; int b; double p, t, o, m; bool ok; } single[] = {
      {P, P, P, P, 3, 0.88, 0.95, 1.0, 0.0, true},       {nullptr, P, P, P, 3, 0.88, 0.95, 1.0, 0.0, false},
      {nullptr, nullptr, P, P, 0, 0.88, 0.95, 1.0, 0.0, true}, {P, nullptr, P, P, 3, 0.88, 0.95, 1.0, 0.0, false},
      {P, P, nullptr, P, 3, 0.88, 0.95, 1.0, 0.0, false}, {P, P, P, nullptr, 3, 0.88, 0.95, 1.0, 0.0, false},
      {odd, P, P, P, 3, 0.88, 0.95, 1.0, 0.0, false},     {P, P, odd, P, 3, 0.88, 0.95, 1.0, 0.0, true},
      {P, P, P, off8, 3, 0.88, 0.95, 1.0, 0.0, false},    {P, P, P, P, 3, nan, 0.95, 1.0, 0.0, false},
      {P, P, P, P, 3, 0.88, nan, 1.0, 0.0, false},        {P, P, P, P, 3, 0.88, 0.95, nan, 0.0, false},
      {P, P, P, P, 3, 0.88, 0.95, 1.0, nan, false},       {P, P, P, P, 3, -1.0, 0.0, 1.0 / 0.0, -1.0 / 0.0, true}};
  for (const auto& c : single)
    tally(proposal_batch_check(c.l, c.i, c.b, 8, 8, c.p, c.t, c.o, c.m, c.a, 16, c.s, need), c.ok, "deva_proposal_batch",
          "single batch", 16, c.b, 8, 8);
  tally(proposal_finish_check(16, nan, P, need, P), false, "deva_proposal_finish", "finish nan", 16, 0, 0, 0);
  tally(proposal_finish_check(16, 0.7, P, need, nullptr), false, "deva_proposal_finish", "finish null", 16, 0, 0, 0);
  tally(proposal_finish_check(16, 0.7, P, need, odd), false, "deva_proposal_finish", "finish odd", 16, 0, 0, 0);
  tally(proposal_gather_check(nullptr, 16, 8, 8, P, need, 0, nullptr), true, "deva_proposal_gather", "gather none", 16, 0, 8, 8);
  tally(proposal_gather_check(nullptr, 16, 8, 8, P, need, 2, P), false, "deva_proposal_gather", "gather arena", 16, 2, 8, 8);
  tally(proposal_gather_check(P, 16, 8, 8, P, need, 2, nullptr), false, "deva_proposal_gather", "gather out", 16, 2, 8, 8);
  tally(box_nms_check(nullptr, nullptr, 0, 0.7, nullptr, 0, nullptr, P), true, "deva_box_nms", "nms none", 0, 0, 0, 0);
  tally(box_nms_check(nullptr, nullptr, 0, 0.7, nullptr, 0, nullptr, nullptr), false, "deva_box_nms", "nms count", 0, 0, 0, 0);
  tally(box_nms_check(nullptr, P, 16, 0.7, P, need, P, P), false, "deva_box_nms", "nms boxes", 16, 0, 0, 0);
  tally(box_nms_check(P, nullptr, 16, 0.7, P, need, P, P), false, "deva_box_nms", "nms scores", 16, 0, 0, 0);
  tally(box_nms_check(P, P, 16, 0.7, P, need, nullptr, P), false, "deva_box_nms", "nms keep", 16, 0, 0, 0);
  tally(box_nms_check(P, P, 16, nan, P, need, P, P), false, "deva_box_nms", "nms nan", 16, 0, 0, 0);
  tally(box_nms_check(P, P, 16, 0.7, P, need, P, P), true, "deva_box_nms", "nms good", 16, 0, 0, 0);
  printf("%ld checks (%ld refused), %ld failures\n", g_calls, g_refused, g_failed);
  return g_failed ? 1 : 0;
}
