// csrc/png/png_plan.cpp under the host sanitizers, in a program of its own (tests/test_png_cpu.py builds it with
// -fsanitize=address,undefined and runs it; nothing is loaded into Python and no GPU is involved).
//
// It sweeps the plan over heights, widths and bytes per pixel around the segment size, the step and the limits, holds
// every plan to its own arithmetic (Z5, Z7), carves the scratch of the accepted calls in a host buffer of exactly the size
// asked for, and sends every argument check of the two launchers through its refusals with made-up addresses.
// Prints "<checks> <refused> <failures>".
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "png_plan.h"

using namespace deva_png;

static long long g_checks = 0, g_refused = 0, g_failures = 0;

#define EXPECT(cond)                                                   \
  do {                                                                 \
    ++g_checks;                                                        \
    if (!(cond)) {                                                     \
      ++g_failures;                                                    \
      fprintf(stderr, "line %d: %s [%s]\n", __LINE__, #cond, last_error()); \
    }                                                                  \
  } while (0)

static bool refused(int rc, const char* word) {
  ++g_refused;
  return rc == 2 && strstr(last_error(), word) != nullptr;
}

static void sweep_plans() {
  const int sides[] = {-1, 0, 1, 2, 7, 8, 9, 15, 16, 17, 300, 341, 342, 480, 854, 1022, 1023, 1024, 1025, 1080, 1920, 2160, 3840, 16383, 16384,
                       16385, 1 << 20};
  const int bpps[] = {-1, 0, 1, 2, 3, 4};
  for (int h : sides)
    for (int w : sides)
      for (int bpp : bpps) {
        struct deva_png_plan p;
        memset(&p, 0x5a, sizeof(p));
        const int rc = png_plan("sweep", h, w, bpp, &p);
        if (bpp != 1 && bpp != 3) {
          EXPECT(refused(rc, "bpp: 1"));
          continue;
        }
        if (h < 1 || w < 1 || h > DEVA_PNG_MAX_SIDE || w > DEVA_PNG_MAX_SIDE) {
          EXPECT(refused(rc, "bad height x width"));
          continue;
        }
        const int64_t n = (int64_t)w * bpp;
        if (n * h > DEVA_PNG_MAX_BYTES) {
          EXPECT(refused(rc, "bytes, a call takes"));
          continue;
        }
        EXPECT(rc == 0);
        const int r = DEVA_PNG_ROWS_PER_SEGMENT;
        EXPECT(p.rows_per_segment == r && p.segments == (h + r - 1) / r && p.row_bytes == n && p.block == kBlock && p.reserved == 0);
        EXPECT((int64_t)p.steps_per_row * DEVA_PNG_STEP >= n + 1 && (int64_t)(p.steps_per_row - 1) * DEVA_PNG_STEP < n + 1);
        // Z7: a segment of r rows at 9 bits a byte, with its 13 bits of block framing, padded, and the stored block's 4 bytes
        const int64_t bits = 3 + 9 * (int64_t)r * (n + 1) + 7 + 3;
        EXPECT(segment_worst(r, n) == (bits + 7) / 8 + 4);
        EXPECT(p.slot_bytes % 16 == 0 && p.slot_bytes >= segment_worst(r, n) && p.slot_bytes < segment_worst(r, n) + 16);
        const int last = h - (p.segments - 1) * r;
        EXPECT(last >= 1 && last <= r);
        EXPECT(p.worst_case == 8 + (int64_t)(p.segments - 1) * segment_worst(r, n) + segment_worst(last, n));
        EXPECT(p.worst_case <= 2 + 6 + (int64_t)p.segments * p.slot_bytes);
        EXPECT(p.scratch_bytes % 256 == 0 && p.scratch_bytes >= 24ll * p.segments + p.slot_bytes * p.segments);
        if (p.scratch_bytes <= (4ll << 20)) {   // the carved pieces lie inside the bytes asked for and do not meet
          std::vector<uint8_t> host(p.scratch_bytes, 0);
          const Scratch sc = carve(host.data(), p);
          const int s = p.segments;
          sc.sizes[0] = 1, sc.sizes[s - 1] = 2;
          sc.sums[0] = 3, sc.sums[2 * s - 1] = 4;
          sc.offsets[0] = 5, sc.offsets[s - 1] = 6;
          sc.slots[0] = 7, sc.slots[(int64_t)s * p.slot_bytes - 1] = 8;
          EXPECT(reinterpret_cast<uint8_t*>(sc.sizes) == host.data() && reinterpret_cast<uint8_t*>(sc.sizes + s) <= reinterpret_cast<uint8_t*>(sc.sums));
          EXPECT(reinterpret_cast<uint8_t*>(sc.sums + 2 * s) <= reinterpret_cast<uint8_t*>(sc.offsets));
          EXPECT(reinterpret_cast<uint8_t*>(sc.offsets + s) <= sc.slots && sc.slots + (int64_t)s * p.slot_bytes <= host.data() + host.size());
          EXPECT(reinterpret_cast<uintptr_t>(sc.slots) % 16 == reinterpret_cast<uintptr_t>(host.data()) % 16);
          EXPECT(sc.sizes[0] == (s == 1 ? 2 : 1) && sc.sums[0] == 3 && sc.offsets[s - 1] == 6 && sc.slots[0] == 7);
        }
      }
}

static void sweep_refusals() {
  // made-up device addresses: every check fails or passes before anything is dereferenced
  uint8_t* const A = reinterpret_cast<uint8_t*>(1ll << 40);
  const int h = 65, w = 129;
  struct deva_png_plan p;
  EXPECT(png_plan("sizes", h, w, 3, &p) == 0);
  const uint8_t* plane = A + 5;                                   // (planes begin at any byte address)
  void* scratch = A + (16 << 20);
  uint8_t* out = A + (32 << 20) + 3;
  int64_t* info = reinterpret_cast<int64_t*>(A + (48 << 20));
  const int64_t sb = p.scratch_bytes, cap = 4096;
  auto deflate = [&](const uint8_t* pl, int h_, int w_, int b_, const void* sc, int64_t sb_, const uint8_t* o, int64_t c, const int64_t* i) {
    return deflate_check(pl, h_, w_, b_, sc, sb_, o, c, i, nullptr);
  };
  EXPECT(deflate(plane, h, w, 3, scratch, sb, out, cap, info) == 0);
  EXPECT(deflate(plane, h, w, 3, scratch, sb + 100, out, cap, info) == 0);
  EXPECT(deflate(plane, h, w, 3, scratch, sb, nullptr, 0, info) == 0);                                   // the total alone
  EXPECT(refused(deflate(nullptr, h, w, 3, scratch, sb, out, cap, info), "plane: null"));
  EXPECT(refused(deflate(plane, 0, w, 3, scratch, sb, out, cap, info), "bad height x width"));
  EXPECT(refused(deflate(plane, h, DEVA_PNG_MAX_SIDE + 1, 3, scratch, sb, out, cap, info), "bad height x width"));
  EXPECT(refused(deflate(plane, DEVA_PNG_MAX_SIDE, DEVA_PNG_MAX_SIDE, 3, scratch, sb, out, cap, info), "bytes, a call takes"));
  EXPECT(refused(deflate(plane, h, w, 2, scratch, sb, out, cap, info), "bpp: 1"));
  EXPECT(refused(deflate(plane, h, w, 3, nullptr, sb, out, cap, info), "scratch: null"));
  EXPECT(refused(deflate(plane, h, w, 3, A + (16 << 20) + 8, sb, out, cap, info), "not 16-byte aligned"));
  EXPECT(refused(deflate(plane, h, w, 3, scratch, sb - 1, out, cap, info), "scratch_bytes"));
  EXPECT(refused(deflate(plane, h, w, 3, scratch, sb, nullptr, cap, info), "out: null"));
  EXPECT(refused(deflate(plane, h, w, 3, scratch, sb, out, -1, info), "capacity"));
  EXPECT(refused(deflate(plane, h, w, 3, scratch, sb, out, (1ll << 40) + 1, info), "capacity"));
  EXPECT(refused(deflate(plane, h, w, 3, scratch, sb, out, cap, nullptr), "info"));
  EXPECT(refused(deflate(plane, h, w, 3, scratch, sb, out, cap, reinterpret_cast<int64_t*>(A + (48 << 20) + 4)), "info"));
  EXPECT(refused(deflate(plane, h, w, 3, scratch, sb, static_cast<uint8_t*>(scratch) + sb - 1, cap, info), "out overlaps scratch"));
  EXPECT(refused(deflate(plane, h, w, 3, scratch, sb, out, cap, reinterpret_cast<int64_t*>(static_cast<uint8_t*>(scratch) + 256)), "info overlaps scratch"));
  EXPECT(refused(deflate(plane, h, w, 3, scratch, sb, reinterpret_cast<uint8_t*>(info) - 4000, cap, info), "info overlaps out"));
  EXPECT(refused(deflate(static_cast<uint8_t*>(scratch) - 10, h, w, 3, scratch, sb, out, cap, info), "plane overlaps scratch"));
  EXPECT(refused(deflate(out + cap - 1, h, w, 3, scratch, sb, out, cap, info), "plane overlaps out"));
  EXPECT(refused(deflate(reinterpret_cast<uint8_t*>(info) - 3 * h * w + 1, h, w, 3, scratch, sb, out, cap, info), "plane overlaps info"));
  auto place = [&](int h_, int w_, int b_, const void* sc, int64_t sb_, const uint8_t* o, int64_t c, const int64_t* i) {
    return place_check("deva_png_place", h_, w_, b_, sc, sb_, o, c, i, nullptr);
  };
  EXPECT(place(h, w, 3, scratch, sb, out, cap, info) == 0);
  EXPECT(refused(place(h, w, 0, scratch, sb, out, cap, info), "bpp: 1"));
  EXPECT(refused(place(h, -4, 3, scratch, sb, out, cap, info), "bad height x width"));
  EXPECT(refused(place(h, w, 3, scratch, 0, out, cap, info), "scratch_bytes"));
  EXPECT(refused(place(h, w, 3, scratch, sb, nullptr, 1, info), "out: null"));
  EXPECT(refused(place(h, w, 3, scratch, sb, out, cap, nullptr), "info"));
  struct deva_png_limits lim;
  EXPECT(deva_png_limits(&lim) == 0 && lim.max_side == DEVA_PNG_MAX_SIDE && lim.max_bytes == DEVA_PNG_MAX_BYTES && lim.block == kBlock &&
         lim.rows_per_segment == DEVA_PNG_ROWS_PER_SEGMENT && lim.step == DEVA_PNG_STEP && lim.lds_bytes == kLdsBytes);
  EXPECT(refused(deva_png_limits(nullptr), "null limits"));
  EXPECT(refused(deva_png_plan(4, 4, 1, nullptr), "null plan"));
  EXPECT(deva_png_version() == DEVA_PNG_ABI_VERSION);
}

int main() {
  sweep_plans();
  sweep_refusals();
  printf("%lld %lld %lld\n", g_checks, g_refused, g_failures);
  return g_failures ? 1 : 0;
}
