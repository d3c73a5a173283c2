// csrc/jpeg/jpeg_plan.cpp under the host sanitizers, in a program of its own (tests/test_jpeg_cpu.py builds it with
// -fsanitize=address,undefined and runs it; nothing is loaded into Python and no GPU is involved).
//
// It sweeps the plan over heights, widths, subsamplings and restart intervals around the MCU, the step and the limits,
// holds every plan to its own arithmetic (J2, J7, J8, J10), carves the scratch of the accepted calls in a host buffer of
// exactly the size asked for, holds the compile-time tables to their rules (J4: the DCT matrix from the cosine; J5: the
// division's range; J6: the codes are prefix-free and complete up to the reserved all-ones code), and sends every
// argument check of the two launchers through its refusals with made-up addresses.
// Prints "<checks> <refused> <failures>".
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "jpeg_plan.h"

using namespace deva_jpeg;

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
  const int sides[] = {-1, 0, 1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 47, 480, 854, 1080, 1920, 2040, 2048, 2056, 2160, 3840, 16383, 16384, 16385, 1 << 20};
  const int subs[] = {0, 420, 422, 444};
  const int restarts[] = {-1, 0, 1, 3, 120, 65535, 65536};
  for (int h : sides)
    for (int w : sides)
      for (int sub : subs)
        for (int restart : restarts) {
          struct deva_jpeg_plan p;
          memset(&p, 0x5a, sizeof(p));
          const int rc = jpeg_plan("sweep", h, w, sub, restart, &p);
          if (sub != 420 && sub != 444) {
            EXPECT(refused(rc, "subsampling: 420"));
            continue;
          }
          if (h < 1 || w < 1 || h > DEVA_JPEG_MAX_SIDE || w > DEVA_JPEG_MAX_SIDE) {
            EXPECT(refused(rc, "bad height x width"));
            continue;
          }
          if ((int64_t)h * w * 3 > DEVA_JPEG_MAX_BYTES) {
            EXPECT(refused(rc, "bytes, a call takes"));
            continue;
          }
          if (restart < 0 || restart > DEVA_JPEG_MAX_RESTART) {
            EXPECT(refused(rc, "restart: 0"));
            continue;
          }
          EXPECT(rc == 0);
          const int mcu = sub == 420 ? 16 : 8, per = sub == 420 ? 6 : 3;
          EXPECT(p.mcu == mcu && p.blocks_per_mcu == per && p.block == kBlock);
          EXPECT(p.mcus_x * mcu >= w && (p.mcus_x - 1) * mcu < w && p.mcus_y * mcu >= h && (p.mcus_y - 1) * mcu < h);
          const int64_t mcus = (int64_t)p.mcus_x * p.mcus_y;
          EXPECT(p.restart == (restart ? restart : p.mcus_x) && p.restart >= 1 && p.restart <= DEVA_JPEG_MAX_RESTART);
          EXPECT((int64_t)p.intervals * p.restart >= mcus && (int64_t)(p.intervals - 1) * p.restart < mcus && p.intervals >= 1);
          EXPECT(p.blocks == mcus * per && p.coef_bytes == 128ll * p.blocks);
          // J8 / J10: an interval at kBlockBits a block, padded, every byte stuffed, the marker
          const int64_t full = mcus < p.restart ? mcus : p.restart, last = mcus - (int64_t)(p.intervals - 1) * p.restart;
          EXPECT(interval_worst(full * per) == 2 * ((full * per * kBlockBits + 7) / 8) + 2);
          EXPECT(p.slot_bytes % 16 == 0 && p.slot_bytes >= interval_worst(full * per) + 16 && p.slot_bytes < interval_worst(full * per) + 32);
          EXPECT(last >= 1 && last <= p.restart);
          EXPECT(p.worst_case == (p.intervals - 1) * interval_worst((int64_t)p.restart * per) + interval_worst(last * per) - 2);
          EXPECT(p.worst_case <= (int64_t)p.intervals * p.slot_bytes);
          EXPECT(p.scratch_bytes % 256 == 0 && p.scratch_bytes >= 16ll * p.intervals + p.coef_bytes + p.slot_bytes * p.intervals);
          if (p.scratch_bytes <= (4ll << 20)) {   // the carved pieces lie inside the bytes asked for and do not meet
            std::vector<uint8_t> host(p.scratch_bytes, 0);
            const Scratch sc = carve(host.data(), p);
            const int s = p.intervals;
            sc.sizes[0] = 1, sc.sizes[s - 1] = 2;
            sc.offsets[0] = 5, sc.offsets[s - 1] = 6;
            sc.coefs[0] = 3, sc.coefs[64ll * p.blocks - 1] = 4;
            sc.slots[0] = 7, sc.slots[(int64_t)s * p.slot_bytes - 1] = 8;
            EXPECT(reinterpret_cast<uint8_t*>(sc.sizes) == host.data() && reinterpret_cast<uint8_t*>(sc.sizes + s) <= reinterpret_cast<uint8_t*>(sc.offsets));
            EXPECT(reinterpret_cast<uint8_t*>(sc.offsets + s) <= reinterpret_cast<uint8_t*>(sc.coefs));
            EXPECT(reinterpret_cast<uint8_t*>(sc.coefs + 64ll * p.blocks) <= sc.slots && sc.slots + (int64_t)s * p.slot_bytes <= host.data() + host.size());
            EXPECT(reinterpret_cast<uintptr_t>(sc.slots) % 16 == reinterpret_cast<uintptr_t>(host.data()) % 16);
            EXPECT(reinterpret_cast<uintptr_t>(sc.coefs) % 16 == reinterpret_cast<uintptr_t>(host.data()) % 16);
            EXPECT(sc.sizes[0] == (s == 1 ? 2 : 1) && sc.offsets[s - 1] == 6 && sc.coefs[0] == 3 && sc.slots[0] == 7);
          }
        }
}

static void sweep_tables() {
  // J4: the matrix from the cosine
  const double pi = 3.14159265358979323846;
  for (int k = 0; k < 8; ++k)
    for (int n = 0; n < 8; ++n) EXPECT(kDct[k][n] == (int)lrint(8192 * (k ? 0.5 : sqrt(0.125)) * cos((2 * n + 1) * k * pi / 16)));
  // the zigzag is a permutation that walks the anti-diagonals
  int seen[64] = {0};
  for (int z = 0; z < 64; ++z) {
    EXPECT(kZigzag[z] < 64 && !seen[kZigzag[z]]++);
    if (z) EXPECT(kZigzag[z] / 8 + kZigzag[z] % 8 >= kZigzag[z - 1] / 8 + kZigzag[z - 1] % 8);
  }
  // J5: libjpeg's scaling at its corners; every table entry 1 .. 255
  EXPECT(quant(16, 50) == 16 && quant(16, 75) == 8 && quant(16, 100) == 1 && quant(99, 1) == 255 && quant(10, 95) == 1 && quant(121, 25) == 242);
  for (int q = 1; q <= 100; ++q) {
    const QuantTables t = quant_tables(q);
    uint8_t dqt[128];
    EXPECT(deva_jpeg_quant(q, dqt) == 0);
    for (int z = 0; z < 64; ++z) EXPECT(t.q[0][z] >= 1 && t.q[1][z] >= 1 && dqt[z] == t.q[0][kZigzag[z]] && dqt[64 + z] == t.q[1][kZigzag[z]]);
  }
  // J6: each table's codes are distinct, prefix-free, and fill the code space but for the all-ones code (Kraft sum 1 - 2^-16 * k)
  const HuffmanTables tables = huffman_tables();
  const int first[4] = {0, 256, 512, 528}, count[4] = {256, 256, 16, 16}, symbols[4] = {162, 162, 12, 12};
  for (int t = 0; t < 4; ++t) {
    int coded = 0;
    long long kraft = 0;
    for (int a = 0; a < count[t]; ++a) {
      const uint32_t ea = tables.entry[first[t] + a], la = ea >> 16;
      if (!la) continue;
      ++coded;
      kraft += 1ll << (16 - la);
      EXPECT(la <= 16 && (ea & 0xffff) < (1u << la) && (ea & 0xffff) != (1u << la) - 1);
      for (int b = 0; b < count[t]; ++b) {
        const uint32_t eb = tables.entry[first[t] + b], lb = eb >> 16;
        if (b != a && lb >= la && lb) EXPECT(((eb & 0xffff) >> (lb - la)) != (ea & 0xffff));
      }
    }
    EXPECT(coded == symbols[t] && kraft < (1ll << 16));
  }
  EXPECT((tables.entry[0xF0] >> 16) == 11 && (tables.entry[256 + 0xF0] >> 16) == 10);
  // every AC symbol the coder can form has a code: runs 0 .. 15 with sizes 1 .. 10, EOB, ZRL; every DC size 0 .. 11
  for (int chroma = 0; chroma < 2; ++chroma) {
    for (int run = 0; run < 16; ++run)
      for (int size = 1; size <= 10; ++size) EXPECT(tables.entry[256 * chroma + (run << 4 | size)] >> 16);
    for (int size = 0; size <= 11; ++size) EXPECT(tables.entry[512 + 16 * chroma + size] >> 16);
    EXPECT(tables.entry[256 * chroma] >> 16);
  }
  // the longest block is what kBlockBits says
  int longest_dc = 0, longest_ac = 0;
  for (int size = 0; size <= 11; ++size) longest_dc = std::max<int>(longest_dc, (int)(tables.entry[512 + size] >> 16) + size);
  for (int chroma = 0; chroma < 2; ++chroma)
    for (int s = 0; s < 256; ++s)
      if ((s & 15) <= 10) longest_ac = std::max<int>(longest_ac, (int)(tables.entry[256 * chroma + s] >> 16) + (s & 15));
  EXPECT(longest_dc <= 20 && longest_ac <= 26 && kBlockBits == 20 + 63 * 26);
}

static void sweep_refusals() {
  // made-up device addresses: every check fails or passes before anything is dereferenced
  uint8_t* const A = reinterpret_cast<uint8_t*>(1ll << 40);
  const int h = 65, w = 129;
  struct deva_jpeg_plan p;
  EXPECT(jpeg_plan("sizes", h, w, 420, 0, &p) == 0);
  const uint8_t* plane = A + 5;                                   // (planes begin at any byte address)
  void* scratch = A + (16 << 20);
  uint8_t* out = A + (32 << 20) + 3;
  int64_t* info = reinterpret_cast<int64_t*>(A + (48 << 20));
  const int64_t sb = p.scratch_bytes, cap = 4096;
  auto scan = [&](const uint8_t* pl, int h_, int w_, int q_, int s_, int r_, const void* sc, int64_t sb_, const uint8_t* o, int64_t c, const int64_t* i) {
    return scan_check(pl, h_, w_, q_, s_, r_, sc, sb_, o, c, i, nullptr);
  };
  EXPECT(scan(plane, h, w, 75, 420, 0, scratch, sb, out, cap, info) == 0);
  EXPECT(scan(plane, h, w, 1, 420, 0, scratch, sb + 100, out, cap, info) == 0);
  EXPECT(scan(plane, h, w, 100, 420, 0, scratch, sb, nullptr, 0, info) == 0);                                   // the total alone
  EXPECT(refused(scan(nullptr, h, w, 75, 420, 0, scratch, sb, out, cap, info), "plane: null"));
  EXPECT(refused(scan(plane, 0, w, 75, 420, 0, scratch, sb, out, cap, info), "bad height x width"));
  EXPECT(refused(scan(plane, h, DEVA_JPEG_MAX_SIDE + 1, 75, 420, 0, scratch, sb, out, cap, info), "bad height x width"));
  EXPECT(refused(scan(plane, DEVA_JPEG_MAX_SIDE, DEVA_JPEG_MAX_SIDE, 75, 420, 0, scratch, sb, out, cap, info), "bytes, a call takes"));
  EXPECT(refused(scan(plane, h, w, 0, 420, 0, scratch, sb, out, cap, info), "quality: 1 to 100"));
  EXPECT(refused(scan(plane, h, w, 101, 420, 0, scratch, sb, out, cap, info), "quality: 1 to 100"));
  EXPECT(refused(scan(plane, h, w, 75, 422, 0, scratch, sb, out, cap, info), "subsampling: 420"));
  EXPECT(refused(scan(plane, h, w, 75, 420, -1, scratch, sb, out, cap, info), "restart: 0"));
  EXPECT(refused(scan(plane, h, w, 75, 420, 65536, scratch, sb, out, cap, info), "restart: 0"));
  EXPECT(refused(scan(plane, h, w, 75, 420, 0, nullptr, sb, out, cap, info), "scratch: null"));
  EXPECT(refused(scan(plane, h, w, 75, 420, 0, A + (16 << 20) + 8, sb, out, cap, info), "not 16-byte aligned"));
  EXPECT(refused(scan(plane, h, w, 75, 420, 0, scratch, sb - 1, out, cap, info), "scratch_bytes"));
  EXPECT(refused(scan(plane, h, w, 75, 444, 1, scratch, sb, out, cap, info), "scratch_bytes"));                 // (another plan needs more)
  EXPECT(refused(scan(plane, h, w, 75, 420, 0, scratch, sb, nullptr, cap, info), "out: null"));
  EXPECT(refused(scan(plane, h, w, 75, 420, 0, scratch, sb, out, -1, info), "capacity"));
  EXPECT(refused(scan(plane, h, w, 75, 420, 0, scratch, sb, out, (1ll << 40) + 1, info), "capacity"));
  EXPECT(refused(scan(plane, h, w, 75, 420, 0, scratch, sb, out, cap, nullptr), "info"));
  EXPECT(refused(scan(plane, h, w, 75, 420, 0, scratch, sb, out, cap, reinterpret_cast<int64_t*>(A + (48 << 20) + 4)), "info"));
  EXPECT(refused(scan(plane, h, w, 75, 420, 0, scratch, sb, static_cast<uint8_t*>(scratch) + sb - 1, cap, info), "out overlaps scratch"));
  EXPECT(refused(scan(plane, h, w, 75, 420, 0, scratch, sb, out, cap, reinterpret_cast<int64_t*>(static_cast<uint8_t*>(scratch) + 256)), "info overlaps scratch"));
  EXPECT(refused(scan(plane, h, w, 75, 420, 0, scratch, sb, reinterpret_cast<uint8_t*>(info) - 4000, cap, info), "info overlaps out"));
  EXPECT(refused(scan(static_cast<uint8_t*>(scratch) - 10, h, w, 75, 420, 0, scratch, sb, out, cap, info), "plane overlaps scratch"));
  EXPECT(refused(scan(out + cap - 1, h, w, 75, 420, 0, scratch, sb, out, cap, info), "plane overlaps out"));
  EXPECT(refused(scan(reinterpret_cast<uint8_t*>(info) - 3 * h * w + 1, h, w, 75, 420, 0, scratch, sb, out, cap, info), "plane overlaps info"));
  auto place = [&](int h_, int w_, int s_, int r_, const void* sc, int64_t sb_, const uint8_t* o, int64_t c, const int64_t* i) {
    return place_check("deva_jpeg_place", h_, w_, s_, r_, sc, sb_, o, c, i, nullptr);
  };
  EXPECT(place(h, w, 420, 0, scratch, sb, out, cap, info) == 0);
  EXPECT(refused(place(h, w, 0, 0, scratch, sb, out, cap, info), "subsampling: 420"));
  EXPECT(refused(place(h, -4, 420, 0, scratch, sb, out, cap, info), "bad height x width"));
  EXPECT(refused(place(h, w, 420, 0, scratch, 0, out, cap, info), "scratch_bytes"));
  EXPECT(refused(place(h, w, 420, 0, scratch, sb, nullptr, 1, info), "out: null"));
  EXPECT(refused(place(h, w, 420, 0, scratch, sb, out, cap, nullptr), "info"));
  struct deva_jpeg_limits lim;
  EXPECT(deva_jpeg_limits(&lim) == 0 && lim.max_side == DEVA_JPEG_MAX_SIDE && lim.max_bytes == DEVA_JPEG_MAX_BYTES && lim.block == kBlock &&
         lim.max_restart == DEVA_JPEG_MAX_RESTART && lim.block_bits == kBlockBits && lim.lds_bytes == kLdsBytes);
  EXPECT(refused(deva_jpeg_limits(nullptr), "null limits"));
  EXPECT(refused(deva_jpeg_plan(4, 4, 420, 0, nullptr), "null plan"));
  EXPECT(refused(deva_jpeg_quant(75, nullptr), "null tables"));
  uint8_t dqt[128];
  EXPECT(refused(deva_jpeg_quant(0, dqt), "quality: 1 to 100"));
  EXPECT(deva_jpeg_version() == DEVA_JPEG_ABI_VERSION);
}

int main() {
  sweep_plans();
  sweep_tables();
  sweep_refusals();
  printf("%lld %lld %lld\n", g_checks, g_refused, g_failures);
  return g_failures ? 1 : 0;
}
