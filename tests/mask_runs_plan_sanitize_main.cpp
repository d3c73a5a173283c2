// csrc/mask_runs/mask_runs_plan.cpp under the host sanitizers, in a program of its own (tests/test_mask_runs_cpu.py
// builds it with -fsanitize=address,undefined and runs it; nothing is loaded into Python and no GPU is involved).
//
// It sweeps the launch decision over sizes up to the largest plane there is and over mask numbers around the limits,
// holds every plan to its own arithmetic (tiles, segments, scan steps, grids, scratch bytes; nothing beyond an int32 or
// the scratch limit), carves the scratch of the accepted calls and touches the first and last word of both pieces in a
// host buffer of exactly the size asked for, and sends every argument check of deva_runs_count and deva_runs_write
// through its refusals with made-up addresses.  Prints "<checks> <refused> <failures>".
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "mask_runs_plan.h"

using namespace deva_runs;

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
  const int sizes[] = {1, 2, 9, 33, 63, 64, 65, 67, 127, 128, 129, 144, 480, 854, 1080, 1920, 2048, 2049, 4096, 46340, 46341, 65536, 1 << 20};
  const int masks[] = {0, 1, 2, 3, 64, 255, 256, 257, 300, 4096, 65535, 65536};
  for (int h : sizes)
    for (int w : sizes)
      for (int n : masks) {
        struct deva_runs_plan p;
        memset(&p, 0x5a, sizeof(p));
        const int rc = runs_plan("sweep", n, h, w, &p);
        const int64_t tiles_y = ((int64_t)h + kTile - 1) / kTile, tiles_x = ((int64_t)w + kTile - 1) / kTile;
        const int64_t segments = (int64_t)w * tiles_y, bytes = (int64_t)n * segments * kSegmentBytes;
        if ((int64_t)h * w > kMaxPixels) {
          EXPECT(refused(rc, "bad height x width"));
          EXPECT(deva_runs_scratch(n, h, w) == -1);
          continue;
        }
        if (bytes > DEVA_RUNS_MAX_SCRATCH) {
          EXPECT(refused(rc, "bytes of scratch"));
          EXPECT(deva_runs_scratch(n, h, w) == -1);
          continue;
        }
        EXPECT(rc == 0);
        EXPECT(p.tiles_x == tiles_x && p.tiles_y == tiles_y && p.segments == segments && p.scratch_bytes == bytes);
        EXPECT(p.scan_chunks == (segments + DEVA_RUNS_SCAN_CHUNK - 1) / DEVA_RUNS_SCAN_CHUNK);
        EXPECT(p.mask_chunks == (n + DEVA_RUNS_MASK_CHUNK - 1) / DEVA_RUNS_MASK_CHUNK);
        const int64_t tiles = n * tiles_x * tiles_y, groups = n * ((segments + kBlock - 1) / kBlock);
        EXPECT(p.count_grid == (tiles < kMaxGrid ? tiles : kMaxGrid) && p.write_grid == (groups < kMaxGrid ? groups : kMaxGrid));
        EXPECT((n == 0) == (p.count_grid == 0) && (n == 0) == (p.write_grid == 0));
        EXPECT(deva_runs_scratch(n, h, w) == bytes && bytes % 4 == 0);
        if (n > 0 && bytes <= (1 << 22)) {     // the carved pieces lie inside the bytes asked for and do not meet
          std::vector<int32_t> host(bytes / 4, 0);
          const Scratch sc = carve(host.data(), n, p);
          sc.off[0] = 1;
          sc.off[(int64_t)n * segments - 1] = 2;
          sc.bits[0] = 3;
          sc.bits[2 * (int64_t)n * segments - 1] = 4;
          EXPECT(reinterpret_cast<int32_t*>(sc.bits) == sc.off + (int64_t)n * segments);
          EXPECT(host.front() == (n * segments == 1 ? 2 : 1) && host.back() == 4);
        }
      }
}

static void sweep_refusals() {
  // made-up device addresses: every check fails or passes before anything is dereferenced
  char* const A = reinterpret_cast<char*>(1ll << 40);
  const int n = 3, h = 65, w = 129;
  struct deva_runs_plan p;
  EXPECT(runs_plan("x", n, h, w, &p) == 0);
  const int64_t need = p.scratch_bytes, plane_bytes = (int64_t)n * h * w * 4;
  void* planes = A;
  void* scratch = A + (1 << 28);
  int32_t* n_out = reinterpret_cast<int32_t*>(A + (2 << 28));
  int64_t* base = reinterpret_cast<int64_t*>(A + (3 << 28));
  int64_t* total = reinterpret_cast<int64_t*>(A + (4 << 28));
  int64_t* first = reinterpret_cast<int64_t*>(A + (5 << 28));
  int32_t* stats = reinterpret_cast<int32_t*>(A + (6 << 28));
  int32_t* bounds = reinterpret_cast<int32_t*>(A + (7ll << 28));
  auto count = [&](const void* pl, int dtype, int n_, int h_, int w_, const void* sc, int64_t sb, const int32_t* no, const int64_t* b,
                   const int64_t* t, const int64_t* f, const int32_t* s) { return count_check(pl, dtype, n_, h_, w_, sc, sb, no, b, t, f, s, nullptr); };
  EXPECT(count(planes, DEVA_RUNS_F32, n, h, w, scratch, need, n_out, base, total, first, stats) == 0);
  EXPECT(count(A + 1, DEVA_RUNS_U8, n, h, w, scratch, need, n_out, base, total, nullptr, nullptr) == 0);      // E7: any byte address
  EXPECT(count(nullptr, 0, 0, h, w, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == 0);           // no masks: no work
  EXPECT(refused(count(planes, 2, n, h, w, scratch, need, n_out, base, total, first, stats), "dtype"));
  EXPECT(refused(count(planes, 0, -1, h, w, scratch, need, n_out, base, total, first, stats), "n: 0 to"));
  EXPECT(refused(count(planes, 0, DEVA_RUNS_MAX_MASKS + 1, h, w, scratch, need, n_out, base, total, first, stats), "n: 0 to"));
  EXPECT(refused(count(planes, 0, n, 0, w, scratch, need, n_out, base, total, first, stats), "bad height x width"));
  EXPECT(refused(count(planes, 0, n, 46341, 46341, scratch, need, n_out, base, total, first, stats), "bad height x width"));
  EXPECT(refused(count(planes, 0, 65536, 1080, 1920, scratch, need, n_out, base, total, first, stats), "bytes of scratch"));
  EXPECT(refused(count(nullptr, 0, n, h, w, scratch, need, n_out, base, total, first, stats), "planes"));
  EXPECT(refused(count(A + 2, DEVA_RUNS_F32, n, h, w, scratch, need, n_out, base, total, first, stats), "planes"));
  EXPECT(refused(count(planes, 0, n, h, w, nullptr, need, n_out, base, total, first, stats), "scratch: null"));
  EXPECT(refused(count(planes, 0, n, h, w, A + (1 << 28) + 2, need, n_out, base, total, first, stats), "scratch: null or not 4-byte"));
  EXPECT(refused(count(planes, 0, n, h, w, scratch, need - 1, n_out, base, total, first, stats), "scratch_bytes"));
  EXPECT(refused(count(planes, 0, n, h, w, scratch, need, nullptr, base, total, first, stats), "n_out"));
  EXPECT(refused(count(planes, 0, n, h, w, scratch, need, n_out, nullptr, total, first, stats), "base"));
  EXPECT(refused(count(planes, 0, n, h, w, scratch, need, n_out, reinterpret_cast<int64_t*>(A + (3 << 28) + 4), total, first, stats), "base"));
  EXPECT(refused(count(planes, 0, n, h, w, scratch, need, n_out, base, nullptr, first, stats), "total"));
  EXPECT(refused(count(planes, 0, n, h, w, scratch, need, n_out, base, total, total, stats), "first"));
  EXPECT(refused(count(planes, 0, n, h, w, scratch, need, n_out, base, total, reinterpret_cast<int64_t*>(A + (5 << 28) + 4), stats), "first"));
  EXPECT(refused(count(planes, 0, n, h, w, scratch, need, n_out, base, total, first, reinterpret_cast<int32_t*>(A + (6 << 28) + 2)), "stats"));
  EXPECT(refused(count(planes, DEVA_RUNS_F32, n, h, w, A + plane_bytes - 4, need, n_out, base, total, first, stats), "scratch overlaps the planes"));
  EXPECT(refused(count(planes, 0, n, h, w, scratch, need, n_out, reinterpret_cast<int64_t*>(n_out + 2), total, first, stats), "overlaps"));
  EXPECT(refused(count(planes, 0, n, h, w, scratch, need, n_out, base, base + n - 1, first, stats), "overlaps"));
  EXPECT(refused(count(planes, 0, n, h, w, scratch, need, n_out, base, total, base, stats), "overlaps first"));
  EXPECT(refused(count(planes, 0, n, h, w, scratch, need, n_out, base, total, first, n_out + n - 1), "overlaps"));
  auto write = [&](int n_, int h_, int w_, const void* sc, int64_t sb, const int64_t* b, const int32_t* bo, int64_t cap) {
    return write_check(n_, h_, w_, sc, sb, b, bo, cap, nullptr);
  };
  EXPECT(write(n, h, w, scratch, need, base, bounds, 1000) == 0);
  EXPECT(write(n, h, w, scratch, need, base, nullptr, 0) == 0);
  EXPECT(write(0, h, w, nullptr, 0, nullptr, nullptr, 0) == 0);
  EXPECT(refused(write(n, h, w, scratch, need, base, bounds, -1), "capacity"));
  EXPECT(refused(write(n, h, w, scratch, need, base, bounds, (1ll << 60) + 1), "capacity"));
  EXPECT(refused(write(n, h, w, scratch, need, base, nullptr, 5), "bounds"));
  EXPECT(refused(write(n, h, w, scratch, need, base, reinterpret_cast<int32_t*>(A + (7ll << 28) + 2), 5), "bounds"));
  EXPECT(refused(write(n, h, w, nullptr, need, base, bounds, 5), "scratch: null"));
  EXPECT(refused(write(n, h, w, scratch, need - 4, base, bounds, 5), "scratch_bytes"));
  EXPECT(refused(write(n, h, w, scratch, need, nullptr, bounds, 5), "base"));
  EXPECT(refused(write(n, h, 0, scratch, need, base, bounds, 5), "bad height x width"));
  EXPECT(refused(write(n, h, w, scratch, need, base, reinterpret_cast<int32_t*>(A + (1 << 28) - 8), 5), "bounds overlaps scratch"));
  EXPECT(refused(write(n, h, w, scratch, need, base, reinterpret_cast<int32_t*>(base + 1), 5), "bounds overlaps base"));
  struct deva_runs_limits lim;
  EXPECT(deva_runs_limits(&lim) == 0 && lim.max_masks == DEVA_RUNS_MAX_MASKS && lim.max_scratch == DEVA_RUNS_MAX_SCRATCH && lim.tile == kTile);
  EXPECT(refused(deva_runs_limits(nullptr), "null limits"));
  EXPECT(refused(deva_runs_plan(1, 4, 4, nullptr), "null plan"));
  EXPECT(deva_runs_version() == DEVA_RUNS_ABI_VERSION);
}

int main() {
  sweep_plans();
  sweep_refusals();
  printf("%lld %lld %lld\n", g_checks, g_refused, g_failures);
  return g_failures ? 1 : 0;
}
