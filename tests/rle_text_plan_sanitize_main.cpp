// csrc/rle_text/rle_text_plan.cpp under the host sanitizers, in a program of its own (tests/test_rle_text_cpu.py builds it
// with -fsanitize=address,undefined and runs it; nothing is loaded into Python and no GPU is involved).
//
// It sweeps the launch decision over sizes up to the largest plane there is, mask numbers around the limits and text
// lengths around 2^26 words and 2^31 characters, holds every plan to its own arithmetic, holds deva_text_max_chars to
// the widths of C1 on both sides of every edge, carves the parser's scratch of the accepted calls in a host buffer of
// exactly the size asked for, and sends every argument check of the three launchers through its refusals with made-up
// addresses.  Prints "<checks> <refused> <failures>".
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "rle_text_plan.h"

using namespace deva_text;

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
  const int sizes[] = {1, 2, 9, 33, 63, 64, 65, 480, 854, 1080, 1920, 4096, 46340, 46341, 65536, 1 << 20};
  const int masks[] = {-1, 0, 1, 2, 255, 256, 257, 513, 65535, 65536, 65537};
  const int64_t texts[] = {-1, 0, 1, 1023, 1024, 1025, (1ll << 26) - 131074, (1ll << 26) - 3, (1ll << 26) - 2, (1ll << 26) - 1, 1ll << 26,
                           (1ll << 31) - 1, 1ll << 31};
  for (int h : sizes)
    for (int w : sizes)
      for (int n : masks)
        for (int64_t chars : texts) {
          struct deva_text_plan p;
          memset(&p, 0x5a, sizeof(p));
          const int rc = text_plan("sweep", n, h, w, chars, &p);
          if ((int64_t)h * w > kMaxPixels) {
            EXPECT(refused(rc, "bad height x width"));
            continue;
          }
          if (n < 0 || n > DEVA_TEXT_MAX_MASKS) {
            EXPECT(refused(rc, "n: 0 to"));
            continue;
          }
          if (chars < 0 || chars > kMaxText) {
            EXPECT(refused(rc, "chars_len: 0 to"));
            continue;
          }
          const int64_t words = 2ll * n + 1 + chars;
          if (words > DEVA_TEXT_MAX_WORDS) {
            EXPECT(refused(rc, "words, a call takes"));
            continue;
          }
          EXPECT(rc == 0);
          EXPECT(p.mask_grid == (uint32_t)n && p.scan_grid == (n ? 1u : 0u) && p.items == kItems && p.reserved == 0);
          EXPECT(p.mask_chunks == (n + DEVA_TEXT_MASK_CHUNK - 1) / DEVA_TEXT_MASK_CHUNK);
          EXPECT(p.min_words == words && p.parse_scratch_bytes == 8ll * n && p.parse_scratch_bytes == deva_text_parse_scratch(n));
          EXPECT(p.value_chars == deva_text_max_chars((int64_t)h * w) && p.value_chars >= 1 && p.value_chars <= 7);
          if (n > 0 && n <= 4096) {          // the carved pieces lie inside the bytes asked for and do not meet
            std::vector<int32_t> host(p.parse_scratch_bytes / 4, 0);
            const Scratch sc = carve(host.data(), n);
            sc.values[0] = 1;
            sc.values[n - 1] = 2;
            sc.flags[0] = 3;
            sc.flags[n - 1] = 4;
            EXPECT(sc.flags == sc.values + n && host.back() == 4 && host.front() == (n == 1 ? 2 : 1));
          }
        }
  EXPECT(deva_text_parse_scratch(-1) == -1 && deva_text_parse_scratch(DEVA_TEXT_MAX_MASKS + 1) == -1);
}

static void sweep_widths() {
  // C1: k characters hold the values -2^(5k-1) .. 2^(5k-1) - 1
  for (int k = 1; k <= 12; ++k) {
    const int64_t edge = 1ll << (5 * k - 1);
    EXPECT(value_chars(edge - 1) == k && value_chars(edge) == k + 1 && value_chars(-edge) == k && value_chars(-edge - 1) == k + 1);
  }
  EXPECT(value_chars(0) == 1 && value_chars(-1) == 1 && value_chars(INT64_MAX) == 13 && value_chars(INT64_MIN) == 13);
  EXPECT(deva_text_max_chars(0) == -1 && deva_text_max_chars(-5) == -1 && deva_text_max_chars(1ll << 31) == -1);
  EXPECT(deva_text_max_chars(1) == 1 && deva_text_max_chars(15) == 1 && deva_text_max_chars(16) == 2 && deva_text_max_chars(17) == 2);
  EXPECT(deva_text_max_chars(480 * 854) == 4 && deva_text_max_chars(1080 * 1920) == 5 && deva_text_max_chars((1ll << 31) - 1) == 7);
  for (int64_t total = 1; total < (1ll << 31); total = total * 3 + 1) {
    const int widest = deva_text_max_chars(total);
    EXPECT(value_chars(total) <= widest && value_chars(-total) <= widest && (value_chars(total) == widest || value_chars(-total) == widest));
  }
}

static void sweep_refusals() {
  // made-up device addresses: every check fails or passes before anything is dereferenced
  char* const A = reinterpret_cast<char*>(1ll << 40);
  const int n = 3, h = 65, w = 129;
  const int64_t bounds_len = 100, capacity = 500, chars_len = 40, words_cap = 2 * n + 1 + chars_len;
  const int32_t* n_in = reinterpret_cast<int32_t*>(A);
  const int64_t* base = reinterpret_cast<int64_t*>(A + (1 << 20));
  const int32_t* bounds = reinterpret_cast<int32_t*>(A + (2 << 20));
  int32_t* text_len = reinterpret_cast<int32_t*>(A + (3 << 20));
  int64_t* text_base = reinterpret_cast<int64_t*>(A + (4 << 20));
  int64_t* text_total = reinterpret_cast<int64_t*>(A + (5 << 20));
  int64_t* first = reinterpret_cast<int64_t*>(A + (6 << 20));
  uint8_t* chars = reinterpret_cast<uint8_t*>(A + (7 << 20) + 1);      // (texts begin at any byte address)
  int64_t* text_first = reinterpret_cast<int64_t*>(A + (8 << 20));
  void* scratch = A + (9 << 20);
  int32_t* runs = reinterpret_cast<int32_t*>(A + (10 << 20));
  int64_t* info = reinterpret_cast<int64_t*>(A + (11 << 20));
  auto count = [&](const int32_t* ni, const int64_t* b, const int32_t* bo, int64_t bl, int n_, int h_, int w_, const int32_t* tl, const int64_t* tb,
                   const int64_t* tt, const int64_t* f) { return count_check(ni, b, bo, bl, n_, h_, w_, tl, tb, tt, f, nullptr); };
  EXPECT(count(n_in, base, bounds, bounds_len, n, h, w, text_len, text_base, text_total, first) == 0);
  EXPECT(count(n_in, base, nullptr, 0, n, h, w, text_len, text_base, text_total, nullptr) == 0);
  EXPECT(count(nullptr, nullptr, nullptr, 0, 0, h, w, nullptr, nullptr, nullptr, nullptr) == 0);                 // no masks: no work
  EXPECT(refused(count(n_in, base, bounds, bounds_len, -1, h, w, text_len, text_base, text_total, first), "n: 0 to"));
  EXPECT(refused(count(n_in, base, bounds, bounds_len, DEVA_TEXT_MAX_MASKS + 1, h, w, text_len, text_base, text_total, first), "n: 0 to"));
  EXPECT(refused(count(n_in, base, bounds, bounds_len, n, 0, w, text_len, text_base, text_total, first), "bad height x width"));
  EXPECT(refused(count(n_in, base, bounds, bounds_len, n, 46341, 46341, text_len, text_base, text_total, first), "bad height x width"));
  EXPECT(refused(count(n_in, base, bounds, -1, n, h, w, text_len, text_base, text_total, first), "bounds_len"));
  EXPECT(refused(count(nullptr, base, bounds, bounds_len, n, h, w, text_len, text_base, text_total, first), "n_in"));
  EXPECT(refused(count(reinterpret_cast<const int32_t*>(A + 2), base, bounds, bounds_len, n, h, w, text_len, text_base, text_total, first), "n_in"));
  EXPECT(refused(count(n_in, nullptr, bounds, bounds_len, n, h, w, text_len, text_base, text_total, first), "base"));
  EXPECT(refused(count(n_in, reinterpret_cast<const int64_t*>(A + (1 << 20) + 4), bounds, bounds_len, n, h, w, text_len, text_base, text_total, first), "base"));
  EXPECT(refused(count(n_in, base, nullptr, bounds_len, n, h, w, text_len, text_base, text_total, first), "bounds: null"));
  EXPECT(refused(count(n_in, base, reinterpret_cast<const int32_t*>(A + (2 << 20) + 1), bounds_len, n, h, w, text_len, text_base, text_total, first), "bounds"));
  EXPECT(refused(count(n_in, base, bounds, bounds_len, n, h, w, nullptr, text_base, text_total, first), "text_len"));
  EXPECT(refused(count(n_in, base, bounds, bounds_len, n, h, w, text_len, nullptr, text_total, first), "text_base"));
  EXPECT(refused(count(n_in, base, bounds, bounds_len, n, h, w, text_len, text_base, nullptr, first), "text_total"));
  EXPECT(refused(count(n_in, base, bounds, bounds_len, n, h, w, text_len, text_base, text_total, text_total), "first"));
  EXPECT(refused(count(n_in, base, bounds, bounds_len, n, h, w, text_len, text_base, text_total, reinterpret_cast<int64_t*>(A + (6 << 20) + 4)), "first"));
  EXPECT(refused(count(n_in, base, bounds, bounds_len, n, h, w, const_cast<int32_t*>(n_in + 2), text_base, text_total, first), "text_len overlaps n_in"));
  EXPECT(refused(count(n_in, base, bounds, bounds_len, n, h, w, text_len, const_cast<int64_t*>(base + 2), text_total, first), "text_base overlaps base"));
  EXPECT(refused(count(n_in, base, bounds, bounds_len, n, h, w, const_cast<int32_t*>(bounds + 99), text_base, text_total, first), "text_len overlaps bounds"));
  EXPECT(refused(count(n_in, base, bounds, bounds_len, n, h, w, text_len, text_base, text_base + 2, first), "overlaps"));
  EXPECT(refused(count(n_in, base, bounds, bounds_len, n, h, w, text_len, text_base, text_total, text_base + 1), "text_base overlaps first"));
  auto write = [&](const int32_t* ni, const int64_t* b, const int32_t* bo, int64_t bl, int n_, int h_, int w_, const int64_t* tb, const uint8_t* c,
                   int64_t cap) { return write_check(ni, b, bo, bl, n_, h_, w_, tb, c, cap, nullptr); };
  EXPECT(write(n_in, base, bounds, bounds_len, n, h, w, text_base, chars, capacity) == 0);
  EXPECT(write(n_in, base, bounds, bounds_len, n, h, w, text_base, nullptr, 0) == 0);
  EXPECT(write(nullptr, nullptr, nullptr, 0, 0, h, w, nullptr, nullptr, 0) == 0);
  EXPECT(refused(write(n_in, base, bounds, bounds_len, n, h, w, text_base, chars, -1), "capacity"));
  EXPECT(refused(write(n_in, base, bounds, bounds_len, n, h, w, text_base, chars, (1ll << 60) + 1), "capacity"));
  EXPECT(refused(write(n_in, base, bounds, bounds_len, n, h, w, text_base, nullptr, 5), "chars: null"));
  EXPECT(refused(write(n_in, base, bounds, bounds_len, n, h, w, nullptr, chars, 5), "text_base"));
  EXPECT(refused(write(nullptr, base, bounds, bounds_len, n, h, w, text_base, chars, 5), "n_in"));
  EXPECT(refused(write(n_in, base, bounds, bounds_len, n, h, 0, text_base, chars, 5), "bad height x width"));
  EXPECT(refused(write(n_in, base, bounds, bounds_len, n, h, w, text_base, reinterpret_cast<const uint8_t*>(bounds) + 399, 5), "chars overlaps bounds"));
  EXPECT(refused(write(n_in, base, bounds, bounds_len, n, h, w, text_base, reinterpret_cast<const uint8_t*>(text_base) - 4, 5), "chars overlaps text_base"));
  auto parse = [&](const uint8_t* c, int64_t cl, const int64_t* tf, int n_, int h_, int w_, const void* sc, int64_t sb, const int32_t* r, int64_t wc,
                   const int64_t* i) { return parse_check(c, cl, tf, n_, h_, w_, sc, sb, r, wc, i, nullptr); };
  EXPECT(parse(chars, chars_len, text_first, n, h, w, scratch, 8 * n, runs, words_cap, info) == 0);
  EXPECT(parse(nullptr, 0, text_first, n, h, w, scratch, 8 * n, runs, 2 * n + 1, info) == 0);
  EXPECT(parse(nullptr, 0, text_first, 0, h, w, nullptr, 0, runs, 1, info) == 0);
  EXPECT(refused(parse(chars, chars_len, text_first, n, h, w, scratch, 8 * n, runs, words_cap - 1, info), "words_cap"));
  EXPECT(refused(parse(chars, chars_len, text_first, n, h, w, scratch, 8 * n, runs, DEVA_TEXT_MAX_WORDS + 1ll, info), "words_cap"));
  EXPECT(refused(parse(chars, 1ll << 31, text_first, n, h, w, scratch, 8 * n, runs, words_cap, info), "chars_len"));
  EXPECT(refused(parse(chars, -1, text_first, n, h, w, scratch, 8 * n, runs, words_cap, info), "chars_len"));
  EXPECT(refused(parse(chars, 1ll << 26, text_first, n, h, w, scratch, 8 * n, runs, words_cap, info), "words, a call takes"));
  EXPECT(refused(parse(nullptr, chars_len, text_first, n, h, w, scratch, 8 * n, runs, words_cap, info), "chars: null"));
  EXPECT(refused(parse(chars, chars_len, nullptr, n, h, w, scratch, 8 * n, runs, words_cap, info), "text_first"));
  EXPECT(refused(parse(chars, chars_len, reinterpret_cast<int64_t*>(A + 4), n, h, w, scratch, 8 * n, runs, words_cap, info), "text_first"));
  EXPECT(refused(parse(chars, chars_len, text_first, n, h, w, nullptr, 8 * n, runs, words_cap, info), "scratch: null"));
  EXPECT(refused(parse(chars, chars_len, text_first, n, h, w, A + 2, 8 * n, runs, words_cap, info), "scratch: null or not 4-byte"));
  EXPECT(refused(parse(chars, chars_len, text_first, n, h, w, scratch, 8 * n - 1, runs, words_cap, info), "scratch_bytes"));
  EXPECT(refused(parse(chars, chars_len, text_first, n, h, w, scratch, 8 * n, nullptr, words_cap, info), "runs"));
  EXPECT(refused(parse(chars, chars_len, text_first, n, h, w, scratch, 8 * n, runs, words_cap, nullptr), "info"));
  EXPECT(refused(parse(chars, chars_len, text_first, n, h, w, scratch, 8 * n, runs, words_cap, reinterpret_cast<int64_t*>(A + 4)), "info"));
  EXPECT(refused(parse(chars, chars_len, text_first, n, -3, w, scratch, 8 * n, runs, words_cap, info), "bad height x width"));
  EXPECT(refused(parse(chars, chars_len, text_first, n, h, w, scratch, 8 * n, reinterpret_cast<int32_t*>(chars + 3), words_cap, info), "runs overlaps chars"));
  EXPECT(refused(parse(chars, chars_len, text_first, n, h, w, scratch, 8 * n, reinterpret_cast<int32_t*>(text_first + n), words_cap, info),
                 "runs overlaps text_first"));
  EXPECT(refused(parse(chars, chars_len, text_first, n, h, w, scratch, 8 * n, runs, words_cap, reinterpret_cast<int64_t*>(runs + words_cap - 1)), "overlaps"));
  EXPECT(refused(parse(chars, chars_len, text_first, n, h, w, runs + words_cap - 1, 8 * n, runs, words_cap, info), "overlaps"));
  struct deva_text_limits lim;
  EXPECT(deva_text_limits(&lim) == 0 && lim.max_masks == DEVA_TEXT_MAX_MASKS && lim.max_words == DEVA_TEXT_MAX_WORDS && lim.block == kBlock &&
         lim.max_chars == DEVA_TEXT_MAX_CHARS && lim.scan_chunk == DEVA_TEXT_SCAN_CHUNK && lim.mask_chunk == DEVA_TEXT_MASK_CHUNK);
  EXPECT(refused(deva_text_limits(nullptr), "null limits"));
  EXPECT(refused(deva_text_plan(1, 4, 4, 0, nullptr), "null plan"));
  EXPECT(deva_text_version() == DEVA_TEXT_ABI_VERSION);
}

int main() {
  sweep_plans();
  sweep_widths();
  sweep_refusals();
  printf("%lld %lld %lld\n", g_checks, g_refused, g_failures);
  return g_failures ? 1 : 0;
}
