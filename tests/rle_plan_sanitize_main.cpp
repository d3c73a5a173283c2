// Stand-alone host program for tests/test_rle_cpu.py: the HIP-free side of the run-length decoder under the host
// sanitizers.  Three parts:
//  1. csrc/rle/rle_plan.cpp: the launch decision over the product of its boundary values, and every check of
//     deva_rle_decode with made-up device addresses (nothing on the device side is dereferenced).
//  2. rule D2 (runs_check) on run arrays that are heap blocks of exactly their size: valid ones, and each of them broken in
//     every way D2 names, the index words included.  A check that read outside an array would be caught here.
//  3. csrc/rle/rle_walk.h, the arithmetic of the kernel, driven as the kernel drives it (a tile of 64 x 64, a column and
//     16 rows a lane, shifted rows, 16-byte pieces) into an output block of exactly its size at every misalignment,
//     against a decoder written as a loop: every element written once, every whole piece aligned, nothing outside.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "deva_rle.h"
#include "rle_plan.h"
#include "rle_walk.h"

static long g_calls = 0, g_refused = 0, g_failed = 0;

static void fail(const char* what, long a, long b, long c, long d) {
  ++g_failed;
  fprintf(stderr, "FAIL %s: %ld %ld %ld %ld (%s)\n", what, a, b, c, d, deva_rle_last_error());
}

static void tally(int e, bool want, const char* text, const char* what, long a, long b, long c, long d) {
  ++g_calls;
  if (e != 0) ++g_refused;
  if ((e == 0) != want) fail(what, a, b, c, d);
  if (e != 0 && (e != 2 || !strstr(deva_rle_last_error(), text))) fail("refusal text", a, b, c, d);
  deva_rle::set_error("%s", "");
}

static uint64_t g_seed = 0x9e3779b97f4a7c15ull;
static uint32_t rnd(uint32_t below) {
  g_seed = g_seed * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(g_seed >> 33) % below;
}

// ------------------------------------------------------------------------------------------ 1. the plan
static void plan_cases() {
  const int sides[] = {-1, 0, 1, 2, 63, 64, 65, 46340, 46341, 65536, INT32_MAX};
  const int counts[] = {-1, 0, 1, 7, DEVA_RLE_MAX_MASKS, DEVA_RLE_MAX_MASKS + 1};
  for (int n : counts)
    for (int h : sides)
      for (int w : sides)
        for (int oh : {0, 1, 65, 46341})
          for (int ow : {1, 64, 46341, INT32_MAX})
            for (int dtype : {-1, DEVA_RLE_U8, DEVA_RLE_F32, 2}) {
              auto ok = [](int a, int b) { return a > 0 && b > 0 && (int64_t)a * b < (1ll << 31); };
              const bool want = ok(h, w) && ok(oh, ow) && n >= 0 && n <= DEVA_RLE_MAX_MASKS && (dtype == 0 || dtype == 1);
              struct deva_rle_plan plan;
              memset(&plan, 0xff, sizeof(plan));
              const int e = deva_rle_plan(n, h, w, oh, ow, dtype, &plan);
              tally(e, want, "deva_rle_plan", "plan", n, h, oh, ow);
              if (e == 0) {
                const int64_t tiles = (int64_t)n * plan.tiles_x * plan.tiles_y;
                if (plan.tiles_x != ((int64_t)ow + 63) / 64 || plan.tiles_y != ((int64_t)oh + 63) / 64 || plan.grid > 65536u ||
                    plan.grid != (uint32_t)(tiles < 65536 ? tiles : 65536) || plan.lds_bytes != 64 * 80 ||
                    plan.out_bytes != (int64_t)n * oh * ow * (dtype ? 4 : 1) || plan.scale_y != (float)h / (float)oh)
                  fail("plan fields", n, h, oh, ow);
              }
            }
  tally(deva_rle_plan(1, 4, 4, 4, 4, 0, nullptr), false, "null plan", "null plan", 0, 0, 0, 0);
  tally(deva_rle_limits(nullptr), false, "null limits", "null limits", 0, 0, 0, 0);
  struct deva_rle_limits lim;
  tally(deva_rle_limits(&lim), true, "", "limits", 0, 0, 0, 0);
  if (lim.max_masks != DEVA_RLE_MAX_MASKS || lim.max_words != DEVA_RLE_MAX_WORDS || lim.tile != 64 || lim.block != 256) fail("limits", 0, 0, 0, 0);
}

// ------------------------------------------------------------------------------------------ 2. D2
// counts of every mask -> the run array, a heap block of exactly its words
static std::vector<int32_t> run_array(const std::vector<std::vector<int>>& masks) {
  const int n = (int)masks.size();
  std::vector<int32_t> words(n + 1, 0);
  for (int k = 0; k < n; ++k) words[k + 1] = words[k] + (int32_t)masks[k].size() + 1;
  for (const auto& c : masks) {
    int32_t s = 0;
    words.push_back(0);
    for (int v : c) words.push_back(s += v);
  }
  words.shrink_to_fit();
  return std::vector<int32_t>(words);   // (a copy: capacity == size, so the sanitizer sees the true end)
}

// random counts that sum to total, with zeros in front, inside (also twice in a row) and at the end
static std::vector<int> random_counts(int total) {
  std::vector<int> c;
  int left = total;
  if (rnd(3) == 0) c.push_back(0);
  while (left > 0) {
    const int v = rnd(4) == 0 ? 0 : 1 + (int)rnd((uint32_t)(left < 9 ? left : 9));
    c.push_back(v > left ? left : v);
    left -= c.back();
    if (rnd(8) == 0) c.push_back(0), c.push_back(0);
  }
  if (rnd(3) == 0) c.push_back(0);
  return c;
}

static void d2_cases() {
  char name[32];
  for (int round = 0; round < 300; ++round) {
    const int h = 1 + (int)rnd(9), w = 1 + (int)rnd(9), n = 1 + (int)rnd(5);
    std::vector<std::vector<int>> masks;
    for (int k = 0; k < n; ++k) masks.push_back(random_counts(h * w));
    const std::vector<int32_t> good = run_array(masks);
    tally(deva_rle_check(good.data(), (int64_t)good.size(), n, h, w), true, "", "valid run array", round, n, h, w);
    const int k = (int)rnd(n);
    snprintf(name, sizeof(name), "mask %d:", k);
    for (int way = 0; way < 4; ++way) {   // a count of -1, a sum one short, one long, no counts at all: each names mask k
      auto broken = masks;
      auto& c = broken[k];
      if (way == 0) {
        size_t at = rnd((uint32_t)c.size());
        c[at] += 1;   // (the sum stays: the count after it, or a new one, takes the -1)
        if (at + 1 < c.size() && c[at + 1] == 0) c[at + 1] = -1; else c.insert(c.begin() + at + 1, -1);
      } else if (way == 1) {
        size_t at = 0;
        while (c[at] == 0) ++at;
        c[at] -= 1;
      } else if (way == 2) {
        c.back() += 1;
      } else {
        c.clear();
      }
      const std::vector<int32_t> bad = run_array(broken);
      const int e = deva_rle_check(bad.data(), (int64_t)bad.size(), n, h, w);
      if (e != 0 && !strstr(deva_rle_last_error(), way == 0 ? "is negative" : way == 3 ? "no counts" : "the counts sum to"))
        fail("the text of a broken mask", round, way, k, n);
      tally(e, false, name, "broken counts", round, way, k, n);
    }
    // the index words: every one of them set to values that point outside the array, the word count off by one
    for (int at = 0; at <= n; ++at)
      for (int32_t v : {-1, 1, (int32_t)good.size(), INT32_MAX, INT32_MIN}) {
        std::vector<int32_t> bad(good);
        if (bad[at] == v) continue;
        bad[at] = v;
        tally(deva_rle_check(bad.data(), (int64_t)bad.size(), n, h, w), false, "deva_rle_check", "broken index", round, at, v, n);
      }
    tally(deva_rle_check(good.data(), (int64_t)good.size() - 1, n, h, w), false, "deva_rle_check", "a word short", round, n, h, w);
    tally(deva_rle_check(good.data(), n, n, h, w), false, "words", "the index alone", round, n, h, w);
    tally(deva_rle_check(good.data(), (int64_t)good.size(), n, h + 1, w), false, "mask 0:", "another size", round, n, h, w);
  }
  const int32_t none[1] = {0};
  tally(deva_rle_check(none, 1, 0, 3, 3), true, "", "no masks", 0, 0, 0, 0);
  tally(deva_rle_check(nullptr, 1, 0, 3, 3), false, "null run array", "null", 0, 0, 0, 0);
  tally(deva_rle_check(none, (int64_t)DEVA_RLE_MAX_WORDS + 1, 0, 3, 3), false, "words", "too many words", 0, 0, 0, 0);
  // deva_rle_decode's own: made-up device addresses, refused before anything could be launched
  const std::vector<int32_t> good = run_array({{4, 5}, {0, 9}});
  const int32_t* dev = reinterpret_cast<const int32_t*>(uintptr_t(1) << 40);
  char* out = reinterpret_cast<char*>(uintptr_t(1) << 41);
  struct deva_rle_plan plan;
  using deva_rle::decode_check;
  tally(decode_check(good.data(), dev, good.size(), 2, 3, 3, 6, 5, DEVA_RLE_F32, out, &plan), true, "", "decode_check", 0, 0, 0, 0);
  tally(decode_check(good.data(), dev, good.size(), 2, 3, 3, 6, 5, DEVA_RLE_F32, out + 2, &plan), false, "misaligned out", "out", 0, 0, 0, 0);
  tally(decode_check(good.data(), dev, good.size(), 2, 3, 3, 6, 5, DEVA_RLE_U8, out + 3, nullptr), true, "", "a byte address", 0, 0, 0, 0);
  tally(decode_check(good.data(), dev, good.size(), 2, 3, 3, 6, 5, DEVA_RLE_U8, nullptr, &plan), false, "null or misaligned out", "null out", 0, 0, 0, 0);
  tally(decode_check(good.data(), nullptr, good.size(), 2, 3, 3, 6, 5, DEVA_RLE_U8, out, &plan), false, "run array on the device", "null runs", 0, 0, 0, 0);
  tally(decode_check(nullptr, dev, good.size(), 2, 3, 3, 6, 5, DEVA_RLE_U8, out, &plan), false, "null run array", "null host runs", 0, 0, 0, 0);
  tally(decode_check(good.data(), reinterpret_cast<const int32_t*>(out + 56), good.size(), 2, 3, 3, 6, 5, DEVA_RLE_U8, out, &plan), false,
        "overlaps", "overlap", 0, 0, 0, 0);
  tally(decode_check(good.data(), dev, good.size(), 2, 3, 4, 6, 5, DEVA_RLE_U8, out, &plan), false, "mask 0:", "size", 0, 0, 0, 0);
  tally(decode_check(nullptr, nullptr, 0, 0, 3, 3, 6, 5, DEVA_RLE_U8, nullptr, &plan), true, "", "no masks is no work", 0, 0, 0, 0);
}

// ------------------------------------------------------------------------------------------ 3. the kernel's arithmetic
template <typename T>
static void kernel_model(const std::vector<std::vector<int>>& masks, int h, int w, int oh, int ow, int misalign) {
  using namespace deva_rle;
  const int n = (int)masks.size();
  constexpr int E = 16 / (int)sizeof(T), kPieces = kTile / E + 1;
  const std::vector<int32_t> words = run_array(masks);
  const int32_t* first = words.data();
  const int32_t* starts = words.data() + n + 1;
  struct deva_rle_plan plan;
  if (deva_rle_plan(n, h, w, oh, ow, sizeof(T) == 4, &plan)) return fail("model plan", h, w, oh, ow);
  // the loop decoder: D1 pixel by pixel, D3 with the same fp32 scale
  std::vector<uint8_t> want((size_t)n * oh * ow);
  for (int k = 0; k < n; ++k) {
    std::vector<uint8_t> flat;
    for (size_t r = 0; r < masks[k].size(); ++r) flat.insert(flat.end(), masks[k][r], (uint8_t)(r & 1));
    for (int y = 0; y < oh; ++y)
      for (int x = 0; x < ow; ++x)
        want[((size_t)k * oh + y) * ow + x] = flat[(size_t)source_index(x, plan.scale_x, w) * h + source_index(y, plan.scale_y, h)];
  }
  // an output of exactly its size that begins `misalign` elements above a 16-byte boundary (the block itself is aligned)
  const size_t elements = (size_t)n * oh * ow;
  T* block = static_cast<T*>(aligned_alloc(16, (elements + misalign) * sizeof(T) + 16 - ((elements + misalign) * sizeof(T)) % 16));
  T* out = block + misalign;
  for (int i = 0; i < misalign; ++i) block[i] = (T)7;
  std::vector<int> written(elements, 0);
  const uint32_t out_low = (uint32_t)reinterpret_cast<uintptr_t>(out);
  std::vector<uint8_t> tile(kTile * kPitch);
  for (int64_t t = 0; t < (int64_t)n * plan.tiles_x * plan.tiles_y; ++t) {
    const int per_plane = plan.tiles_x * plan.tiles_y, k = (int)(t / per_plane), in_plane = (int)(t % per_plane);
    const int y0 = in_plane / plan.tiles_x * kTile, x0 = in_plane % plan.tiles_x * kTile;
    const int th = oh - y0 < kTile ? oh - y0 : kTile, tw = ow - x0 < kTile ? ow - x0 : kTile;
    const int64_t plane = (int64_t)k * oh * ow;
    std::fill(tile.begin(), tile.end(), (uint8_t)0xA5);
    for (int tid = 0; tid < kBlock; ++tid) {   // the walk
      const int col = tid % kTile, seg = tid / kTile, r0 = seg * kSegRows, r1 = r0 + kSegRows < th ? r0 + kSegRows : th;
      if (!(col < tw && r0 < r1)) continue;
      const int32_t* s = starts + first[k];
      const int runs_k = first[k + 1] - first[k] - 1;
      const int column = source_index(x0 + col, plan.scale_x, w) * h;
      int p = column + source_index(y0 + r0, plan.scale_y, h);
      int run = owner(s, runs_k, p), next = s[run + 1];
      for (int r = r0; r < r1; ++r) {
        p = column + source_index(y0 + r, plan.scale_y, h);
        run = advance(s, run, next, p);
        const int shift = row_shift(out_low, (uint32_t)plane + (uint32_t)(y0 + r) * (uint32_t)ow + (uint32_t)x0, sizeof(T));
        tile.at(r * kPitch + shift + col) = (uint8_t)(run & 1);
      }
    }
    for (int item = 0; item < th * kPieces; ++item) {   // the store
      const int r = item / kPieces, u0 = item % kPieces * E;
      const int shift = row_shift(out_low, (uint32_t)plane + (uint32_t)(y0 + r) * (uint32_t)ow + (uint32_t)x0, sizeof(T));
      const int64_t row = plane + (int64_t)(y0 + r) * ow + x0;
      int c0;
      const bool whole = whole_piece(u0, shift, tw, E, c0);
      if (whole && reinterpret_cast<uintptr_t>(out + row + c0) % 16 != 0) fail("a whole piece is not aligned", r, u0, shift, misalign);
      for (int e = 0; e < E; ++e)
        if (whole || (c0 + e >= 0 && c0 + e < tw)) {
          out[row + c0 + e] = (T)tile.at(r * kPitch + u0 + e);
          ++written[row + c0 + e];
        }
    }
  }
  long bad = 0;
  for (size_t i = 0; i < elements; ++i) bad += written[i] != 1 || out[i] != (T)want[i];
  for (int i = 0; i < misalign; ++i) bad += block[i] != (T)7;
  ++g_calls;
  if (bad) fail("the model differs from the loop decoder", h, w, oh * 100000 + ow, misalign);
  free(block);
}

static void model_cases() {
  const int sizes[][4] = {{1, 1, 1, 1}, {1, 9, 1, 9}, {9, 1, 9, 1}, {2, 2, 2, 2}, {7, 5, 70, 130}, {33, 67, 33, 67}, {33, 67, 66, 134},
                          {65, 129, 48, 95}, {64, 64, 64, 64}, {65, 129, 65, 129}, {3, 200, 5, 131}, {200, 3, 131, 5}};
  for (const auto& s : sizes) {
    const int h = s[0], w = s[1];
    std::vector<std::vector<int>> masks = {{h * w}, {0, h * w}, std::vector<int>(h * w, 1), std::vector<int>(w, h),
                                           {0, h * w / 2, 0, 0, h * w - h * w / 2, 0}};
    for (int k = 0; k < 3; ++k) masks.push_back(random_counts(h * w));
    for (int misalign = 0; misalign < 16; ++misalign) kernel_model<uint8_t>(masks, h, w, s[2], s[3], misalign);
    for (int misalign = 0; misalign < 4; ++misalign) kernel_model<float>(masks, h, w, s[2], s[3], misalign);
  }
}

int main() {
  plan_cases();
  d2_cases();
  model_cases();
  printf("%ld checks, %ld refused, %ld failures\n", g_calls, g_refused, g_failed);
  return g_failed ? 1 : 0;
}
