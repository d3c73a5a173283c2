// Host side of the run-length text codec (rle_text.hip): every argument check of deva_text_encode_count,
// deva_text_encode_write and deva_text_parse, the scratch layout and the launch decision that deva_text_plan exposes.
// No HIP in here: rle_text_plan.cpp builds with the host compiler alone (tests/rle_text_plan_sanitize_main.cpp runs it
// under the host sanitizers).
#pragma once
#include <stdint.h>

#include "../host_args.h"
#include "deva_rle_text.h"

namespace deva_text {
using namespace host_args;

constexpr int kBlock = 256;                                  // lanes of a workgroup: 4 waves
constexpr int kItems = DEVA_TEXT_SCAN_CHUNK / kBlock;        // counts or characters a lane takes in one step
constexpr int64_t kMaxPixels = (1ll << 31) - 1;
constexpr int64_t kMaxText = (1ll << 31) - 1;                // C8: L < 2^31
constexpr int kMaskScratchBytes = 8;                         // the parser's: an int32 value count and an int32 of flags

void set_error(const char* fmt, ...);  // rle_text_plan.cpp; text behind deva_text_last_error()
const char* last_error();

#define DEVA_TEXT_REQUIRE(cond, ...) HOST_ARGS_REQUIRE(deva_text::set_error, cond, __VA_ARGS__)

// C1 on the host: the characters of the canonical coding of x (1 .. 13)
inline int value_chars(int64_t x) {
  for (int width = 1;; ++width) {
    const int c = (int)(x & 0x1f);
    x >>= 5;
    if ((c & 0x10) ? x == -1 : x == 0) return width;
  }
}

// the parser's scratch of one call, in int32 words: values[n], then flags[n]
struct Scratch {
  int32_t* values;
  int32_t* flags;
};
inline Scratch carve(void* scratch, int n) {
  int32_t* words = static_cast<int32_t*>(scratch);
  return {words, words + n};
}

// the sizes alone (C8) -> 0 and *plan, or 2 with the text set
int text_plan(const char* what, int n, int height, int width, int64_t chars, struct deva_text_plan* plan);

// every check of deva_text_encode_count, before any launch -> 0 and *plan, or 2 with the text set
int count_check(const int32_t* n_in, const int64_t* base, const int32_t* bounds, int64_t bounds_len, int n, int height, int width,
                const int32_t* text_len, const int64_t* text_base, const int64_t* text_total, const int64_t* first,
                struct deva_text_plan* plan);

// every check of deva_text_encode_write
int write_check(const int32_t* n_in, const int64_t* base, const int32_t* bounds, int64_t bounds_len, int n, int height, int width,
                const int64_t* text_base, const uint8_t* chars, int64_t capacity, struct deva_text_plan* plan);

// every check of deva_text_parse
int parse_check(const uint8_t* chars, int64_t chars_len, const int64_t* text_first, int n, int height, int width, const void* scratch,
                int64_t scratch_bytes, const int32_t* runs, int64_t words_cap, const int64_t* info, struct deva_text_plan* plan);

}  // namespace deva_text
