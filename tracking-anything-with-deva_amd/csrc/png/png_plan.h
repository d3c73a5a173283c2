// Host side of the PNG deflate coder (png_encode.hip): every argument check of deva_png_deflate and deva_png_place, the
// segment geometry, the scratch layout and the capacity sizes that deva_png_plan exposes.  No HIP in here:
// png_plan.cpp builds with the host compiler alone (tests/png_plan_sanitize_main.cpp runs it under the host sanitizers).
#pragma once
#include <stdint.h>

#include "../host_args.h"
#include "deva_png.h"

namespace deva_png {
using namespace host_args;

constexpr int kBlock = 256;                       // lanes of a workgroup: 4 waves
constexpr int kItems = DEVA_PNG_STEP / kBlock;    // bytes of a row string a lane takes in one step
constexpr int kBufferBytes = 4096;                // the bit buffer of a workgroup in LDS (see png_encode.hip for the bound)
constexpr int kStageBytes = DEVA_PNG_STEP + 48;   // one staged window of a row: the step's bytes, two before, one behind, alignment
constexpr int kLdsBytes = kBufferBytes + 2 * kStageBytes + 128;

void set_error(const char* fmt, ...);  // png_plan.cpp; text behind deva_png_last_error()
const char* last_error();

#define DEVA_PNG_REQUIRE(cond, ...) HOST_ARGS_REQUIRE(deva_png::set_error, cond, __VA_ARGS__)

// Z5 / Z7: the bytes of a segment of `rows` rows at most: block header, every byte a 9-bit literal, end-of-block, the
// stored block's three bits, the padding to a byte, 00 00 FF FF
inline int64_t segment_worst(int64_t rows, int64_t row_bytes) { return (3 + 9 * rows * (row_bytes + 1) + 7 + 3 + 7) / 8 + 4; }

// the scratch of one call, front to back, every piece on a 256-byte boundary
struct Scratch {
  int64_t* sizes;     // [segments] bytes of every segment
  uint32_t* sums;     // [2 * segments] the Adler sums of every segment, each below 65521
  int64_t* offsets;   // [segments] where every segment begins in the stream
  uint8_t* slots;     // [segments][slot_bytes]
};
inline int64_t scratch_layout(int segments, int64_t slot_bytes, int64_t (&at)[4]) {
  ScratchLayout lay;
  at[0] = lay.take(8ll * segments);
  at[1] = lay.take(8ll * segments);
  at[2] = lay.take(8ll * segments);
  at[3] = lay.take(slot_bytes * segments);
  return lay.at;
}
inline Scratch carve(void* scratch, const struct deva_png_plan& plan) {
  int64_t at[4];
  scratch_layout(plan.segments, plan.slot_bytes, at);
  uint8_t* base = static_cast<uint8_t*>(scratch);
  return {reinterpret_cast<int64_t*>(base + at[0]), reinterpret_cast<uint32_t*>(base + at[1]), reinterpret_cast<int64_t*>(base + at[2]),
          base + at[3]};
}

// the sizes alone (Z1) -> 0 and *plan, or 2 with the text set
int png_plan(const char* what, int height, int width, int bpp, struct deva_png_plan* plan);

// every check of deva_png_place, before any launch -> 0 and *plan, or 2 with the text set
int place_check(const char* what, int height, int width, int bpp, const void* scratch, int64_t scratch_bytes, const uint8_t* out,
                int64_t capacity, const int64_t* info, struct deva_png_plan* plan);

// every check of deva_png_deflate
int deflate_check(const uint8_t* plane, int height, int width, int bpp, const void* scratch, int64_t scratch_bytes, const uint8_t* out,
                  int64_t capacity, const int64_t* info, struct deva_png_plan* plan);

}  // namespace deva_png
