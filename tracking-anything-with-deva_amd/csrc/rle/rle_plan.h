// Host side of the run-length decoder (rle_decode.hip): every argument check of deva_rle_decode, rule D2 on the run array
// and the launch decision that deva_rle_plan exposes.  No HIP in here: rle_plan.cpp builds with the host compiler alone
// (tests/rle_plan_sanitize_main.cpp runs it under the host sanitizers).
#pragma once
#include <stdint.h>

#include "../host_args.h"
#include "deva_rle.h"

namespace deva_rle {
using namespace host_args;

constexpr int kTile = DEVA_RLE_TILE;   // output pixels a workgroup owns, each way
constexpr int kBlock = 256;            // lanes of a workgroup: 4 waves
constexpr int kSegRows = kTile * kTile / kBlock;   // rows a lane walks: a column of the tile is shared by kBlock / kTile lanes
constexpr int kPitch = kTile + 16;     // bytes of a tile row in LDS: a row is shifted by up to 15 bytes (rle_decode.hip)
constexpr int kMaxGrid = 65536;        // workgroups of a launch; more tiles are walked in a grid-stride loop
constexpr int64_t kMaxPixels = (1ll << 31) - 1;

void set_error(const char* fmt, ...);  // rle_plan.cpp; text behind deva_rle_last_error()
const char* last_error();

#define DEVA_RLE_REQUIRE(cond, ...) HOST_ARGS_REQUIRE(deva_rle::set_error, cond, __VA_ARGS__)

inline int element_bytes(int dtype) { return dtype == DEVA_RLE_F32 ? 4 : 1; }

// the sizes alone -> 0 and *plan, or 2 with the text set
int decode_plan(const char* what, int n, int height, int width, int out_height, int out_width, int dtype, struct deva_rle_plan* plan);

// D2 on the run array (host memory) -> 0, or 2 with the text set, which names the mask
int runs_check(const char* what, const int32_t* runs, int64_t words, int n, int height, int width);

// every check of deva_rle_decode, before any launch -> 0 and *plan, or 2 with the text set
int decode_check(const int32_t* runs_host, const int32_t* runs_device, int64_t words, int n, int height, int width, int out_height,
                 int out_width, int dtype, const void* out, struct deva_rle_plan* plan);

}  // namespace deva_rle
