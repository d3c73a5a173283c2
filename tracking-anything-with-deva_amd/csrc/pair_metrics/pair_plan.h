// Host side of the pair counts (pair_counts.hip): every argument check of deva_pair_counts and the launch decision
// that deva_pair_plan exposes.  No HIP in here: pair_plan.cpp builds with the host compiler alone
// (tests/pair_plan_sanitize_main.cpp runs it under the host sanitizers).
#pragma once
#include <stdint.h>

#include "../host_args.h"
#include "deva_pair_metrics.h"

namespace deva_pair {
using namespace host_args;

constexpr int kBlock = 256;     // lanes of a workgroup: 4 waves
constexpr int kWave = 64;
constexpr int kMaxGrid = 2048;  // workgroups of a launch: 8 per CU; a larger plane is walked in a grid-stride loop
constexpr int kMaxMatchGrid = 1024;  // of the disk search: 4 per CU (at 64 x 64 slots five tables of 33 KB fit a CU's LDS)
constexpr int64_t kMaxPixels = 1ll << 30;
constexpr int kWordBytes = 16;  // the two boundary words of a pixel, side by side

void set_error(const char* fmt, ...);  // pair_plan.cpp; text behind deva_pair_last_error()
const char* last_error();

#define DEVA_PAIR_REQUIRE(cond, ...) HOST_ARGS_REQUIRE(deva_pair::set_error, cond, __VA_ARGS__)

// bytes of one pixel of a plane, 0 for an unknown encoding
int encoding_bytes(int encoding);

// the sizes alone -> 0 and *plan, or 2 with the text set
int pair_plan(const char* what, int height, int width, int n_gt, int n_pred, int radius, struct deva_pair_plan* plan);

// every check of deva_pair_counts, before any launch -> 0 and *plan, or 2 with the text set
int pair_counts_check(const void* gt, int gt_encoding, const void* gt_ids, int n_gt, const void* pred, int pred_encoding,
                      const void* pred_ids, int n_pred, const void* pred_lut, int channels, int height, int width, int radius,
                      const void* scratch, int64_t scratch_bytes, const void* singles, const void* pairs,
                      struct deva_pair_plan* plan);

}  // namespace deva_pair
