// Host side of the run-length overlap (rle_overlap.hip): every argument check of deva_overlap_intersections, rule O2 on
// the run arrays and the launch decision that deva_overlap_plan exposes.  No HIP in here: rle_overlap_plan.cpp builds
// with the host compiler alone (tests/rle_overlap_plan_sanitize_main.cpp runs it under the host sanitizers).
#pragma once
#include <stdint.h>

#include "../host_args.h"
#include "deva_rle_overlap.h"

namespace deva_overlap {
using namespace host_args;

constexpr int kBlock = 256;                      // lanes of a workgroup: 4 waves
constexpr int kChunkD = DEVA_OVERLAP_D_CHUNK;    // detections a workgroup of the pair pass owns
constexpr int kLdsRuns = DEVA_OVERLAP_LDS_RUNS;  // runs of a g that is held in LDS
constexpr int kScanItems = DEVA_OVERLAP_SCAN_CHUNK / kBlock;   // starts a lane scans in one step
constexpr int kMaxGrid = 65536;                  // workgroups of a launch; more work is walked in a grid-stride loop
constexpr int64_t kMaxPixels = (1ll << 31) - 1;
// LDS of the pair pass: g's starts and ones_before, the chunk's counters and box flags
constexpr int kLdsBytes = 2 * (kLdsRuns + 1) * 4 + 2 * kChunkD * 4;

void set_error(const char* fmt, ...);  // rle_overlap_plan.cpp; text behind deva_overlap_last_error()
const char* last_error();

#define DEVA_OVERLAP_REQUIRE(cond, ...) HOST_ARGS_REQUIRE(deva_overlap::set_error, cond, __VA_ARGS__)

inline const char* side_name(int side) { return side == DEVA_OVERLAP_GT ? "gt" : "dt"; }

// the sizes alone -> 0 and *plan, or 2 with the text set
int pair_plan(const char* what, int d, int g, int64_t words_g, struct deva_overlap_plan* plan);

// O2 on one side's run array (host memory) -> 0, or 2 with the text set, which names the side and the mask
int runs_check(const char* what, int side, const int32_t* runs, int64_t words, int n, int height, int width);

// every check of deva_overlap_intersections, before any launch -> 0 and *plan, or 2 with the text set
int intersections_check(const int32_t* dt_host, const int32_t* dt_device, int64_t dt_words, int d, const int32_t* gt_host,
                        const int32_t* gt_device, int64_t gt_words, int g, int height, int width, const int32_t* box_d,
                        const int32_t* box_g, const void* scratch, int64_t scratch_bytes, const uint32_t* inter, int64_t pitch,
                        const uint32_t* area_d, const uint32_t* area_g, struct deva_overlap_plan* plan);

}  // namespace deva_overlap
