// Host side of the run-length encoder (mask_runs.hip): every argument check of deva_runs_count and deva_runs_write, the
// scratch layout and the launch decision that deva_runs_plan exposes.  No HIP in here: mask_runs_plan.cpp builds with
// the host compiler alone (tests/mask_runs_plan_sanitize_main.cpp runs it under the host sanitizers).
#pragma once
#include <stdint.h>

#include "../host_args.h"
#include "deva_mask_runs.h"

namespace deva_runs {
using namespace host_args;

constexpr int kTile = DEVA_RUNS_TILE;            // pixels a workgroup owns, each way; rows of a segment
constexpr int kBlock = 256;                      // lanes of a workgroup: 4 waves
constexpr int kScanItems = DEVA_RUNS_SCAN_CHUNK / kBlock;   // segments a lane scans in one step
constexpr int kMaxGrid = 65536;                  // workgroups of a launch; more work is walked in a grid-stride loop
constexpr int64_t kMaxPixels = (1ll << 31) - 1;
constexpr int kSegmentBytes = 12;                // E6: an int32 offset and a 64-bit word as two int32

void set_error(const char* fmt, ...);  // mask_runs_plan.cpp; text behind deva_runs_last_error()
const char* last_error();

#define DEVA_RUNS_REQUIRE(cond, ...) HOST_ARGS_REQUIRE(deva_runs::set_error, cond, __VA_ARGS__)

inline int element_bytes(int dtype) { return dtype == DEVA_RUNS_F32 ? 4 : 1; }

// the scratch of one call, in int32 words: off[n * segments], then bits[n * segments][2] (low word, high word)
struct Scratch {
  int32_t* off;
  uint32_t* bits;
};
inline Scratch carve(void* scratch, int n, const struct deva_runs_plan& plan) {
  int32_t* words = static_cast<int32_t*>(scratch);
  return {words, reinterpret_cast<uint32_t*>(words + (int64_t)n * plan.segments)};
}

// the sizes alone (E6) -> 0 and *plan, or 2 with the text set
int runs_plan(const char* what, int n, int height, int width, struct deva_runs_plan* plan);

// every check of deva_runs_count, before any launch -> 0 and *plan, or 2 with the text set
int count_check(const void* planes, int dtype, int n, int height, int width, const void* scratch, int64_t scratch_bytes,
                const int32_t* n_out, const int64_t* base, const int64_t* total, const int64_t* first, const int32_t* stats,
                struct deva_runs_plan* plan);

// every check of deva_runs_write, before any launch -> 0 and *plan, or 2 with the text set
int write_check(int n, int height, int width, const void* scratch, int64_t scratch_bytes, const int64_t* base, const int32_t* bounds,
                int64_t capacity, struct deva_runs_plan* plan);

}  // namespace deva_runs
