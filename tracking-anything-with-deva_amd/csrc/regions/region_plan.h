// Host side of the region kernels (regions.hip): every argument check of deva_regions_label and deva_regions_clean,
// the scratch layout of a plane in flight and the launch decision that deva_regions_plan exposes.  No HIP in here:
// region_plan.cpp builds with the host compiler alone (tests/region_plan_sanitize_main.cpp runs it under the host
// sanitizers).
#pragma once
#include <stdint.h>

#include "../host_args.h"
#include "deva_regions.h"

namespace deva_regions {
using namespace host_args;

constexpr int kTile = DEVA_REGIONS_TILE;
constexpr int kBlock = 256;      // lanes of a workgroup: 4 waves
constexpr int kWave = 64;
constexpr int kMaxGrid = 65536;  // workgroups of a launch: 256 per CU; more work is walked in a grid-stride loop
constexpr int64_t kMaxPixels = 1ll << 30;
constexpr int kStateWords = 16;  // the decision words of a plane (regions.hip: State)

void set_error(const char* fmt, ...);  // region_plan.cpp; text behind deva_regions_last_error()
const char* last_error();

#define DEVA_REGIONS_REQUIRE(cond, ...) HOST_ARGS_REQUIRE(deva_regions::set_error, cond, __VA_ARGS__)

// where the pieces of one plane in flight lie in its plane_bytes of scratch
struct PlaneLayout {
  int64_t labels, areas, state, bytes;
};
PlaneLayout plane_layout(int64_t pixels);

// the sizes alone -> 0 and *plan, or 2 with the text set.  budget_bytes < 0: no budget (one pass)
int region_plan(const char* what, int height, int width, int n, int64_t budget_bytes, struct deva_regions_plan* plan);

// every check of the two entry points, before any launch -> 0 and *plan, or 2 with the text set
int label_check(const void* planes, int n, int height, int width, const void* labels, struct deva_regions_plan* plan);
int clean_check(const void* planes, int n, int height, int width, int min_area, const void* records, const void* scratch,
                int64_t scratch_bytes, struct deva_regions_plan* plan);

}  // namespace deva_regions
