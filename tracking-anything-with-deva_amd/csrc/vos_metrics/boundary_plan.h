// Host side of the DAVIS counts (boundary_counts.hip): the radius rule, every argument check of deva_vos_boundary_counts
// and the launch decision that deva_vos_boundary_plan exposes.  No HIP in here: boundary_plan.cpp builds with the host
// compiler alone (tests/vos_plan_sanitize_main.cpp runs it under the host sanitizers).
#pragma once
#include <stdint.h>

#include "../host_args.h"
#include "deva_vos_metrics.h"

namespace deva_vos {
using namespace host_args;

constexpr int kBlock = 256;     // lanes of a workgroup: 4 waves
constexpr int kWave = 64;
constexpr int kMaxGrid = 2048;  // workgroups of a launch: 8 per CU; a larger plane is walked in a grid-stride loop
constexpr int kMaxMatchGrid = 1024;  // of the disk search: 4 per CU, whose 16 waves are resident together at its register count
constexpr int64_t kMaxPixels = 1ll << 30;
constexpr int kWordBytes = 16;  // the two boundary words of a pixel, side by side

void set_error(const char* fmt, ...);  // boundary_plan.cpp; text behind deva_vos_last_error()
const char* last_error();

#define DEVA_VOS_REQUIRE(cond, ...) HOST_ARGS_REQUIRE(deva_vos::set_error, cond, __VA_ARGS__)

// bytes of one pixel of a plane (the BINARY flag is ignored), 0 for an unknown encoding
int encoding_bytes(int encoding);

// R3 -> 0 and *radius, or 2 with the text set
int boundary_radius(const char* what, int height, int width, double bound_th, int* radius);

// the sizes alone -> 0 and *plan, or 2 with the text set
int boundary_plan(const char* what, int height, int width, int n_objects, int radius, deva_vos_plan* plan);

// every check of deva_vos_boundary_counts, before any launch -> 0 and *plan, or 2 with the text set
int boundary_counts_check(const void* gt, int gt_encoding, const void* pred, int pred_encoding, const void* ids, int n_objects,
                          const void* pred_lut, int channels, int height, int width, int radius, const void* scratch,
                          int64_t scratch_bytes, const void* counts, deva_vos_plan* plan);

}  // namespace deva_vos
