// Host side of the joint count (panoptic_counts.hip): every argument check of deva_metrics_panoptic_counts and the
// launch decision that deva_metrics_panoptic_plan exposes.  No HIP in here: panoptic_plan.cpp builds with the host
// compiler alone (tests/panoptic_plan_sanitize_main.cpp runs it under the host sanitizers).
#pragma once
#include <stdint.h>

#include "../host_args.h"
#include "deva_metrics.h"

namespace deva_metrics {
using namespace host_args;

constexpr int kBlock = 256;            // lanes of a workgroup
constexpr int kMaxGrid = 2048;         // workgroups of a launch: 8 per CU; a larger plane is walked in a grid-stride loop
constexpr int64_t kMaxPixels = 1ll << 30;

void set_error(const char* fmt, ...);  // panoptic_plan.cpp; text behind deva_metrics_last_error()
const char* last_error();

#define DEVA_METRICS_REQUIRE(cond, ...) HOST_ARGS_REQUIRE(deva_metrics::set_error, cond, __VA_ARGS__)

// bytes of one pixel of a plane, 0 for an unknown encoding
int encoding_bytes(int encoding);

// the sizes alone -> 0 and *plan, or 2 with the text set
int panoptic_plan(const char* what, int height, int width, int n_gt, int n_pred, deva_metrics_plan* plan);

// every check of deva_metrics_panoptic_counts, before any launch -> 0 and *plan, or 2 with the text set
int panoptic_counts_check(const void* gt, int gt_encoding, const void* gt_ids, int n_gt, const void* pred, int pred_encoding,
                          const void* pred_ids, int n_pred, const void* pred_lut, int channels, int height, int width,
                          const void* counts, deva_metrics_plan* plan);

}  // namespace deva_metrics
