// Host side of the low-resolution filter (lowres.hip): every argument check of its three launching entry points (rule
// L7 of include/deva_lowres.h), the launch decision that deva_lowres_plan exposes, and the host half of rule L1.  No
// HIP in here: lowres_plan.cpp builds with the host compiler alone (tests/lowres_plan_sanitize_main.cpp runs it under
// the host sanitizers).  The scratch is the proposal filter's: ../proposal_plan.h, compiled here as there.
#pragma once
#include <stdint.h>

#include "../host_args.h"
#include "../proposal_plan.h"
#include "deva_lowres.h"

namespace deva_lowres {
using namespace host_args;

constexpr int kBlock = 256;          // lanes of a workgroup: 4 waves
constexpr int kPiece = 16;           // bytes of one store of the byte passes; pixels a lane takes in one step
constexpr int kBandPixels = 16384;   // output pixels of a band at most (a band is at least one row)
constexpr int kMaxGridY = 65535;
constexpr int kMidPerOutMax = 3;     // tile path only while a band forms at most this many values of `mid` per output pixel
constexpr int64_t kMaxPlanes = 1ll << 30;

void set_error(const char* fmt, ...);  // lowres_plan.cpp; text behind deva_lowres_last_error()
const char* last_error();

#define DEVA_LOWRES_REQUIRE(cond, ...) HOST_ARGS_REQUIRE(deva_lowres::set_error, cond, __VA_ARGS__)

// L1's scale: one rounded fp32 division
inline float axis_scale(int n_in, int n_out) { return (float)n_in / (float)n_out; }

// rows of the source that `cover` consecutive destination rows of a resize n_in -> n_out can touch, at most: the source
// index of L1 is monotone in d and advances by the scale per row (up to its rounding), i0 and i1 add one row, and one
// more stands for the roundings
inline int rows_touched(int cover, int n_in, int n_out) {
  const double span = (double)cover * (double)n_in / (double)n_out;
  const int64_t rows = (int64_t)span + 1 + 3;
  return rows < n_in ? (int)rows : n_in;
}

// L7 on the geometry alone -> 0, or 2 with the text set
int geometry_check(const char* what, const struct deva_lowres_geometry* g);
// the launch decision (after geometry_check) -> 0 and *plan, or 2 with the text set
int lowres_plan(const char* what, const struct deva_lowres_geometry* g, struct deva_lowres_plan* plan);

// every check of the entry points, before any launch -> 0 and *plan, or 2 with the text set
int upsample_check(const void* low, int batch, const struct deva_lowres_geometry* g, const void* out, struct deva_lowres_plan* plan);
int select_check(const void* low, const void* scores, int batch, int per_box, const struct deva_lowres_geometry* g,
                 double mask_threshold, const void* out, const void* chosen, struct deva_lowres_plan* plan);
int proposal_check(const void* low, const void* iou_preds, int batch, const struct deva_lowres_geometry* g, double pred_iou_thresh,
                   double stability_score_thresh, double stability_score_offset, double mask_threshold, const void* arena,
                   int capacity, const void* scratch, int64_t scratch_bytes, struct deva_lowres_plan* plan);

}  // namespace deva_lowres
