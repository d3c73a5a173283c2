// Host side of deva_detection_assemble (detections.hip): argument checks and the layout of its scratch memory.  No HIP
// in here (detection_plan.cpp builds with the host compiler alone, as conv_plan.cpp does).
#pragma once
#include <stdint.h>

namespace deva {

constexpr int kDetMaxMasks = 4096;       // one LDS counter pair per mask and the background: 32 KiB
constexpr int kDetChunk = 16384;         // pixels of one mask that one workgroup of the area pass sums
constexpr int kDetRecord = 8;            // int32 per mask in the record table (include/deva_hip.h)
enum { DET_SUPPRESS_SMALL = 0, DET_PREFER_SMALL = 1, DET_TEXT = 2 };

struct DetectionPlan {
  int chunks;  // area-pass workgroups per mask
  // byte offsets into the scratch, each a multiple of 256
  int64_t off_part_area, off_part_orig, off_part_src;  // [n][chunks] float / int32 / int32
  int64_t off_area, off_orig, off_src, off_mult;       // [n] float / int32 / int32 / float
  int64_t off_stats;                                   // [n + 1][2] int32: mask_area, both (entry 0: the background)
  int64_t off_lut;                                     // [n + 1] int32: plane value -> id
  int64_t off_plane;                                   // [oh][ow] uint16: hard index | (P_hard >= 0.5) << 15
  int64_t bytes;
};

// the layout for n >= 1 masks; sizes must already have passed detection_sizes_ok
DetectionPlan detection_plan(int n, int h0, int w0, int oh, int ow);
bool detection_sizes_ok(int n, int h0, int w0, int oh, int ow);

// every check of deva_detection_assemble, before any launch -> 0, or 2 with the text set
int detection_check(const void* masks, int n, int h0, int w0, int oh, int ow, int policy, double overlap_threshold,
                    const void* scratch, int64_t scratch_bytes, const void* out, const void* records);

}  // namespace deva
