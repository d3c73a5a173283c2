// Host side of the box prompts of a text-prompted detection frame (box_prompts.hip): the argument checks of
// deva_box_nms_xyxy and deva_box_mask_select and the launch geometry of the latter.  No HIP in here
// (box_prompt_plan.cpp builds with the host compiler alone, as proposal_plan.cpp does).
#pragma once
#include <stdint.h>

namespace deva {

constexpr int kBoxMaxPerBox = 16;       // candidate planes per box (a segmenter's multimask output has 3 or 4)
constexpr int kBoxChunk = 16384;        // elements of one plane that one workgroup of the select pass takes
constexpr int kBoxMaxGridY = 65535;     // boxes of one launch (grid.y); a longer batch is cut into these
constexpr int64_t kBoxMaxPixels = 1ll << 30;

// workgroups per plane: the plane's elements plus the up to 3 that align its first group of four floats
int box_select_chunks(int height, int width);

// every check of the entry points, before any launch -> 0, or 2 with the text set
int box_nms_xyxy_check(const void* boxes, const void* scores, int n_boxes, double thresh, const void* scratch,
                       int64_t scratch_bytes, const void* keep, const void* n_keep);
int box_mask_select_check(const void* logits, const void* scores, int batch, int per_box, int height, int width,
                          double mask_threshold, const void* out, const void* chosen);

}  // namespace deva
