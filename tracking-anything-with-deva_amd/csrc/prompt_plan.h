// Host side of the prompt-point choice (prompts.hip): argument checks and the layout of its scratch memory.  No HIP in
// here (prompt_plan.cpp builds with the host compiler alone, as proposal_plan.cpp does).
#pragma once
#include <stdint.h>

namespace deva {

constexpr int kPromptScale = 16;          // the low-resolution map is [H/16, W/16]; filter scale and support, both axes
constexpr int kPromptTaps = 32;           // taps of an unclipped window: positions 16 o - 8 ... 16 o + 23
constexpr int kPromptMaxPoints = 16384;   // points of one call: one workgroup of 1024 threads, 16 rounds
constexpr int kPromptMaxSide = 65536;
constexpr int64_t kPromptMaxPixels = 1ll << 30;
constexpr int kPromptTileX = 64;          // outputs per row of one workgroup of the horizontal pass (one wave)
constexpr int kPromptTileRows = 4;        // rows of that workgroup (one wave each)

struct PromptPlan {
  int low_h, low_w;  // H / 16, W / 16
  // byte offsets into the scratch, each a multiple of 256
  int64_t off_rows;  // [H][low_w] fp32: the horizontal pass
  int64_t off_low;   // [low_h][low_w] fp32: the map that is sampled
  int64_t bytes;
};

// height, width in [16, kPromptMaxSide] and at most kPromptMaxPixels pixels
bool prompt_size_ok(int height, int width);
bool prompt_points_ok(int points);
// the layout for a size and a number of points that are ok
PromptPlan prompt_plan(int height, int width);

// every check of deva_prompt_points, before any launch -> 0, or 2 with the text set
int prompt_points_check(const void* mask, int mask_elem_bytes, int height, int width, const void* points_xy, int points,
                        double threshold, const void* scratch, int64_t scratch_bytes, const void* out_points,
                        const void* out_labels, const void* out_count);

}  // namespace deva
