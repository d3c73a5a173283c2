// Host side of the proposal filter (proposals.hip): argument checks and the layout of its scratch memory.  No HIP in
// here (proposal_plan.cpp builds with the host compiler alone, as detection_plan.cpp does).
#pragma once
#include <stdint.h>

#include "host_args.h"

namespace deva {

constexpr int kPropMaxMasks = 4096;   // stored masks per frame: kDetMaxMasks, and 64 lanes x one 64-bit suppression word
constexpr int kPropBatch = 1024;      // masks of one decide launch (one thread each); a longer batch is cut into these
constexpr int kPropChunk = 16384;     // elements of one plane that one workgroup of the stats / binarise / gather pass takes
constexpr int kPropStat = 8;          // int32 per mask in the batch records: hi, lo, x_min, i_min, x_max, i_max, 2 unused
constexpr int kPropRow = 8;           // int32 per stored mask in the frame's table and in the result (include/deva_hip.h)
constexpr int kPropHeader = 4;        // int32 in front of the result rows: stored, passed, kept, 0
constexpr int64_t kPropMaxPixels = 1ll << 30;

struct ProposalPlan {
  int words;  // 64-bit words of one row of the suppression matrix
  // byte offsets into the scratch, each a multiple of 256
  int64_t off_stats;   // [kPropBatch][kPropStat] int32
  int64_t off_slots;   // [kPropBatch] int32: arena slot of each mask of the batch, -1 without one
  int64_t off_count;   // [4] int32: masks that passed so far this frame (stored = min(passed, capacity)), 3 unused
  int64_t off_table;   // [capacity][kPropRow] int32 in arrival order
  int64_t off_order;   // [capacity] int32: position in the NMS order -> index
  int64_t off_keep;    // [capacity] int32: the kept indices in that order
  int64_t off_nkeep;   // [4] int32: their number, 3 unused
  int64_t off_matrix;  // [capacity][words] uint64: bit c of row r = the box at position c > r overlaps the one at r
  int64_t bytes;
};

// the layout for 1 <= capacity <= kPropMaxMasks.  Defined here with internal linkage: libdeva_lowres.so (lowres/) works on the
// same scratch and compiles the same text, and no library exports or shares a symbol for it.
static inline ProposalPlan proposal_plan(int capacity) {
  ProposalPlan p;
  p.words = (capacity + 63) / 64;
  host_args::ScratchLayout s;
  p.off_stats = s.take((int64_t)kPropBatch * kPropStat * 4);
  p.off_slots = s.take((int64_t)kPropBatch * 4);
  p.off_count = s.take(256);
  p.off_table = s.take((int64_t)capacity * kPropRow * 4);
  p.off_order = s.take((int64_t)capacity * 4);
  p.off_keep = s.take((int64_t)capacity * 4);
  p.off_nkeep = s.take(256);
  p.off_matrix = s.take((int64_t)capacity * p.words * 8);
  p.bytes = s.at;
  return p;
}
bool proposal_capacity_ok(int capacity);
// workgroups per plane of the chunked passes: the plane's elements plus the up to 15 that align its first group
int proposal_chunks(int height, int width);

// every check of the entry points, before any launch -> 0, or 2 with the text set
int proposal_begin_check(int capacity, const void* scratch, int64_t scratch_bytes);
int proposal_batch_check(const void* logits, const void* iou_preds, int batch, int height, int width, double pred_iou_thresh,
                         double stability_score_thresh, double stability_score_offset, double mask_threshold,
                         const void* arena, int capacity, const void* scratch, int64_t scratch_bytes);
int proposal_finish_check(int capacity, double box_nms_thresh, const void* scratch, int64_t scratch_bytes, const void* result);
int proposal_gather_check(const void* arena, int capacity, int height, int width, const void* scratch, int64_t scratch_bytes,
                          int n_kept, const void* out);
int box_nms_check(const void* boxes, const void* scores, int m, double box_nms_thresh, const void* scratch,
                  int64_t scratch_bytes, const void* keep, const void* n_keep);

// the rank / matrix / reduce launches of rule 5 on checked arguments (proposals.hip; shared with box_prompts.hip):
// boxes int32 [n][4], or fp32 [n][4] taken as given with boxes_f32; `what` names the entry point in an error
int box_nms_run(const char* what, const void* boxes, bool boxes_f32, const float* scores, int n_boxes, double thresh,
                void* scratch, int32_t* keep, int32_t* n_keep, void* stream);

}  // namespace deva
