// Box prompts of a text-prompted detection frame: the detector's fp32 boxes through box NMS, and the best of a
// segmenter's candidate masks per box as a byte plane (the reference: deva/ext/grounding_dino.py:101-115, torchvision's
// nms on the host, then per box sam.predict, np.argmax(scores) and a numpy mask; contract: include/deva_hip.h,
// deva_box_nms_xyxy and deva_box_mask_select).
//
//   nms       the rank / matrix / reduce launches of proposals.hip with the boxes loaded as fp32
//   select    grid (chunk, box): every workgroup derives the box's choice from its <= 16 scores (uniform loads), then
//             streams its chunk of the chosen plane: one 16-byte load and one 4-byte store per group of four pixels.
//             4 bytes read and 1 written per pixel and box; the planes that are not chosen are never touched.
#include "box_choice.h"  // box_choice
#include "box_prompt_plan.h"
#include "common.h"
#include "proposal_plan.h"

namespace deva {
namespace {

struct BoxSelectArgs {
  const float* logits;  // plane 0 of box 0 of this launch
  const float* scores;  // its first score
  int per_box, hw;
  float t_mask;
  uint8_t* out;      // plane of box 0 of this launch
  int32_t* chosen;   // its choice, or NULL
};

// The chosen plane is walked in the aligned space of prop_stats_kernel (proposals.hip): element e sits at the 16-byte
// boundary below the plane plus 4 e bytes, the plane is e in [shift, shift + hw), a group of four with e % 4 == 0 is one
// aligned 16-byte load.  Pixel i = e - shift goes to out + i; whether the four bytes of a group form an aligned word
// there is the same for every group of a plane.
__global__ void __launch_bounds__(256) box_select_kernel(BoxSelectArgs a) {
  const int b = blockIdx.y, t = threadIdx.x;
  const int pick = box_choice(a.scores + (int64_t)b * a.per_box, a.per_box);
  if (a.chosen && blockIdx.x == 0 && t == 0) a.chosen[b] = pick;
  const float* p = a.logits + ((int64_t)b * a.per_box + pick) * a.hw;
  uint8_t* o = a.out + (int64_t)b * a.hw;
  const int shift = (int)(reinterpret_cast<uintptr_t>(p) >> 2 & 3);
  const bool words = ((reinterpret_cast<uintptr_t>(o) - (uintptr_t)shift) & 3) == 0;
  const int e_first = blockIdx.x * kBoxChunk, e_end = shift + a.hw;
  const float* base = p - shift;  // (16-byte aligned; nothing below the plane is read)
  const float tm = a.t_mask;
#pragma unroll 4
  for (int it = 0; it < kBoxChunk / 1024; ++it) {
    const int e0 = e_first + it * 1024 + 4 * t;
    if (e0 >= e_end) break;
    const int i = e0 - shift;
    if (e0 >= shift && e0 + 4 <= e_end) {
      const float4 v = *reinterpret_cast<const float4*>(base + e0);
      const uint32_t word = (uint32_t)(v.x > tm) | (uint32_t)(v.y > tm) << 8 | (uint32_t)(v.z > tm) << 16 | (uint32_t)(v.w > tm) << 24;
      if (words) {
        *reinterpret_cast<uint32_t*>(o + i) = word;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) o[i + j] = (uint8_t)(word >> (8 * j));
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (e0 + j >= shift && e0 + j < e_end) o[i + j] = base[e0 + j] > tm;
    }
  }
}

}  // namespace
}  // namespace deva

using namespace deva;

extern "C" int deva_box_nms_xyxy(const float* boxes, const float* scores, int n_boxes, double thresh, void* scratch,
                                 int64_t scratch_bytes, int32_t* keep, int32_t* n_keep, void* stream) {
  if (int e = box_nms_xyxy_check(boxes, scores, n_boxes, thresh, scratch, scratch_bytes, keep, n_keep)) return e;
  return box_nms_run("deva_box_nms_xyxy", boxes, true, scores, n_boxes, thresh, scratch, keep, n_keep, stream);
}

extern "C" int deva_box_mask_select(const float* logits, const float* scores, int batch, int per_box, int height, int width,
                                    double mask_threshold, uint8_t* out, int32_t* chosen, void* stream) {
  if (int e = box_mask_select_check(logits, scores, batch, per_box, height, width, mask_threshold, out, chosen)) return e;
  if (batch == 0) return 0;
  BoxSelectArgs a = {};
  a.per_box = per_box, a.hw = height * width;
  a.t_mask = (float)mask_threshold;
  const unsigned chunks = (unsigned)box_select_chunks(height, width);
  for (int first = 0; first < batch; first += kBoxMaxGridY) {
    const int nb = batch - first < kBoxMaxGridY ? batch - first : kBoxMaxGridY;
    a.logits = logits + (int64_t)first * per_box * a.hw;
    a.scores = scores + (int64_t)first * per_box;
    a.out = out + (int64_t)first * a.hw;
    a.chosen = chosen ? chosen + first : nullptr;
    hipLaunchKernelGGL(box_select_kernel, dim3(chunks, (unsigned)nb), dim3(256), 0, (hipStream_t)stream, a);
  }
  return check_launch("deva_box_mask_select");
}
