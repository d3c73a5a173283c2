// The per-pixel decision of the output tail, shared by deva_index_mask (merge.hip) and deva_frame_result
// (frame_result.hip): channel index of the first maximum of the probabilities resized to the output size.
//
// Bilinear arithmetic follows ATen's upsample_bilinear2d (align_corners=False): source coordinate
// scale*(dst+0.5)-0.5 clamped at 0, neighbour index clamped at the border, rows blended after columns.  The
// roundings are written out (one fused multiply-add for the coordinate; per row one rounded product and one fused
// multiply-add; the row blend two rounded products and an add -- the form deva_index_mask has always been compiled
// to, see also ensemble.hip) so that every translation unit that includes this file decides a near-tie the same way.
#pragma once
#include "common.h"

namespace deva {

__device__ __forceinline__ int resized_argmax(const float* __restrict__ prob, int channels, int h, int w, int oh,
                                              int ow, float scale_y, float scale_x, int y, int x) {
#pragma clang fp contract(off)
  const int64_t plane = (int64_t)h * w;
  int best = 0;
  if (oh == h && ow == w) {
    const int64_t i = (int64_t)y * ow + x;
    float bv = prob[i];
    for (int c = 1; c < channels; ++c) {
      const float v = prob[(int64_t)c * plane + i];
      if (v > bv) {
        bv = v;
        best = c;
      }
    }
  } else {
    const float sy = fmaxf(__builtin_fmaf(scale_y, (float)y + 0.5f, -0.5f), 0.0f);
    const float sx = fmaxf(__builtin_fmaf(scale_x, (float)x + 0.5f, -0.5f), 0.0f);
    const int y0 = min((int)sy, h - 1), x0 = min((int)sx, w - 1);
    const int y1 = y0 + (y0 < h - 1 ? 1 : 0), x1 = x0 + (x0 < w - 1 ? 1 : 0);
    const float ly1 = sy - (float)y0, lx1 = sx - (float)x0;
    const float ly0 = 1.0f - ly1, lx0 = 1.0f - lx1;
    float bv = -INFINITY;
    for (int c = 0; c < channels; ++c) {
      const float* pc = prob + (int64_t)c * plane;
      const float top = __builtin_fmaf(lx1, pc[(int64_t)y0 * w + x1], lx0 * pc[(int64_t)y0 * w + x0]);
      const float bot = __builtin_fmaf(lx0, pc[(int64_t)y1 * w + x0], lx1 * pc[(int64_t)y1 * w + x1]);
      const float v = ly0 * top + ly1 * bot;
      if (v > bv) {
        bv = v;
        best = c;
      }
    }
  }
  return best;
}

}  // namespace deva
