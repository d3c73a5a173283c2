// The per-pixel decision of the output tail, shared by deva_index_mask (merge.hip) and deva_frame_result
// (frame_result.hip): channel index of the first maximum of the probabilities resized to the output size.  The
// sampling itself (resize_taps / resize_sample) is also what deva_detection_assemble (detections.hip) resizes a
// detector's byte masks with.
//
// Bilinear arithmetic follows ATen's upsample_bilinear2d (align_corners=False): source coordinate
// scale*(dst+0.5)-0.5 clamped at 0, neighbour index clamped at the border, rows blended after columns.  The
// roundings are written out (one fused multiply-add for the coordinate; per row one rounded product and one fused
// multiply-add; the row blend two rounded products and an add -- the form deva_index_mask has always been compiled
// to, see also ensemble.hip) so that every translation unit that includes this file decides a near-tie the same way.
#pragma once
#include "common.h"

namespace deva {

// where one output pixel samples its source plane: the two rows, the two columns and their weights
struct ResizeTaps {
  int y0, y1, x0, x1;
  float ly0, ly1, lx0, lx1;
};

__device__ __forceinline__ ResizeTaps resize_taps(int h, int w, float scale_y, float scale_x, int y, int x) {
#pragma clang fp contract(off)
  ResizeTaps t;
  const float sy = fmaxf(__builtin_fmaf(scale_y, (float)y + 0.5f, -0.5f), 0.0f);
  const float sx = fmaxf(__builtin_fmaf(scale_x, (float)x + 0.5f, -0.5f), 0.0f);
  t.y0 = min((int)sy, h - 1);
  t.x0 = min((int)sx, w - 1);
  t.y1 = t.y0 + (t.y0 < h - 1 ? 1 : 0);
  t.x1 = t.x0 + (t.x0 < w - 1 ? 1 : 0);
  t.ly1 = sy - (float)t.y0;
  t.lx1 = sx - (float)t.x0;
  t.ly0 = 1.0f - t.ly1;
  t.lx0 = 1.0f - t.lx1;
  return t;
}

// the resized value of one [h][w] plane (fp32, or bytes read as their value) at the taps
template <typename T>
__device__ __forceinline__ float resize_sample(const ResizeTaps& t, const T* __restrict__ pc, int w) {
#pragma clang fp contract(off)
  const float top =
      __builtin_fmaf(t.lx1, (float)pc[(int64_t)t.y0 * w + t.x1], t.lx0 * (float)pc[(int64_t)t.y0 * w + t.x0]);
  const float bot =
      __builtin_fmaf(t.lx0, (float)pc[(int64_t)t.y1 * w + t.x0], t.lx1 * (float)pc[(int64_t)t.y1 * w + t.x1]);
  return t.ly0 * top + t.ly1 * bot;
}

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
    const ResizeTaps t = resize_taps(h, w, scale_y, scale_x, y, x);
    float bv = -INFINITY;
    for (int c = 0; c < channels; ++c) {
      const float v = resize_sample(t, prob + (int64_t)c * plane, w);
      if (v > bv) {
        bv = v;
        best = c;
      }
    }
  }
  return best;
}

}  // namespace deva
