// Prompt points of an automatic detection frame: the forward mask of the tracker -> the grid points that fall on
// background, which is where the segmenter is asked (the reference's statement, deva/ext/automatic_sam.py:67-89, is
// fifteen ATen launches, a boolean-index copy and a .cpu(); contract: include/deva_hip.h, deva_prompt_points).
//
//   rows    grid (4 rows, 64 outputs): one wave per row loads its segment of the mask with 16-byte loads where the
//           address allows (element by element at the ends), keeps `> 0` as bytes in LDS, then one lane per output
//           reads its 32 bytes (two 16-byte LDS reads) and sums the horizontal filter in tap order -> [H][W/16] fp32
//   low     one thread per cell of the map: the vertical filter over the 32 rows of its window -> [H/16][W/16] fp32
//   sample  ONE workgroup of 1024 threads, rounds of 1024 points: the bilinear sample of the map, the label, and the
//           kept points in input order by wave ballots and a scan of the sixteen wave counts (no atomics)
//
// The filter is the antialiased triangle of aa_taps (pointwise.hip) with scale = 16 exactly: the window of output o is
// the positions 16 o - 8 ... 16 o + 23 clipped to the axis, the weight of the j-th position of the unclipped window is
// 1 - |j - 15.5| / 16 (a multiple of 1/32: the sum of any of them is exact in any order), divided by the sum over the
// positions that exist.  Taps are computed where they are used: no per-thread table.
#include "common.h"
#include "prompt_plan.h"

// Every product and every sum below is its own rounded fp32 operation (the contract fixes their order).  HIP contracts
// a * b + c into one fused operation by default, and the _rn intrinsics do not prevent it (they are a * b and a + b in
// a header that is compiled with contraction on): so contraction is off for this file and the operators are written out.
#pragma clang fp contract(off)

namespace deva {
namespace {

constexpr int kSpan = kPromptScale * kPromptTileX + kPromptScale;  // positions one wave needs: 16 ox0 - 8 ... 16 (ox0 + 64) + 7
static_assert(kSpan % 16 == 0 && kPromptTaps == 2 * kPromptScale, "the LDS rows are read in 16-byte pieces");

// weight, before the division by the window's sum, of position j of an unclipped window
__device__ __forceinline__ constexpr float prompt_tap(int j) {
  return j < kPromptScale ? ((float)j + 0.5f) * (1.0f / kPromptScale) : (31.5f - (float)j) * (1.0f / kPromptScale);
}

// positions [lo, hi) of the unclipped window of output o that lie on an axis of n, and the sum of their weights
__device__ __forceinline__ float prompt_window(int o, int n, int& lo, int& hi) {
  const int first = kPromptScale * o - kPromptScale / 2;
  lo = first < 0 ? -first : 0;
  hi = n - first < kPromptTaps ? n - first : kPromptTaps;
  float total = 0.0f;
#pragma unroll
  for (int j = 0; j < kPromptTaps; ++j)
    if (j >= lo && j < hi) total += prompt_tap(j);
  return total;
}

template <int E>
__device__ __forceinline__ uint8_t prompt_foreground(const uint8_t* p) {
  if (E == 8) return *reinterpret_cast<const int64_t*>(p) > 0;  // 64 bits: a long id above 2^31 is foreground, -3 is not
  return *p > 0;
}

// ------------------------------------------------------------------------------------------ rows
template <int E>
__global__ void __launch_bounds__(256) prompt_rows_kernel(const uint8_t* __restrict__ mask, int h, int w, int low_w,
                                                          float* __restrict__ rows) {
  __shared__ __attribute__((aligned(16))) uint8_t fg[kPromptTileRows][kSpan];
  const int t = threadIdx.x, lane = t & 63, r = t >> 6;
  const int y = blockIdx.x * kPromptTileRows + r, ox0 = blockIdx.y * kPromptTileX;
  const int p0 = kPromptScale * ox0 - kPromptScale / 2;  // position of fg[r][0]
  for (int i = t; i < kPromptTileRows * kSpan / 16; i += 256) reinterpret_cast<uint4*>(&fg[0][0])[i] = make_uint4(0, 0, 0, 0);
  __syncthreads();
  if (y < h) {
    const int xa = p0 < 0 ? 0 : p0, xb = p0 + kSpan < w ? p0 + kSpan : w;  // (xa < xb: ox0 < low_w)
    const uint8_t* row = mask + (int64_t)y * w * E;
    const uint8_t* begin = row + (int64_t)xa * E;
    const uint8_t* end = row + (int64_t)xb * E;
    // "aligned space": group g is the 16 bytes at the 16-byte boundary below `begin` plus 16 g; only the first and
    // the last group of a row can reach outside [begin, end) and those load element by element
    const int shift = (int)(reinterpret_cast<uintptr_t>(begin) & 15);
    const int groups = (int)(((end - begin) + shift + 15) >> 4);
    uint8_t* s = &fg[r][xa - p0] - shift / E;  // s[k] = element k of group 0 (indices below shift / E are never written)
    for (int g = lane; g < groups; g += 64) {
      const uint8_t* a = begin - shift + 16 * (int64_t)g;
      uint8_t* to = s + g * (16 / E);
      if (a >= begin && a + 16 <= end) {
        const uint4 v = *reinterpret_cast<const uint4*>(a);
        if (E == 8) {
          to[0] = (int32_t)v.y > 0 || (v.y == 0 && v.x != 0);
          to[1] = (int32_t)v.w > 0 || (v.w == 0 && v.z != 0);
        } else {
          const uint32_t word[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
          for (int k = 0; k < 16; ++k) to[k] = (word[k >> 2] >> (8 * (k & 3)) & 0xff) != 0;
        }
      } else {
        for (int k = 0; k < 16 / E; ++k) {
          const uint8_t* q = a + k * E;
          if (q >= begin && q < end) to[k] = prompt_foreground<E>(q);
        }
      }
    }
  }
  __syncthreads();
  const int ox = ox0 + lane;
  if (y >= h || ox >= low_w) return;
  const uint4 lo4 = *reinterpret_cast<const uint4*>(&fg[r][16 * lane]);
  const uint4 hi4 = *reinterpret_cast<const uint4*>(&fg[r][16 * lane + 16]);
  const uint32_t word[8] = {lo4.x, lo4.y, lo4.z, lo4.w, hi4.x, hi4.y, hi4.z, hi4.w};
  int lo, hi;
  const float total = prompt_window(ox, w, lo, hi);
  float acc = 0.0f;
#pragma unroll
  for (int j = 0; j < kPromptTaps; ++j)
    if (j >= lo && j < hi) {  // (the value is 0 or 1: the product is the weight or 0, the sum is in tap order)
      const float wj = __fdiv_rn(prompt_tap(j), total);
      acc = acc + ((word[j >> 2] >> (8 * (j & 3)) & 0xff) ? wj : 0.0f);
    }
  rows[(int64_t)y * low_w + ox] = acc;
}

// ------------------------------------------------------------------------------------------ low
__global__ void __launch_bounds__(256) prompt_low_kernel(const float* __restrict__ rows, int h, int low_h, int low_w,
                                                         float* __restrict__ low) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= low_h * low_w) return;
  const int oy = i / low_w, ox = i - oy * low_w;
  int lo, hi;
  const float total = prompt_window(oy, h, lo, hi);
  const float* col = rows + ((int64_t)kPromptScale * oy - kPromptScale / 2) * low_w + ox;  // (read at lo <= j < hi only)
  float acc = 0.0f;
#pragma unroll
  for (int j = 0; j < kPromptTaps; ++j)
    if (j >= lo && j < hi) {
      const float product = col[(int64_t)j * low_w] * __fdiv_rn(prompt_tap(j), total);
      acc = acc + product;
    }
  low[i] = acc;
}

// ------------------------------------------------------------------------------------------ sample
// F.grid_sample(align_corners=False, padding_mode='zeros') of one point, every operation a rounded fp32 one in the
// order of the header (rule 4); a tap outside the map contributes 0, a coordinate that is not finite has no tap inside
__device__ __forceinline__ float prompt_tap_value(const float* low, int low_h, int low_w, float fy, float fx, float wgt) {
  const bool inside = fy >= 0.0f && fy <= (float)(low_h - 1) && fx >= 0.0f && fx <= (float)(low_w - 1);
  return inside ? low[(int)fy * low_w + (int)fx] * wgt : 0.0f;
}

__device__ __forceinline__ float prompt_unnormalize(float c, int n) {
  const float g = c * 2.0f - 1.0f;
  const float scaled = (g + 1.0f) * (float)n;
  return (scaled - 1.0f) * 0.5f;  // (/ 2 is exact either way)
}

__device__ __forceinline__ float prompt_label(const float* low, int low_h, int low_w, float x, float y) {
  const float ix = prompt_unnormalize(x, low_w), iy = prompt_unnormalize(y, low_h);
  const float x0 = floorf(ix), y0 = floorf(iy);
  const float x1 = x0 + 1.0f, y1 = y0 + 1.0f;
  const float rx = x1 - ix, lx = ix - x0, ry = y1 - iy, ly = iy - y0;
  const float nw = prompt_tap_value(low, low_h, low_w, y0, x0, rx * ry);
  const float ne = prompt_tap_value(low, low_h, low_w, y0, x1, lx * ry);
  const float sw = prompt_tap_value(low, low_h, low_w, y1, x0, rx * ly);
  const float se = prompt_tap_value(low, low_h, low_w, y1, x1, lx * ly);
  return ((nw + ne) + sw) + se;
}

__global__ void __launch_bounds__(1024) prompt_sample_kernel(const float* __restrict__ low, int low_h, int low_w,
                                                             const float* __restrict__ points_xy, int points, float threshold,
                                                             float* __restrict__ out_points, float* __restrict__ out_labels,
                                                             int32_t* __restrict__ out_count) {
  __shared__ int32_t wave_sum[1024 / 64];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  int kept_before = 0;  // kept points of the earlier rounds
  for (int first = 0; first < points; first += 1024) {
    const int i = first + t;
    bool keep = false;
    float x = 0.0f, y = 0.0f;
    if (i < points) {
      x = points_xy[2 * i], y = points_xy[2 * i + 1];
      const float label = prompt_label(low, low_h, low_w, x, y);
      out_labels[i] = label;
      keep = label < threshold;  // strict; a NaN label is not kept
    }
    const unsigned long long ballot = __ballot(keep);
    if (lane == 0) wave_sum[wave] = __popcll(ballot);
    __syncthreads();
    int offset = 0, total = 0;
    for (int v = 0; v < 1024 / 64; ++v) {
      const int n = wave_sum[v];
      offset += v < wave ? n : 0;
      total += n;
    }
    if (keep) {
      const int at = kept_before + offset + __popcll(ballot & ((1ull << lane) - 1));  // input order; at <= i < points
      out_points[2 * at] = x, out_points[2 * at + 1] = y;
    }
    kept_before += total;
    __syncthreads();  // (wave_sum is rewritten by the next round)
  }
  if (t == 0) out_count[0] = kept_before;
}

}  // namespace
}  // namespace deva

using namespace deva;

extern "C" int deva_prompt_points(const void* mask, int mask_elem_bytes, int height, int width, const float* points_xy,
                                  int points, double threshold, void* scratch, int64_t scratch_bytes, float* out_points,
                                  float* out_labels, int32_t* out_count, void* stream) {
  if (int e = prompt_points_check(mask, mask_elem_bytes, height, width, points_xy, points, threshold, scratch, scratch_bytes,
                                  out_points, out_labels, out_count))
    return e;
  const PromptPlan p = prompt_plan(height, width);
  hipStream_t s = (hipStream_t)stream;
  float* rows = reinterpret_cast<float*>(static_cast<char*>(scratch) + p.off_rows);
  float* low = reinterpret_cast<float*>(static_cast<char*>(scratch) + p.off_low);
  const dim3 tiles((unsigned)ceil_div(height, kPromptTileRows), (unsigned)ceil_div(p.low_w, kPromptTileX));
  if (mask_elem_bytes == 8)
    hipLaunchKernelGGL(prompt_rows_kernel<8>, tiles, dim3(256), 0, s, static_cast<const uint8_t*>(mask), height, width,
                       p.low_w, rows);
  else
    hipLaunchKernelGGL(prompt_rows_kernel<1>, tiles, dim3(256), 0, s, static_cast<const uint8_t*>(mask), height, width,
                       p.low_w, rows);
  hipLaunchKernelGGL(prompt_low_kernel, dim3((unsigned)ceil_div((int64_t)p.low_h * p.low_w, 256)), dim3(256), 0, s, rows,
                     height, p.low_h, p.low_w, low);
  hipLaunchKernelGGL(prompt_sample_kernel, dim3(1), dim3(1024), 0, s, low, p.low_h, p.low_w, points_xy, points,
                     (float)threshold, out_points, out_labels, out_count);
  return check_launch("deva_prompt_points");
}
