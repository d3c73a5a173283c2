// Detector output -> (index mask, per-mask records): the tails of the reference's auto_segment
// (deva/ext/automatic_sam.py:93-145, both policies) and segment_with_text (deva/ext/grounding_dino.py:117-142), which
// make an N*H*W fp32 copy of the masks, two scaled copies and an argmax, and then loop over the masks on the host with
// several full-frame passes and synchronisations each.  Here the N byte planes are read twice (contract:
// include/deva_hip.h, deva_detection_assemble):
//
//   area    grid (chunk, mask): per-workgroup partial sums of P_k (fp32, fixed order), of #(P_k > 0.5) and of the
//           mask's own pixel count into scratch; no atomics.  At equal sizes P_k is the byte and 16 of them are one load.
//   prep    one workgroup: the partials in chunk order -> area_k, the score multiplier of the policy (area_k,
//           2 max(area) - area_k, or 1 + the paint position for the text policy); zeroes the counters of `decide`.
//   decide  per output pixel the first maximum over the N planes against the background -> uint16 plane
//           (hard index | (P_hard >= 0.5) << 15); mask_area and `both` per mask in LDS counters (integer atomics,
//           exact), merged into the global table with one atomic per touched entry.
//   table   one workgroup: keep rule, ids by a prefix scan in index (or paint) order -> id table and the records.
//   paint   int64 [oh][ow] through the id table.
//
// The text policy is the same pipeline: painting in a fixed order with "later overwrites earlier" is the covering
// mask with the last paint position, so its score is (P_k > 0.5) * (1 + position) against a background of 0.
// P_k is resize_sample (index_argmax.h): the arithmetic of deva_index_mask.
#include "common.h"
#include "detection_plan.h"
#include "index_argmax.h"

namespace deva {
namespace {

enum { DET_VEC16 = 0, DET_BYTES = 1, DET_RESIZE = 2 };  // how a kernel reads P_k

struct DetArgs {
  const uint8_t* masks;
  int n, h0, w0, oh, ow;
  float scale_y, scale_x;
  int policy;
  float threshold;
  int consistent;
  int chunks;
  float* part_area;
  int32_t* part_orig;
  int32_t* part_src;
  float* area;
  int32_t* orig;
  int32_t* src;
  float* mult;
  int32_t* stats;
  int32_t* lut;
  uint16_t* plane;
  const float* scores;
  int64_t* out;
  int32_t* records;
};

__device__ __forceinline__ int byte_of(const uint4& v, int j) {
  const uint32_t w = j < 4 ? v.x : (j < 8 ? v.y : (j < 12 ? v.z : v.w));
  return (int)(w >> (8 * (j & 3)) & 0xff);
}

// ------------------------------------------------------------------------------------------ area
template <int MODE>
__global__ void __launch_bounds__(256) det_area_kernel(DetArgs a) {
  __shared__ float red_area[256];
  __shared__ int32_t red_orig[256], red_src[256];
  const int k = blockIdx.y, c = blockIdx.x, t = threadIdx.x;
  const int64_t dst = (int64_t)a.oh * a.ow, srcn = (int64_t)a.h0 * a.w0;
  const uint8_t* pk = a.masks + (int64_t)k * srcn;
  const int64_t lo = (int64_t)c * kDetChunk;
  const int64_t hi = lo + kDetChunk < dst ? lo + kDetChunk : dst;
  float sum = 0.0f;
  int32_t orig = 0, src = 0;
  if (MODE == DET_VEC16) {  // (dst % 16 == 0: the range is whole groups of 16)
    int32_t bytes = 0;
    for (int64_t i = lo + t * 16; i < hi; i += 256 * 16) {
      const uint4 v = *reinterpret_cast<const uint4*>(pk + i);
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const int b = byte_of(v, j);
        bytes += b;
        orig += b != 0;
      }
    }
    sum = (float)bytes;  // (at most 16384 * 255: exact)
    src = orig;
  } else if (MODE == DET_BYTES) {
    int32_t bytes = 0;
    for (int64_t i = lo + t; i < hi; i += 256) {
      const int b = pk[i];
      bytes += b;
      orig += b != 0;
    }
    sum = (float)bytes;
    src = orig;
  } else {
    for (int64_t i = lo + t; i < hi; i += 256) {
      const int y = (int)(i / a.ow), x = (int)(i - (int64_t)y * a.ow);
      const float p = resize_sample(resize_taps(a.h0, a.w0, a.scale_y, a.scale_x, y, x), pk, a.w0);
      sum += p;
      orig += p > 0.5f;
    }
    const int64_t shi = lo + kDetChunk < srcn ? lo + kDetChunk : srcn;
    for (int64_t i = lo + t; i < shi; i += 256) src += pk[i] != 0;
  }
  red_area[t] = sum;
  red_orig[t] = orig;
  red_src[t] = src;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {  // a fixed tree: the same sum for the same bytes, run after run
    if (t < s) {
      red_area[t] += red_area[t + s];
      red_orig[t] += red_orig[t + s];
      red_src[t] += red_src[t + s];
    }
    __syncthreads();
  }
  if (t == 0) {
    const int64_t at = (int64_t)k * a.chunks + c;
    a.part_area[at] = red_area[0];
    a.part_orig[at] = red_orig[0];
    a.part_src[at] = red_src[0];
  }
}

// ------------------------------------------------------------------------------------------ prep
__global__ void __launch_bounds__(1024) det_prep_kernel(DetArgs a) {
#pragma clang fp contract(off)
  __shared__ float s_area[kDetMaxMasks];
  __shared__ int32_t s_src[kDetMaxMasks];
  __shared__ float s_max[1024];
  const int t = threadIdx.x, n = a.n;
  float mx = 0.0f;
  for (int k = t; k < n; k += 1024) {
    float area = 0.0f;
    int32_t orig = 0, src = 0;
    for (int c = 0; c < a.chunks; ++c) {  // chunk order, always
      const int64_t at = (int64_t)k * a.chunks + c;
      area += a.part_area[at];
      orig += a.part_orig[at];
      src += a.part_src[at];
    }
    a.area[k] = area;
    a.orig[k] = orig;
    a.src[k] = src;
    s_area[k] = area;
    s_src[k] = src;
    mx = fmaxf(mx, area);
  }
  s_max[t] = mx;
  for (int i = t; i < (n + 1) * 2; i += 1024) a.stats[i] = 0;
  __syncthreads();
  for (int s = 512; s > 0; s >>= 1) {
    if (t < s) s_max[t] = fmaxf(s_max[t], s_max[t + s]);
    __syncthreads();
  }
  const float top = s_max[0];
  for (int k = t; k < n; k += 1024) {
    float m;
    if (a.policy == DET_SUPPRESS_SMALL) {
      m = s_area[k];
    } else if (a.policy == DET_PREFER_SMALL) {
      m = top * 2.0f - s_area[k];
    } else {  // paint position: larger masks first, among equal ones the higher index first
      const int32_t mine = s_src[k];
      int before = 0;
      for (int j = 0; j < n; ++j) {
        const int32_t other = s_src[j];
        before += other > mine || (other == mine && j > k);
      }
      m = (float)(before + 1);
    }
    a.mult[k] = m;
  }
}

// ------------------------------------------------------------------------------------------ decide
__device__ __forceinline__ float det_score(bool text, float p, float m) {
#pragma clang fp contract(off)
  return text ? (p > 0.5f ? m : 0.0f) : p * m;
}

__device__ __forceinline__ void det_count(int32_t* table, int hard, int count, int both) {
  atomicAdd(table + hard * 2, count);
  if (both) atomicAdd(table + hard * 2 + 1, both);
}

template <int MODE, bool TEXT>
__global__ void __launch_bounds__(256) det_decide_kernel(DetArgs a) {
  extern __shared__ int32_t lds_count[];  // [n + 1][2]: mask_area, both
  const int n = a.n;
  for (int i = threadIdx.x; i < (n + 1) * 2; i += blockDim.x) lds_count[i] = 0;
  __syncthreads();
  const int64_t dst = (int64_t)a.oh * a.ow, srcn = (int64_t)a.h0 * a.w0;
  const float background = TEXT ? 0.0f : 0.1f;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  if (MODE == DET_VEC16) {
    const int64_t groups = dst >> 4;
    for (int64_t g = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; g < groups; g += stride) {
      const uint8_t* at = a.masks + (g << 4);
      float bv[16], bp[16];
      int best[16];
#pragma unroll
      for (int j = 0; j < 16; ++j) bv[j] = background, bp[j] = 0.0f, best[j] = 0;
#pragma unroll 4
      for (int k = 0; k < n; ++k) {
        const uint4 v = *reinterpret_cast<const uint4*>(at + (int64_t)k * srcn);
        const float m = a.mult[k];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          const float p = (float)byte_of(v, j);
          const float s = det_score(TEXT, p, m);
          if (s > bv[j]) bv[j] = s, bp[j] = p, best[j] = k + 1;
        }
      }
      uint32_t w[8];
      int run = best[0], count = 0, both = 0;  // runs of one mask among the 16 pixels: one update each
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const int flag = TEXT ? (best[j] != 0) : (bp[j] >= 0.5f);
        const uint32_t v = (uint32_t)best[j] | (uint32_t)flag << 15;
        w[j >> 1] = (j & 1) ? (w[j >> 1] | v << 16) : v;
        if (best[j] != run) {
          det_count(lds_count, run, count, both);
          run = best[j], count = 0, both = 0;
        }
        ++count;
        both += flag;
      }
      det_count(lds_count, run, count, both);
      uint4* to = reinterpret_cast<uint4*>(a.plane + (g << 4));
      to[0] = make_uint4(w[0], w[1], w[2], w[3]);
      to[1] = make_uint4(w[4], w[5], w[6], w[7]);
    }
  } else {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < dst; i += stride) {
      ResizeTaps taps = {};
      if (MODE == DET_RESIZE) {
        const int y = (int)(i / a.ow), x = (int)(i - (int64_t)y * a.ow);
        taps = resize_taps(a.h0, a.w0, a.scale_y, a.scale_x, y, x);
      }
      float bv = background, bp = 0.0f;
      int best = 0;
#pragma unroll 4
      for (int k = 0; k < n; ++k) {
        const uint8_t* pk = a.masks + (int64_t)k * srcn;
        const float p = MODE == DET_RESIZE ? resize_sample(taps, pk, a.w0) : (float)pk[i];
        const float s = det_score(TEXT, p, a.mult[k]);
        if (s > bv) bv = s, bp = p, best = k + 1;
      }
      const int flag = TEXT ? (best != 0) : (bp >= 0.5f);
      a.plane[i] = (uint16_t)(best | flag << 15);
      det_count(lds_count, best, 1, flag);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < (n + 1) * 2; i += blockDim.x)
    if (lds_count[i]) atomicAdd(a.stats + i, lds_count[i]);
}

// ------------------------------------------------------------------------------------------ table
__device__ __forceinline__ bool det_keep(const DetArgs& a, int k) {
  const int32_t mask_area = a.stats[(k + 1) * 2], both = a.stats[(k + 1) * 2 + 1], orig = a.orig[k];
  if (a.policy == DET_TEXT) return orig > 0;
  if (a.policy == DET_PREFER_SMALL) return mask_area > 0;
  // (hard == k).sum() / (P_k > 0.5).sum() < threshold, as torch evaluates it: both counts to fp32, an fp32 division,
  // the threshold rounded to fp32
  return mask_area > 0 && orig > 0 && both > 0 && !(__fdiv_rn((float)mask_area, (float)orig) < a.threshold);
}

__global__ void __launch_bounds__(256) det_table_kernel(DetArgs a) {
  __shared__ int32_t s_mask_of[kDetMaxMasks];  // slot in id order -> mask
  __shared__ int32_t s_part[256];
  const int t = threadIdx.x, n = a.n;
  const bool text = a.policy == DET_TEXT;
  for (int k = t; k < n; k += 256) s_mask_of[text ? (int)a.mult[k] - 1 : k] = k;
  __syncthreads();
  const int per = (n + 255) / 256;
  const int lo = min(t * per, n), hi = min(lo + per, n);
  int32_t kept = 0;
  for (int s = lo; s < hi; ++s) kept += det_keep(a, s_mask_of[s]);
  s_part[t] = kept;
  __syncthreads();
  if (t == 0) {
    int32_t run = 0;
    for (int i = 0; i < 256; ++i) {
      const int32_t v = s_part[i];
      s_part[i] = run;
      run += v;
    }
    a.lut[0] = 0;
  }
  __syncthreads();
  int32_t run = s_part[t];
  for (int s = lo; s < hi; ++s) {
    const int k = s_mask_of[s];
    const int32_t id = det_keep(a, k) ? ++run : 0;
    a.lut[k + 1] = (a.policy == DET_PREFER_SMALL && !a.consistent) ? k + 1 : id;
    int32_t* r = a.records + (int64_t)k * kDetRecord;
    r[0] = id;
    r[1] = a.stats[(k + 1) * 2];
    r[2] = a.orig[k];
    r[3] = a.stats[(k + 1) * 2 + 1];
    r[4] = a.src[k];
    r[5] = s;
    r[6] = a.scores ? __float_as_int(a.scores[k]) : 0;
    r[7] = 0;
  }
}

// ------------------------------------------------------------------------------------------ paint
template <bool VEC>
__global__ void __launch_bounds__(256) det_paint_kernel(DetArgs a) {
  const int64_t dst = (int64_t)a.oh * a.ow;
  const bool need_flag = a.policy == DET_SUPPRESS_SMALL;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t items = VEC ? dst >> 2 : dst;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < items; i += stride) {
    if (VEC) {
      const uint2 v = *reinterpret_cast<const uint2*>(a.plane + (i << 2));
      const uint32_t p[4] = {v.x & 0xffff, v.x >> 16, v.y & 0xffff, v.y >> 16};
      int64_t id[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) id[j] = (need_flag && !(p[j] >> 15)) ? 0 : (int64_t)a.lut[p[j] & 0x7fff];
      longlong2* to = reinterpret_cast<longlong2*>(a.out + (i << 2));
      to[0] = make_longlong2(id[0], id[1]);
      to[1] = make_longlong2(id[2], id[3]);
    } else {
      const uint32_t p = a.plane[i];
      a.out[i] = (need_flag && !(p >> 15)) ? 0 : (int64_t)a.lut[p & 0x7fff];
    }
  }
}

}  // namespace
}  // namespace deva

using namespace deva;

extern "C" int deva_detection_assemble(const uint8_t* masks, int n_masks, int height, int width, int out_height,
                                       int out_width, int policy, double overlap_threshold, int consistent_ids,
                                       const float* scores, void* scratch, int64_t scratch_bytes, int64_t* out,
                                       int32_t* records, void* stream) {
  if (int e = detection_check(masks, n_masks, height, width, out_height, out_width, policy, overlap_threshold, scratch,
                              scratch_bytes, out, records))
    return e;
  hipStream_t s = (hipStream_t)stream;
  const int64_t dst = (int64_t)out_height * out_width;
  if (n_masks == 0) {
    if (hipMemsetAsync(out, 0, (size_t)dst * sizeof(int64_t), s) != hipSuccess) return check_launch("deva_detection_assemble");
    return 0;
  }
  const DetectionPlan p = detection_plan(n_masks, height, width, out_height, out_width);
  char* base = static_cast<char*>(scratch);
  DetArgs a = {};
  a.masks = masks;
  a.n = n_masks, a.h0 = height, a.w0 = width, a.oh = out_height, a.ow = out_width;
  a.scale_y = (float)height / (float)out_height;
  a.scale_x = (float)width / (float)out_width;
  a.policy = policy;
  a.threshold = (float)overlap_threshold;
  a.consistent = consistent_ids != 0;
  a.chunks = p.chunks;
  a.part_area = reinterpret_cast<float*>(base + p.off_part_area);
  a.part_orig = reinterpret_cast<int32_t*>(base + p.off_part_orig);
  a.part_src = reinterpret_cast<int32_t*>(base + p.off_part_src);
  a.area = reinterpret_cast<float*>(base + p.off_area);
  a.orig = reinterpret_cast<int32_t*>(base + p.off_orig);
  a.src = reinterpret_cast<int32_t*>(base + p.off_src);
  a.mult = reinterpret_cast<float*>(base + p.off_mult);
  a.stats = reinterpret_cast<int32_t*>(base + p.off_stats);
  a.lut = reinterpret_cast<int32_t*>(base + p.off_lut);
  a.plane = reinterpret_cast<uint16_t*>(base + p.off_plane);
  a.scores = scores;
  a.out = out;
  a.records = records;

  const bool equal = out_height == height && out_width == width;
  const int mode = !equal ? DET_RESIZE
                          : (dst % 16 == 0 && aligned(masks, 16) ? DET_VEC16 : DET_BYTES);
  const bool text = policy == DET_TEXT;
  const dim3 t(256), area_grid((unsigned)p.chunks, (unsigned)n_masks);
  int64_t blocks = ceil_div(mode == DET_VEC16 ? dst / 16 : dst, 256);
  if (blocks > 2048) blocks = 2048;
  const dim3 g((unsigned)blocks);
  const size_t smem = sizeof(int32_t) * 2 * ((size_t)n_masks + 1);
#define DEVA_DET_LAUNCH(M)                                                                     \
  do {                                                                                         \
    hipLaunchKernelGGL((det_area_kernel<M>), area_grid, t, 0, s, a);                           \
    hipLaunchKernelGGL(det_prep_kernel, dim3(1), dim3(1024), 0, s, a);                         \
    if (text) hipLaunchKernelGGL((det_decide_kernel<M, true>), g, t, smem, s, a);              \
    else hipLaunchKernelGGL((det_decide_kernel<M, false>), g, t, smem, s, a);                  \
  } while (0)
  if (mode == DET_VEC16) DEVA_DET_LAUNCH(DET_VEC16);
  else if (mode == DET_BYTES) DEVA_DET_LAUNCH(DET_BYTES);
  else DEVA_DET_LAUNCH(DET_RESIZE);
#undef DEVA_DET_LAUNCH
  hipLaunchKernelGGL(det_table_kernel, dim3(1), dim3(256), 0, s, a);
  const bool vec = dst % 4 == 0 && aligned(out, 16);
  int64_t paint_blocks = ceil_div(vec ? dst / 4 : dst, 256);
  if (paint_blocks > 2048) paint_blocks = 2048;
  if (vec) hipLaunchKernelGGL((det_paint_kernel<true>), dim3((unsigned)paint_blocks), t, 0, s, a);
  else hipLaunchKernelGGL((det_paint_kernel<false>), dim3((unsigned)paint_blocks), t, 0, s, a);
  return check_launch("deva_detection_assemble");
}
