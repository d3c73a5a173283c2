// Proposal filter of a promptable segmenter: mask logits and predicted IoUs, batch by batch -> the binary masks, scores
// and boxes that survive the IoU drop, the stability drop and box NMS (the reference's generator,
// deva/ext/SAM/automatic_mask_generator.py:332-352 per batch and :272-278 per image; contract: include/deva_hip.h,
// deva_proposal_batch).  The reference reads every fp32 plane five to seven times and copies the survivors after each
// drop with a host synchronisation; here a live plane is read once, a stored one twice, and nothing synchronises
// before the frame's one copy of the result table:
//
//   per batch
//   stats     grid (chunk, mask): hi = #(x > t_hi), lo = #(x > t_lo) and the box of x > t_mask; wave shuffles, LDS,
//             then one integer atomic per workgroup and field into the mask's record.  A mask that is not live exits.
//   decide    one workgroup, one thread per mask: stability, the arena slot by an order-preserving scan, the table
//             row; re-zeroes the records.
//   binarize  grid (chunk, mask): x > t_mask as bytes into the slot.  A mask without a slot exits.
//   at finish
//   rank      position of every stored mask under (descending iou_pred, ascending arrival)
//   matrix    one lane per pair in that order; the 64-bit row words are the wave's ballot
//   reduce    one wave, lane l holds word l of the removed set: walks the rows, writes the keep list and the result
//   gather    the kept byte planes in keep order (after the host has read how many)
#include "common.h"
#include "proposal_device.h"  // PropArgs, prop_live, PropTally, prop_take, prop_commit, prop_decide_kernel
#include "proposal_plan.h"

namespace deva {
namespace {

// ------------------------------------------------------------------------------------------ begin
__global__ void __launch_bounds__(kPropBatch) prop_begin_kernel(int32_t* stats, int32_t* count, int32_t* nkeep) {
  const int t = threadIdx.x;
  int32_t* s = stats + t * kPropStat;
  s[0] = 0, s[1] = 0, s[2] = INT_MAX, s[3] = INT_MAX, s[4] = -1, s[5] = -1, s[6] = 0, s[7] = 0;
  if (t < 4) count[t] = 0, nkeep[t] = 0;
}

// ------------------------------------------------------------------------------------------ stats
// The plane is walked as one row of hw floats in "aligned space": element e sits at the 16-byte boundary below the
// plane plus 4 e bytes, so a group of four with e % 4 == 0 is one aligned 16-byte load, and the plane is
// e in [shift, shift + hw).  Only the first and the last group of a plane can be partial; they load element by element.
// A thread keeps the column of its element by counting (one division per thread, none per pixel); the row comes from
// the smallest and largest linear index afterwards.
__global__ void __launch_bounds__(256) prop_stats_kernel(PropArgs a) {
  __shared__ int32_t red[4][6];
  const int k = blockIdx.y, t = threadIdx.x;
  if (!prop_live(a, k)) return;  // (never read)
  const float* p = a.logits + (int64_t)k * a.hw;
  const int shift = (int)(reinterpret_cast<uintptr_t>(p) >> 2 & 3);
  const int e_first = blockIdx.x * kPropChunk, e_end = shift + a.hw;
  if (e_first >= e_end) return;
  const float* base = p - shift;  // (16-byte aligned; nothing below the plane is read)
  const int w = a.w, dx = (1024 - 4) % w;
  PropTally s = {0, 0, INT_MAX, -1, INT_MAX, -1};
  int e0 = e_first + 4 * t;
  int x = e0 >= shift ? (e0 - shift) % w : (w - (shift - e0) % w) % w;
#pragma unroll 4
  for (int it = 0; it < kPropChunk / 1024; ++it, e0 += 1024) {
    if (e0 >= e_end) break;
    const int i = e0 - shift;
    if (e0 >= shift && e0 + 4 <= e_end) {
      const float4 v = *reinterpret_cast<const float4*>(base + e0);
      const float f[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        prop_take(a, f[j], i + j, x, s);
        x = x + 1 == w ? 0 : x + 1;
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (e0 + j >= shift && e0 + j < e_end) prop_take(a, base[e0 + j], i + j, x, s);
        x = x + 1 == w ? 0 : x + 1;
      }
    }
    x += dx;
    if (x >= w) x -= w;
  }
  prop_commit(a, k, s, red);
}

// ------------------------------------------------------------------------------------------ decide
// (prop_decide_kernel: proposal_device.h)

// ------------------------------------------------------------------------------------------ binarize
// Aligned space of the OUTPUT plane: byte e sits at the 16-byte boundary below the slot plus e, a full group of 16 is
// one 16-byte store fed by four 16-byte loads (the floats are 4-byte aligned at least; 16 when the planes' sizes agree).
__global__ void __launch_bounds__(256) prop_binarize_kernel(PropArgs a) {
  const int k = blockIdx.y, t = threadIdx.x;
  const int32_t slot = a.slots[k];
  if (slot < 0 || slot >= a.capacity) return;
  const float* p = a.logits + (int64_t)k * a.hw;
  uint8_t* o = a.arena + (int64_t)slot * a.hw;
  const int shift = (int)(reinterpret_cast<uintptr_t>(o) & 15);
  const int e_first = blockIdx.x * kPropChunk, e_end = shift + a.hw;
  const float tm = a.t_mask;
#pragma unroll
  for (int it = 0; it < kPropChunk / 4096; ++it) {
    const int e0 = e_first + it * 4096 + 16 * t;
    if (e0 >= e_end) break;
    const int i = e0 - shift;
    if (e0 >= shift && e0 + 16 <= e_end) {
      uint32_t word[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float4 v;
        __builtin_memcpy(&v, p + i + 4 * q, 16);  // (4-byte aligned: one 16-byte load all the same)
        word[q] = (uint32_t)(v.x > tm) | (uint32_t)(v.y > tm) << 8 | (uint32_t)(v.z > tm) << 16 | (uint32_t)(v.w > tm) << 24;
      }
      *reinterpret_cast<uint4*>(o + i) = make_uint4(word[0], word[1], word[2], word[3]);
    } else {
      for (int j = 0; j < 16; ++j)
        if (e0 + j >= shift && e0 + j < e_end) o[i + j] = p[i + j] > tm;
    }
  }
}

// ------------------------------------------------------------------------------------------ NMS
struct NmsArgs {
  const int32_t* boxes;   // x0, y0, x1, y1 of box i at boxes + i * box_stride: int32 values, or the bits of fp32 ones
  const int32_t* scores;  // fp32 bits of score i at scores + i * score_stride
  int box_stride, score_stride;
  const int32_t* m_dev;  // the number of boxes lives on the device (clamped to m_max), or NULL: m_max boxes
  int m_max, words;
  double thresh;
  int32_t* order;
  unsigned long long* matrix;
  int32_t* keep;
  int32_t* n_keep;
  const int32_t* table;  // proposals: the frame's table and the result to fill from it
  int32_t* result;
};

__device__ __forceinline__ int nms_count(const NmsArgs& a) {
  if (!a.m_dev) return a.m_max;
  const int32_t m = *a.m_dev;
  return m < 0 ? 0 : (m > a.m_max ? a.m_max : m);
}

// j comes before i: the higher score first (NaN, which torch's descending sort puts first, before every number), among
// equal scores the lower index
__device__ __forceinline__ bool nms_before(float sj, int j, float si, int i) {
  const bool nj = sj != sj, ni = si != si;
  if (nj != ni) return nj;
  if (nj) return j < i;
  return sj > si || (sj == si && j < i);
}

__global__ void __launch_bounds__(256) prop_rank_kernel(NmsArgs a) {
  __shared__ float s_score[kPropMaxMasks];
  const int m = nms_count(a);
  for (int j = threadIdx.x; j < m; j += 256) s_score[j] = __int_as_float(a.scores[(int64_t)j * a.score_stride]);
  __syncthreads();
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= m) return;
  const float si = s_score[i];
  int rank = 0;
  for (int j = 0; j < m; ++j) rank += nms_before(s_score[j], j, si, i);
  a.order[rank] = i;  // (a total order: every position is written once)
}

// kFloat: the boxes are fp32 as given (deva_box_nms_xyxy); otherwise int32 pixel indices, converted (rule 5)
template <bool kFloat>
__device__ __forceinline__ float nms_coord(int32_t v) {
  return kFloat ? __int_as_float(v) : (float)v;
}

template <bool kFloat>
__global__ void __launch_bounds__(256) prop_nms_matrix_kernel(NmsArgs a) {
#pragma clang fp contract(off)
  const int m = nms_count(a);
  const int r = blockIdx.y, word = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= m || word >= a.words) return;
  const int c = word * 64 + lane;
  bool over = false;
  if (c > r && c < m) {
    const int32_t* bi = a.boxes + (int64_t)a.order[r] * a.box_stride;
    const int32_t* bj = a.boxes + (int64_t)a.order[c] * a.box_stride;
    const float ax0 = nms_coord<kFloat>(bi[0]), ay0 = nms_coord<kFloat>(bi[1]);
    const float ax1 = nms_coord<kFloat>(bi[2]), ay1 = nms_coord<kFloat>(bi[3]);
    const float bx0 = nms_coord<kFloat>(bj[0]), by0 = nms_coord<kFloat>(bj[1]);
    const float bx1 = nms_coord<kFloat>(bj[2]), by1 = nms_coord<kFloat>(bj[3]);
    const float area_i = (ax1 - ax0) * (ay1 - ay0), area_j = (bx1 - bx0) * (by1 - by0);
    const float iw = fmaxf(0.0f, fminf(ax1, bx1) - fmaxf(ax0, bx0));
    const float ih = fmaxf(0.0f, fminf(ay1, by1) - fmaxf(ay0, by0));
    const float inter = iw * ih;
    const float ovr = __fdiv_rn(inter, area_i + area_j - inter);
    over = (double)ovr > a.thresh;  // (NaN from 0 / 0: false)
  }
  const unsigned long long bits = __ballot(over);
  if (lane == 0) a.matrix[(int64_t)r * a.words + word] = bits;
}

__global__ void __launch_bounds__(64) prop_nms_reduce_kernel(NmsArgs a) {
  const int m = nms_count(a), lane = threadIdx.x;
  unsigned long long removed = 0;  // word `lane` of the set of suppressed positions
  int n = 0;
  for (int r0 = 0; r0 < m; r0 += 8) {
    unsigned long long row[8];
#pragma unroll
    for (int q = 0; q < 8; ++q)  // the rows do not depend on the walk: eight loads in flight
      row[q] = (r0 + q < m && lane < a.words) ? a.matrix[(int64_t)(r0 + q) * a.words + lane] : 0ull;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int r = r0 + q;
      if (r < m) {
        const unsigned long long mine = __shfl(removed, r >> 6);
        if (!(mine >> (r & 63) & 1)) {
          if (lane == 0) a.keep[n] = a.order[r];
          ++n;
          removed |= row[q];
        }
      }
    }
  }
  if (lane == 0) *a.n_keep = n;
  if (!a.result) return;
  __syncthreads();  // (the keep list is read back by the other lanes)
  if (lane == 0) a.result[0] = m, a.result[1] = *a.m_dev, a.result[2] = n, a.result[3] = 0;
  for (int j = lane; j < n; j += 64) {
    const int32_t* row = a.table + (int64_t)a.keep[j] * kPropRow;
    int32_t* to = a.result + kPropHeader + (int64_t)j * kPropRow;
#pragma unroll
    for (int f = 0; f < kPropRow; ++f) to[f] = row[f];
  }
}

// ------------------------------------------------------------------------------------------ gather
__global__ void __launch_bounds__(256) prop_gather_kernel(const uint8_t* arena, int capacity, int hw, const int32_t* keep,
                                                          uint8_t* out) {
  const int j = blockIdx.y, t = threadIdx.x;
  const int32_t slot = keep[j];
  if (slot < 0 || slot >= capacity) return;
  const uint8_t* p = arena + (int64_t)slot * hw;
  uint8_t* o = out + (int64_t)j * hw;
  const int shift = (int)(reinterpret_cast<uintptr_t>(o) & 15);
  const bool words = ((reinterpret_cast<uintptr_t>(p) ^ reinterpret_cast<uintptr_t>(o)) & 3) == 0;
  const int e_first = blockIdx.x * kPropChunk, e_end = shift + hw;
#pragma unroll
  for (int it = 0; it < kPropChunk / 4096; ++it) {
    const int e0 = e_first + it * 4096 + 16 * t;
    if (e0 >= e_end) break;
    const int i = e0 - shift;
    if (words && e0 >= shift && e0 + 16 <= e_end) {
      uint4 v;
      __builtin_memcpy(&v, __builtin_assume_aligned(p + i, 4), 16);
      *reinterpret_cast<uint4*>(o + i) = v;
    } else {
      for (int q = 0; q < 16; ++q)
        if (e0 + q >= shift && e0 + q < e_end) o[i + q] = p[i + q];
    }
  }
}

void nms_launch(const NmsArgs& a, bool boxes_f32, hipStream_t s) {
  hipLaunchKernelGGL(prop_rank_kernel, dim3((unsigned)ceil_div(a.m_max, 256)), dim3(256), 0, s, a);
  const dim3 grid((unsigned)ceil_div(a.words, 4), (unsigned)a.m_max);
  if (boxes_f32)
    hipLaunchKernelGGL(prop_nms_matrix_kernel<true>, grid, dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL(prop_nms_matrix_kernel<false>, grid, dim3(256), 0, s, a);
  hipLaunchKernelGGL(prop_nms_reduce_kernel, dim3(1), dim3(64), 0, s, a);
}

template <typename T>
T* at(void* scratch, int64_t offset) {
  return reinterpret_cast<T*>(static_cast<char*>(scratch) + offset);
}

}  // namespace

// rule 5 alone on n_boxes (checked by the caller: 0..kPropMaxMasks) int32 or fp32 boxes: deva_box_nms and
// deva_box_nms_xyxy (box_prompts.hip)
int box_nms_run(const char* what, const void* boxes, bool boxes_f32, const float* scores, int n_boxes, double thresh,
                void* scratch, int32_t* keep, int32_t* n_keep, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (n_boxes == 0) {
    if (hipMemsetAsync(n_keep, 0, sizeof(int32_t), s) != hipSuccess) return check_launch(what);
    return 0;
  }
  const ProposalPlan p = proposal_plan(n_boxes);
  NmsArgs a = {};
  a.boxes = static_cast<const int32_t*>(boxes), a.scores = reinterpret_cast<const int32_t*>(scores);
  a.box_stride = 4, a.score_stride = 1;
  a.m_max = n_boxes, a.words = p.words;
  a.thresh = thresh;
  a.order = at<int32_t>(scratch, p.off_order), a.matrix = at<unsigned long long>(scratch, p.off_matrix);
  a.keep = keep, a.n_keep = n_keep;
  nms_launch(a, boxes_f32, s);
  return check_launch(what);
}

}  // namespace deva

using namespace deva;

extern "C" int deva_proposal_begin(int capacity, void* scratch, int64_t scratch_bytes, void* stream) {
  if (int e = proposal_begin_check(capacity, scratch, scratch_bytes)) return e;
  const ProposalPlan p = proposal_plan(capacity);
  hipLaunchKernelGGL(prop_begin_kernel, dim3(1), dim3(kPropBatch), 0, (hipStream_t)stream, at<int32_t>(scratch, p.off_stats),
                     at<int32_t>(scratch, p.off_count), at<int32_t>(scratch, p.off_nkeep));
  return check_launch("deva_proposal_begin");
}

extern "C" int deva_proposal_batch(const float* logits, const float* iou_preds, int batch, int height, int width,
                                   double pred_iou_thresh, double stability_score_thresh, double stability_score_offset,
                                   double mask_threshold, uint8_t* arena, int capacity, void* scratch,
                                   int64_t scratch_bytes, void* stream) {
  if (int e = proposal_batch_check(logits, iou_preds, batch, height, width, pred_iou_thresh, stability_score_thresh,
                                   stability_score_offset, mask_threshold, arena, capacity, scratch, scratch_bytes))
    return e;
  const ProposalPlan p = proposal_plan(capacity);
  hipStream_t s = (hipStream_t)stream;
  PropArgs a = {};
  a.hw = height * width, a.w = width;
  a.t_hi = (float)(mask_threshold + stability_score_offset);
  a.t_lo = (float)(mask_threshold - stability_score_offset);
  a.t_mask = (float)mask_threshold;
  a.t_iou = (float)pred_iou_thresh, a.t_stab = (float)stability_score_thresh;
  a.iou_on = pred_iou_thresh > 0.0, a.stab_on = stability_score_thresh > 0.0;
  a.arena = arena, a.capacity = capacity;
  a.stats = at<int32_t>(scratch, p.off_stats), a.slots = at<int32_t>(scratch, p.off_slots);
  a.count = at<int32_t>(scratch, p.off_count), a.table = at<int32_t>(scratch, p.off_table);
  const unsigned chunks = (unsigned)proposal_chunks(height, width);
  for (int first = 0; first < batch; first += kPropBatch) {
    a.nb = batch - first < kPropBatch ? batch - first : kPropBatch;
    a.logits = logits + (int64_t)first * a.hw;
    a.iou = iou_preds + first;
    const dim3 grid(chunks, (unsigned)a.nb);
    hipLaunchKernelGGL(prop_stats_kernel, grid, dim3(256), 0, s, a);
    hipLaunchKernelGGL(prop_decide_kernel, dim3(1), dim3(kPropBatch), 0, s, a);
    hipLaunchKernelGGL(prop_binarize_kernel, grid, dim3(256), 0, s, a);
  }
  return check_launch("deva_proposal_batch");
}

extern "C" int deva_proposal_finish(int capacity, double box_nms_thresh, void* scratch, int64_t scratch_bytes,
                                    int32_t* result, void* stream) {
  if (int e = proposal_finish_check(capacity, box_nms_thresh, scratch, scratch_bytes, result)) return e;
  const ProposalPlan p = proposal_plan(capacity);
  NmsArgs a = {};
  a.table = at<int32_t>(scratch, p.off_table);
  a.boxes = a.table + 3, a.scores = a.table + 1, a.box_stride = a.score_stride = kPropRow;
  a.m_dev = at<int32_t>(scratch, p.off_count), a.m_max = capacity, a.words = p.words;
  a.thresh = box_nms_thresh;
  a.order = at<int32_t>(scratch, p.off_order), a.matrix = at<unsigned long long>(scratch, p.off_matrix);
  a.keep = at<int32_t>(scratch, p.off_keep), a.n_keep = at<int32_t>(scratch, p.off_nkeep);
  a.result = result;
  nms_launch(a, false, (hipStream_t)stream);
  return check_launch("deva_proposal_finish");
}

extern "C" int deva_proposal_gather(const uint8_t* arena, int capacity, int height, int width, const void* scratch,
                                    int64_t scratch_bytes, int n_kept, uint8_t* out, void* stream) {
  if (int e = proposal_gather_check(arena, capacity, height, width, scratch, scratch_bytes, n_kept, out)) return e;
  if (n_kept == 0) return 0;
  const ProposalPlan p = proposal_plan(capacity);
  hipLaunchKernelGGL(prop_gather_kernel, dim3((unsigned)proposal_chunks(height, width), (unsigned)n_kept), dim3(256), 0,
                     (hipStream_t)stream, arena, capacity, height * width,
                     at<const int32_t>(const_cast<void*>(scratch), p.off_keep), out);
  return check_launch("deva_proposal_gather");
}

extern "C" int deva_box_nms(const int32_t* boxes, const float* scores, int n_boxes, double box_nms_thresh, void* scratch,
                            int64_t scratch_bytes, int32_t* keep, int32_t* n_keep, void* stream) {
  if (int e = box_nms_check(boxes, scores, n_boxes, box_nms_thresh, scratch, scratch_bytes, keep, n_keep)) return e;
  return box_nms_run("deva_box_nms", boxes, false, scores, n_boxes, box_nms_thresh, scratch, keep, n_keep, stream);
}
