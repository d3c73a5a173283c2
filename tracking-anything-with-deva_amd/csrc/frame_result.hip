// Per-frame results (deva/inference/result_utils.py:88-285): what the reference's saver thread computes on the host
// from an int64 H*W mask -- one masked assignment per object for the id remap, one full-frame compare per segment for
// the area and another for the run-length code, one compare-and-paint per object for the RGB id image and a float
// blend of the whole frame -- comes out of one pass over the probabilities here, and a second small kernel group
// turns the channel-index plane into the COCO run boundaries of every object at once.
//
// deva_frame_result decides each output pixel with resized_argmax (index_argmax.h, the decision of deva_index_mask)
// and writes whichever of the products the caller passed a pointer for.
//
// The overlay (result_utils.py:240-242) is (image * alpha + rgb * (1 - alpha)).astype(uint8) with alpha = 1 where
// the object id is 0 and 0.5 elsewhere.  image and rgb are integers <= 255: their halves are exact in fp32, and so is
// the sum of two halves (a multiple of 0.5 below 256); the cast truncates.  The contract is therefore the integer
// form: the image byte where the id is 0, else (image + rgb) >> 1.
//
// Statistics are integer atomics (add / min / max): exact and independent of the order of the pixels.  A workgroup
// accumulates in LDS and merges every touched entry into the global table with one atomic each; tables beyond
// kStatsLdsChannels channels go to the global table directly.
#include <limits.h>

#include "common.h"
#include "index_argmax.h"

namespace deva {
namespace {

constexpr int kStatsLdsChannels = 1024;  // 5 * 4 B per channel: 20 KiB of LDS
enum { STATS_NONE = 0, STATS_LDS = 1, STATS_GLOBAL = 2 };

struct FrameArgs {
  const float* prob;
  int channels, h, w, oh, ow;
  float scale_y, scale_x;
  const int64_t* lut;
  int n_lut;
  const uint8_t* color_lut;
  const uint8_t* image;
  int16_t* index;
  int64_t* labels;
  int32_t* stats;
  uint8_t* color;
  uint8_t* gray;
  uint8_t* blend;
};

__global__ void stats_init_kernel(int32_t* __restrict__ stats, int channels) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= channels * 5) return;
  const int f = i % 5;
  stats[i] = f == 0 ? 0 : (f <= 2 ? INT_MAX : -1);
}

// a run of `count` pixels of channel c in row y from column xa to xb.  The extrema only ever move one way, so a
// plain read that already satisfies the bound makes the atomic unnecessary (a stale read can only cause a
// redundant atomic, never a missed one).
__device__ __forceinline__ void stats_run(int32_t* table, int c, int count, int xa, int xb, int y) {
  int32_t* e = table + c * 5;
  volatile int32_t* v = e;
  atomicAdd(e, count);
  if (xa < v[1]) atomicMin(e + 1, xa);
  if (y < v[2]) atomicMin(e + 2, y);
  if (xb > v[3]) atomicMax(e + 3, xb);
  if (y > v[4]) atomicMax(e + 4, y);
}

__device__ __forceinline__ uint32_t pack4(const int* b) {
  return (uint32_t)b[0] | (uint32_t)b[1] << 8 | (uint32_t)b[2] << 16 | (uint32_t)b[3] << 24;
}

// A thread owns 4 adjacent pixels of one output row.  VEC: ow % 4 == 0 and every plane is aligned for the packed
// store of its 4 pixels (8 B of index, 2 x 16 B of labels, 4 B of gray, 12 B = 3 dwords of color / blend / image);
// otherwise every element is stored on its own and the pixels past the end of a row are dropped.
template <bool VEC, int STATS>
__global__ void __launch_bounds__(256) frame_result_kernel(FrameArgs a) {
  extern __shared__ int32_t lds_stats[];  // [channels][5], STATS_LDS only
  const int oh = a.oh, ow = a.ow;
  if (STATS == STATS_LDS) {
    for (int i = threadIdx.x; i < a.channels * 5; i += blockDim.x) {
      const int f = i % 5;
      lds_stats[i] = f == 0 ? 0 : (f <= 2 ? INT_MAX : -1);
    }
    __syncthreads();
  }
  const int gw = (ow + 3) >> 2;
  const int64_t groups = (int64_t)oh * gw;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < groups; i += (int64_t)gridDim.x * blockDim.x) {
    const int y = (int)(i / gw);
    const int x = (int)(i - (int64_t)y * gw) << 2;
    const int n = VEC ? 4 : min(4, ow - x);
    int best[4];
    int64_t label[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      // (a pixel past the end of the row repeats the last one and is never stored or counted)
      best[p] = resized_argmax(a.prob, a.channels, a.h, a.w, oh, ow, a.scale_y, a.scale_x, y, min(x + p, ow - 1));
      label[p] = a.lut ? (best[p] < a.n_lut ? a.lut[best[p]] : 0) : (int64_t)best[p];
    }
    const int64_t at = (int64_t)y * ow + x;

    if (a.index) {
      if (VEC) {
        *reinterpret_cast<uint2*>(a.index + at) =
            make_uint2((uint32_t)best[0] | (uint32_t)best[1] << 16, (uint32_t)best[2] | (uint32_t)best[3] << 16);
      } else {
#pragma unroll
        for (int p = 0; p < 4; ++p)
          if (p < n) a.index[at + p] = (int16_t)best[p];
      }
    }
    if (a.labels) {
      if (VEC) {
        *reinterpret_cast<longlong2*>(a.labels + at) = make_longlong2(label[0], label[1]);
        *reinterpret_cast<longlong2*>(a.labels + at + 2) = make_longlong2(label[2], label[3]);
      } else {
#pragma unroll
        for (int p = 0; p < 4; ++p)
          if (p < n) a.labels[at + p] = label[p];
      }
    }
    if (a.gray) {
      if (VEC) {
        int g[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) g[p] = (int)(label[p] & 0xff);
        *reinterpret_cast<uint32_t*>(a.gray + at) = pack4(g);
      } else {
#pragma unroll
        for (int p = 0; p < 4; ++p)
          if (p < n) a.gray[at + p] = (uint8_t)(label[p] & 0xff);
      }
    }
    if (a.color || a.blend) {
      int rgb[12], mix[12];
#pragma unroll
      for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int k = 0; k < 3; ++k) rgb[p * 3 + k] = a.color_lut[best[p] * 3 + k];
      if (a.blend) {
        if (VEC) {
          const uint32_t* src = reinterpret_cast<const uint32_t*>(a.image + at * 3);
#pragma unroll
          for (int d = 0; d < 3; ++d) {
            const uint32_t v = src[d];
#pragma unroll
            for (int k = 0; k < 4; ++k) mix[d * 4 + k] = (int)(v >> (8 * k) & 0xff);
          }
        } else {
#pragma unroll
          for (int j = 0; j < 12; ++j) mix[j] = j < n * 3 ? a.image[at * 3 + j] : 0;
        }
#pragma unroll
        for (int j = 0; j < 12; ++j)
          if (label[j / 3] != 0) mix[j] = (mix[j] + rgb[j]) >> 1;
      }
      if (VEC) {
        if (a.color) {
          uint32_t* dst = reinterpret_cast<uint32_t*>(a.color + at * 3);
#pragma unroll
          for (int d = 0; d < 3; ++d) dst[d] = pack4(rgb + d * 4);
        }
        if (a.blend) {
          uint32_t* dst = reinterpret_cast<uint32_t*>(a.blend + at * 3);
#pragma unroll
          for (int d = 0; d < 3; ++d) dst[d] = pack4(mix + d * 4);
        }
      } else {
#pragma unroll
        for (int j = 0; j < 12; ++j) {
          if (j < n * 3) {
            if (a.color) a.color[at * 3 + j] = (uint8_t)rgb[j];
            if (a.blend) a.blend[at * 3 + j] = (uint8_t)mix[j];
          }
        }
      }
    }
    if (STATS != STATS_NONE) {
      int32_t* table = STATS == STATS_LDS ? lds_stats : a.stats;
      int run_c = best[0], run_x = 0;  // runs of equal channel among the thread's pixels: one update each
#pragma unroll
      for (int p = 1; p < 4; ++p) {
        if (p < n && best[p] != run_c) {
          stats_run(table, run_c, p - run_x, x + run_x, x + p - 1, y);
          run_c = best[p];
          run_x = p;
        }
      }
      stats_run(table, run_c, n - run_x, x + run_x, x + n - 1, y);
    }
  }
  if (STATS == STATS_LDS) {
    __syncthreads();
    for (int c = threadIdx.x; c < a.channels; c += blockDim.x) {
      const int32_t* e = lds_stats + c * 5;
      if (e[0] == 0) continue;
      int32_t* g = a.stats + c * 5;
      atomicAdd(g, e[0]);
      atomicMin(g + 1, e[1]);
      atomicMin(g + 2, e[2]);
      atomicMax(g + 3, e[3]);
      atomicMax(g + 4, e[4]);
    }
  }
}

// ------------------------------------------------------------------------------------------ run-length boundaries
// Positions run column-major, p = x * oh + y (the COCO order).  The index plane is transposed once through LDS
// tiles into that order, so that both passes below read it with unit stride.  A workgroup is one wave and owns a
// contiguous range of positions: `count` leaves its number of boundaries per channel, a scan turns the
// (channel, workgroup) table into write offsets, and `write` walks the range 64 positions at a time, ranks the
// boundaries of one channel by a ballot and advances that channel's cursor in LDS.  Integer counts and ordinary
// launches in stream order only.
constexpr int kRleMaxChannels = 4096;     // one LDS counter / cursor per channel: 16 KiB
constexpr int kRleMinRange = 512;         // positions per workgroup (1080p: 4050 waves, 8 steps each)
constexpr int64_t kRleTable = 1ll << 22;  // (channel, workgroup) entries at most

struct RlePlan {
  int64_t total;
  int range, groups;
  int64_t off_counts, off_base, bytes;  // scratch: transposed plane at 0, then the two int32 tables
};

RlePlan rle_plan(int oh, int ow, int channels) {
  RlePlan p;
  p.total = (int64_t)oh * ow;
  const int64_t max_groups = kRleTable / channels;  // >= 1024
  int64_t range = ceil_div(p.total, max_groups);
  if (range < kRleMinRange) range = kRleMinRange;
  p.range = (int)ceil_div(range, 64) * 64;
  p.groups = (int)ceil_div(p.total, p.range);
  p.off_counts = ceil_div(p.total * 2, 256) * 256;
  p.off_base = p.off_counts + ceil_div((int64_t)channels * p.groups * 4, 256) * 256;
  p.bytes = p.off_base + ceil_div((int64_t)channels * 4, 256) * 256;
  return p;
}

// dst[x][y] = src[y][x], 64 x 64 tiles
__global__ void __launch_bounds__(256) transpose_i16_kernel(const int16_t* __restrict__ src, int16_t* __restrict__ dst,
                                                            int oh, int ow) {
  __shared__ int16_t tile[64][65];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int x0 = blockIdx.x * 64, y0 = blockIdx.y * 64;
  for (int r = ty; r < 64; r += 4)
    if (y0 + r < oh && x0 + tx < ow) tile[r][tx] = src[(int64_t)(y0 + r) * ow + x0 + tx];
  __syncthreads();
  for (int r = ty; r < 64; r += 4)
    if (x0 + r < ow && y0 + tx < oh) dst[(int64_t)(x0 + r) * oh + y0 + tx] = tile[tx][r];
}

// the object channel of a plane value: 0 ("no object") for the background and for anything outside the table
__device__ __forceinline__ int object_channel(int v, int channels) { return (v >= 1 && v < channels) ? v : 0; }

// counts[c][g] = boundaries of channel c in the range of workgroup g
__global__ void __launch_bounds__(64) rle_count_kernel(const int16_t* __restrict__ plane, int64_t total, int range,
                                                       int channels, int groups, int32_t* __restrict__ counts) {
  extern __shared__ int32_t lds_count[];
  for (int c = threadIdx.x; c < channels; c += 64) lds_count[c] = 0;
  __syncthreads();
  const int64_t lo = (int64_t)blockIdx.x * range;
  const int64_t hi = lo + range < total ? lo + range : total;
  for (int64_t p = lo + threadIdx.x; p < hi; p += 64) {
    const int cur = object_channel(plane[p], channels);
    const int prev = p ? object_channel(plane[p - 1], channels) : 0;
    if (cur != prev) {
      if (prev) atomicAdd(&lds_count[prev], 1);
      if (cur) atomicAdd(&lds_count[cur], 1);
    }
  }
  __syncthreads();
  for (int c = threadIdx.x; c < channels; c += 64) counts[(int64_t)c * groups + blockIdx.x] = lds_count[c];
}

// one workgroup per channel: counts[c][:] -> its exclusive prefix sum, n[c] = the total (n[0] = 0: no runs are made
// for the background)
__global__ void __launch_bounds__(256) rle_scan_kernel(int32_t* __restrict__ counts, int groups, int32_t* __restrict__ n) {
  __shared__ int32_t part[256];
  const int c = blockIdx.x;
  int32_t* row = counts + (int64_t)c * groups;
  const int chunk = (groups + 255) / 256;
  const int lo = min(threadIdx.x * chunk, groups), hi = min(lo + chunk, groups);
  int32_t sum = 0;
  for (int g = lo; g < hi; ++g) sum += row[g];
  part[threadIdx.x] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    int32_t run = 0;
    for (int t = 0; t < 256; ++t) {
      const int32_t v = part[t];
      part[t] = run;
      run += v;
    }
    n[c] = c ? run : 0;
  }
  __syncthreads();
  int32_t run = part[threadIdx.x];
  for (int g = lo; g < hi; ++g) {
    const int32_t v = row[g];
    row[g] = run;
    run += v;
  }
}

// base[c] = n[1] + ... + n[c-1]: where the boundaries of channel c start in `bounds`
__global__ void rle_base_kernel(const int32_t* __restrict__ n, int channels, int32_t* __restrict__ base) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    int32_t run = 0;
    for (int c = 0; c < channels; ++c) {
      base[c] = run;
      run += c ? n[c] : 0;
    }
  }
}

__global__ void __launch_bounds__(64) rle_write_kernel(const int16_t* __restrict__ plane, int64_t total, int range,
                                                       int channels, int groups, const int32_t* __restrict__ counts,
                                                       const int32_t* __restrict__ base, int32_t* __restrict__ bounds,
                                                       int64_t capacity) {
  extern __shared__ int32_t cursor[];
  for (int c = threadIdx.x; c < channels; c += 64) cursor[c] = base[c] + counts[(int64_t)c * groups + blockIdx.x];
  __syncthreads();
  const int lane = threadIdx.x;
  const uint64_t below = (1ull << lane) - 1;
  const int64_t lo = (int64_t)blockIdx.x * range;
  const int64_t hi = lo + range < total ? lo + range : total;
  for (int64_t p0 = lo; p0 < hi; p0 += 64) {  // (uniform: the whole wave takes every step)
    const int64_t p = p0 + lane;
    int k0 = 0, k1 = 0;  // the channel whose run ends before p, the channel whose run starts at p
    if (p < hi) {
      const int cur = object_channel(plane[p], channels);
      const int prev = p ? object_channel(plane[p - 1], channels) : 0;
      if (cur != prev) {
        k0 = prev;
        k1 = cur;
      }
    }
    uint64_t pending = __ballot(k0 | k1);
    while (pending) {  // one turn per distinct channel with a boundary in this step (typically 1 to 3)
      const int leader = __ffsll((unsigned long long)pending) - 1;
      const int c = __shfl(k0 ? k0 : k1, leader);
      const bool mine = k0 == c || k1 == c;  // (k0 != k1 wherever either is set)
      const uint64_t m = __ballot(mine);
      const int first = cursor[c];
      if (mine) {
        const int64_t at = (int64_t)first + __popcll(m & below);
        if (at < capacity) bounds[at] = (int32_t)p;  // (the host has checked the capacity against n)
        if (k0 == c) k0 = 0; else k1 = 0;
      }
      if (lane == leader) cursor[c] = first + __popcll(m);
      __syncthreads();  // (one wave: orders the cursor update before the next turn's read)
      pending = __ballot(k0 | k1);
    }
  }
}

}  // namespace
}  // namespace deva

using namespace deva;

extern "C" int deva_frame_result(const float* prob, int channels, int height, int width, int out_height, int out_width,
                                 const int64_t* lut, int n_lut, const uint8_t* color_lut, const uint8_t* image,
                                 int16_t* index, int64_t* labels, int32_t* stats, uint8_t* color, uint8_t* gray,
                                 uint8_t* blend, void* stream) {
  DEVA_REQUIRE(prob && channels > 0 && height > 0 && width > 0 && out_height > 0 && out_width > 0,
               "deva_frame_result: bad args");
  DEVA_REQUIRE(index || labels || stats || color || gray || blend, "deva_frame_result: no output requested");
  DEVA_REQUIRE(!lut || n_lut > 0, "deva_frame_result: empty table");
  DEVA_REQUIRE(!index || channels <= 32767, "deva_frame_result: the int16 index plane holds at most 32767 channels (got %d)",
               channels);
  DEVA_REQUIRE(!(color || blend) || color_lut, "deva_frame_result: color / blend need a color table");
  DEVA_REQUIRE(!blend || image, "deva_frame_result: blend needs the image");
  DEVA_REQUIRE((int64_t)out_height * out_width < (1ll << 31) && (int64_t)height * width < (1ll << 31),
               "deva_frame_result: frame of 2^31 pixels or more");
  FrameArgs a = {prob, channels, height, width, out_height, out_width,
                 (float)height / (float)out_height, (float)width / (float)out_width,
                 lut, n_lut, color_lut, image, index, labels, stats, color, gray, blend};
  hipStream_t s = (hipStream_t)stream;
  if (stats)
    hipLaunchKernelGGL(stats_init_kernel, dim3((unsigned)ceil_div((int64_t)channels * 5, 256)), dim3(256), 0, s, stats,
                       channels);
  const bool vec = out_width % 4 == 0 && aligned(index, 8) && aligned(labels, 16) && aligned(gray, 4) &&
                   aligned(color, 4) && aligned(blend, 4) && (!blend || aligned(image, 4));
  const int mode = !stats ? STATS_NONE : (channels <= kStatsLdsChannels ? STATS_LDS : STATS_GLOBAL);
  const size_t smem = mode == STATS_LDS ? sizeof(int32_t) * 5 * (size_t)channels : 0;
  int64_t blocks = ceil_div((int64_t)out_height * ((out_width + 3) / 4), 256);
  if (blocks > 4096) blocks = 4096;
  const dim3 g((unsigned)blocks), t(256);
#define DEVA_FRAME_LAUNCH(V, M) hipLaunchKernelGGL((frame_result_kernel<V, M>), g, t, smem, s, a)
  if (vec) {
    if (mode == STATS_NONE) DEVA_FRAME_LAUNCH(true, STATS_NONE);
    else if (mode == STATS_LDS) DEVA_FRAME_LAUNCH(true, STATS_LDS);
    else DEVA_FRAME_LAUNCH(true, STATS_GLOBAL);
  } else {
    if (mode == STATS_NONE) DEVA_FRAME_LAUNCH(false, STATS_NONE);
    else if (mode == STATS_LDS) DEVA_FRAME_LAUNCH(false, STATS_LDS);
    else DEVA_FRAME_LAUNCH(false, STATS_GLOBAL);
  }
#undef DEVA_FRAME_LAUNCH
  return check_launch("deva_frame_result");
}

extern "C" int64_t deva_mask_rle_scratch(int out_height, int out_width, int channels) {
  if (out_height <= 0 || out_width <= 0 || channels <= 0 || channels > kRleMaxChannels ||
      (int64_t)out_height * out_width >= (1ll << 30))
    return -1;
  return rle_plan(out_height, out_width, channels).bytes;
}

static int rle_args(const char* what, int oh, int ow, int channels, const void* scratch, int64_t scratch_bytes) {
  DEVA_REQUIRE(oh > 0 && ow > 0 && channels > 0 && scratch, "%s: bad args", what);
  DEVA_REQUIRE(channels <= kRleMaxChannels, "%s: at most %d channels (got %d)", what, kRleMaxChannels, channels);
  DEVA_REQUIRE((int64_t)oh * ow < (1ll << 30), "%s: frame of 2^30 pixels or more", what);
  DEVA_REQUIRE(aligned(scratch, 4) && scratch_bytes >= rle_plan(oh, ow, channels).bytes,
               "%s: scratch of %lld bytes, deva_mask_rle_scratch asks for %lld", what, (long long)scratch_bytes,
               (long long)rle_plan(oh, ow, channels).bytes);
  return 0;
}

extern "C" int deva_mask_rle_count(const int16_t* index, int out_height, int out_width, int channels, void* scratch,
                                   int64_t scratch_bytes, int32_t* n, void* stream) {
  DEVA_REQUIRE(index && n, "deva_mask_rle_count: bad args");
  if (int e = rle_args("deva_mask_rle_count", out_height, out_width, channels, scratch, scratch_bytes)) return e;
  const RlePlan p = rle_plan(out_height, out_width, channels);
  int16_t* plane = static_cast<int16_t*>(scratch);
  int32_t* counts = reinterpret_cast<int32_t*>(static_cast<char*>(scratch) + p.off_counts);
  int32_t* base = reinterpret_cast<int32_t*>(static_cast<char*>(scratch) + p.off_base);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(transpose_i16_kernel, dim3((unsigned)ceil_div(out_width, 64), (unsigned)ceil_div(out_height, 64)),
                     dim3(256), 0, s, index, plane, out_height, out_width);
  hipLaunchKernelGGL(rle_count_kernel, dim3((unsigned)p.groups), dim3(64), sizeof(int32_t) * (size_t)channels, s, plane,
                     p.total, p.range, channels, p.groups, counts);
  hipLaunchKernelGGL(rle_scan_kernel, dim3((unsigned)channels), dim3(256), 0, s, counts, p.groups, n);
  hipLaunchKernelGGL(rle_base_kernel, dim3(1), dim3(64), 0, s, n, channels, base);
  return check_launch("deva_mask_rle_count");
}

extern "C" int deva_mask_rle_write(int out_height, int out_width, int channels, const void* scratch,
                                   int64_t scratch_bytes, const int32_t* n_host, int32_t* bounds, int64_t capacity,
                                   void* stream) {
  DEVA_REQUIRE(n_host && capacity >= 0, "deva_mask_rle_write: bad args");
  if (int e = rle_args("deva_mask_rle_write", out_height, out_width, channels, scratch, scratch_bytes)) return e;
  int64_t need = 0;
  for (int c = 1; c < channels; ++c) {
    DEVA_REQUIRE(n_host[c] >= 0, "deva_mask_rle_write: negative count for channel %d", c);
    need += n_host[c];
  }
  DEVA_REQUIRE(need <= capacity, "deva_mask_rle_write: %lld boundaries do not fit a capacity of %lld", (long long)need,
               (long long)capacity);
  if (need == 0) return 0;
  DEVA_REQUIRE(bounds, "deva_mask_rle_write: null output");
  const RlePlan p = rle_plan(out_height, out_width, channels);
  const int16_t* plane = static_cast<const int16_t*>(scratch);
  const int32_t* counts = reinterpret_cast<const int32_t*>(static_cast<const char*>(scratch) + p.off_counts);
  const int32_t* base = reinterpret_cast<const int32_t*>(static_cast<const char*>(scratch) + p.off_base);
  hipLaunchKernelGGL(rle_write_kernel, dim3((unsigned)p.groups), dim3(64), sizeof(int32_t) * (size_t)channels,
                     (hipStream_t)stream, plane, p.total, p.range, channels, p.groups, counts, base, bounds, capacity);
  return check_launch("deva_mask_rle_write");
}
