// Test-time ensemble output tail (evaluation/eval_vos.py:162-164,176-177,188-211 and
// scripts/merge_multi_scale.py:44-66): the reference runs the model once per (--size, --flip) variant, writes every
// run's resized probabilities to disk as uint8 (`--save_scores`) and merges the runs offline: float32 sum of the
// bytes, first-maximum argmax, tmp-id -> object-id table.  Here the K variants' probabilities stay on the device and
// one pass produces the merged labels; the uint8 volumes exist only when the caller asks for them.
//
// Bilinear arithmetic is that of index_mask_kernel (merge.hip): ATen's upsample_bilinear2d, align_corners=False,
// source coordinate scale*(dst+0.5)-0.5 clamped at 0, neighbour index clamped at the border, columns blended before
// rows.  At equal sizes the coordinate is the destination index itself and the far weights are exactly 0, so the blend
// returns the source value bit for bit.  A flipped variant is resized first and mirrored second (the reference's
// order): destination column x reads resized column ow-1-x.
#include "common.h"

namespace deva {
namespace {

constexpr int kMaxVariants = DEVA_ENSEMBLE_MAX_VARIANTS;

struct VariantArg {
  const float* src;
  int64_t plane_stride;
  int row_stride, h, w, flip;
  float scale_y, scale_x;
};

struct EnsembleArgs {
  VariantArg v[kMaxVariants];
  int channels, oh, ow;
  const int64_t* lut;
  int n_lut;
  int64_t* out;
};

// one axis of the resize: near / far source index of destination index d and the far weight
struct Tap {
  int i0, i1;
  float l1;
};

__device__ __forceinline__ Tap axis_tap(int d, int n_src, float scale) {
#pragma clang fp contract(off)
  const float s = fmaxf(__builtin_fmaf(scale, (float)d + 0.5f, -0.5f), 0.0f);
  Tap t;
  t.i0 = min((int)s, n_src - 1);
  t.i1 = t.i0 + (t.i0 < n_src - 1 ? 1 : 0);
  t.l1 = s - (float)t.i0;
  return t;
}

// the four source values of one output pixel as byte offsets into a channel plane, and the far column weight.  A
// plane is read through a buffer descriptor built from wave-uniform values (base of the channel, bytes of the plane):
// the per-pixel state is then 32-bit offsets instead of 64-bit addresses, which is what keeps eight variants' taps in
// registers at a useful occupancy, and the hardware range check comes on top of the index clamps.
struct Quad {
  uint32_t o00, o01, o10, o11;
  float lx1;
};

__device__ __forceinline__ Quad make_quad(const Tap& ty, const Tap& tx, int row_stride) {
  Quad q;
  q.o00 = (uint32_t)(ty.i0 * row_stride + tx.i0) * 4u;
  q.o01 = (uint32_t)(ty.i0 * row_stride + tx.i1) * 4u;
  q.o10 = (uint32_t)(ty.i1 * row_stride + tx.i0) * 4u;
  q.o11 = (uint32_t)(ty.i1 * row_stride + tx.i1) * 4u;
  q.lx1 = tx.l1;
  return q;
}

using Plane = __amdgpu_buffer_rsrc_t;

__device__ __forceinline__ Plane channel_plane(const VariantArg& v, int c) {
  const int bytes = ((v.h - 1) * v.row_stride + v.w) * 4;
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(v.src + (int64_t)c * v.plane_stride), 0, bytes, 0x00020000);
}

__device__ __forceinline__ float at(Plane plane, uint32_t offset) {
  return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(plane, (int)offset, 0, 0));
}

// resized value: lx0 * p[y0][x0] + lx1 * p[y0][x1] and the same of row y1, blended by ly0 / ly1.  The roundings are
// pinned to the ones index_mask_kernel evaluates as compiled (each row one product rounded and one fused multiply-add,
// the row blend two rounded products and an add), so that a lone unflipped variant gives deva_index_mask's labels bit
// for bit and the uint8 volumes and the merged labels agree with each other whatever the surrounding code is.
__device__ __forceinline__ float blend(Plane plane, const Quad& q, float ly1) {
#pragma clang fp contract(off)
  const float ly0 = 1.0f - ly1, lx1 = q.lx1, lx0 = 1.0f - lx1;
  const float top = __builtin_fmaf(lx1, at(plane, q.o01), lx0 * at(plane, q.o00));
  const float bot = __builtin_fmaf(lx0, at(plane, q.o10), lx1 * at(plane, q.o11));
  return ly0 * top + ly1 * bot;
}

// (prob * 255).astype(np.uint8) for probabilities in [0, 1]: truncation; values outside are clamped to the byte range
__device__ __forceinline__ int score_byte(float v) { return min(max((int)(255.0f * v), 0), 255); }

// `--save_scores`: out[c][y][x] = byte(resized[c][y][flip ? ow-1-x : x]); a thread owns 4 adjacent bytes of one row,
// computes their taps once and walks the channels blockIdx.y, blockIdx.y + gridDim.y, ... (uniform per workgroup)
template <bool PACK>
__global__ void __launch_bounds__(256) scores_u8_kernel(VariantArg v, int channels, int oh, int ow,
                                                        uint8_t* __restrict__ out) {
  const int gw = (ow + 3) >> 2;
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= (int64_t)oh * gw) return;
  const int y = (int)(i / gw);
  const int x = (int)(i - (int64_t)y * gw) << 2;
  const Tap ty = axis_tap(y, v.h, v.scale_y);
  Quad q[4];
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int xd = min(x + p, ow - 1);  // (bytes past the end of a row are not stored)
    q[p] = make_quad(ty, axis_tap(v.flip ? ow - 1 - xd : xd, v.w, v.scale_x), v.row_stride);
  }
  for (int c = blockIdx.y; c < channels; c += gridDim.y) {
    const Plane plane = channel_plane(v, c);
    uint8_t* dst = out + ((int64_t)c * oh + y) * ow + x;
    int b[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) b[p] = score_byte(blend(plane, q[p], ty.l1));
    if (PACK) {
      *reinterpret_cast<uint32_t*>(dst) = (uint32_t)b[0] | (uint32_t)b[1] << 8 | (uint32_t)b[2] << 16 | (uint32_t)b[3] << 24;
    } else {
#pragma unroll
      for (int p = 0; p < 4; ++p)
        if (x + p < ow) dst[p] = (uint8_t)b[p];
    }
  }
}

// merged labels: a thread owns 2 adjacent pixels of one output row (one 16-byte store).  The taps of every variant
// are computed once per pixel and kept in registers (K is a template parameter so that the loops unroll); channels
// run outermost with a running best, so their number is not bounded.
template <int K, bool QUANT, bool VEC>
__global__ void __launch_bounds__(256) ensemble_index_mask_kernel(EnsembleArgs a) {
  const int oh = a.oh, ow = a.ow;
  const int gw = (ow + 1) >> 1;
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= (int64_t)oh * gw) return;
  const int y = (int)(i / gw);
  const int x = (int)(i - (int64_t)y * gw) << 1;
  const bool two = VEC || x + 1 < ow;
  const int xb = two ? x + 1 : x;  // (the second pixel of an odd row's last thread repeats the first and is dropped)

  Quad qa[K], qb[K];
  float ly1[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const VariantArg& v = a.v[k];
    const Tap ty = axis_tap(y, v.h, v.scale_y);
    ly1[k] = ty.l1;
    qa[k] = make_quad(ty, axis_tap(v.flip ? ow - 1 - x : x, v.w, v.scale_x), v.row_stride);
    qb[k] = make_quad(ty, axis_tap(v.flip ? ow - 1 - xb : xb, v.w, v.scale_x), v.row_stride);
  }

  int best_a = 0, best_b = 0;
  if (QUANT) {
    int bva = -1, bvb = -1;  // (sums of bytes: 8 * 255 at most)
#pragma unroll 1
    for (int c = 0; c < a.channels; ++c) {
      int sa = 0, sb = 0;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const Plane plane = channel_plane(a.v[k], c);
        sa += score_byte(blend(plane, qa[k], ly1[k]));
        sb += score_byte(blend(plane, qb[k], ly1[k]));
      }
      if (sa > bva) {
        bva = sa;
        best_a = c;
      }
      if (sb > bvb) {
        bvb = sb;
        best_b = c;
      }
    }
  } else {
    float bva = -INFINITY, bvb = -INFINITY;
#pragma unroll 1
    for (int c = 0; c < a.channels; ++c) {
      float sa = 0.0f, sb = 0.0f;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const Plane plane = channel_plane(a.v[k], c);
        const float va = blend(plane, qa[k], ly1[k]);
        const float vb = blend(plane, qb[k], ly1[k]);
        sa = k == 0 ? va : sa + va;  // (variant order)
        sb = k == 0 ? vb : sb + vb;
      }
      if (sa > bva) {
        bva = sa;
        best_a = c;
      }
      if (sb > bvb) {
        bvb = sb;
        best_b = c;
      }
    }
  }
  const int64_t la = a.lut ? (best_a < a.n_lut ? a.lut[best_a] : 0) : (int64_t)best_a;
  const int64_t lb = a.lut ? (best_b < a.n_lut ? a.lut[best_b] : 0) : (int64_t)best_b;
  int64_t* dst = a.out + (int64_t)y * ow + x;
  if (VEC) {
    *reinterpret_cast<longlong2*>(dst) = make_longlong2(la, lb);
  } else {
    dst[0] = la;
    if (two) dst[1] = lb;
  }
}

// dst[r][x] = src[r][width-1-x] for elements of sizeof(T) bytes
template <typename T>
__global__ void __launch_bounds__(256) flip_w_kernel(const T* __restrict__ src, T* __restrict__ dst, int64_t rows,
                                                     int width) {
  const int64_t total = rows * width;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / width;
    const int x = (int)(i - r * width);
    dst[i] = src[r * width + (width - 1 - x)];
  }
}

struct Byte3 {
  uint8_t b[3];
};

int fill_variant(VariantArg& o, const deva_ensemble_variant& v, int oh, int ow) {
  DEVA_REQUIRE(v.src && v.channels > 0 && v.height > 0 && v.width > 0, "deva_ensemble: bad variant");
  DEVA_REQUIRE(v.row_stride >= v.width && v.plane_stride >= (int64_t)v.row_stride * (v.height - 1) + v.width,
               "deva_ensemble: variant strides overlap");
  DEVA_REQUIRE((int64_t)v.row_stride * v.height < (1ll << 29), "deva_ensemble: variant plane of 2 GiB or more");
  o.src = v.src;
  o.plane_stride = v.plane_stride;
  o.row_stride = (int)v.row_stride;
  o.h = v.height;
  o.w = v.width;
  o.flip = v.flip ? 1 : 0;
  o.scale_y = (float)v.height / (float)oh;
  o.scale_x = (float)v.width / (float)ow;
  return 0;
}

template <int K>
void launch_ensemble(const EnsembleArgs& a, bool quant, bool vec, unsigned blocks, hipStream_t stream) {
  if (quant) {
    if (vec)
      hipLaunchKernelGGL((ensemble_index_mask_kernel<K, true, true>), dim3(blocks), dim3(256), 0, stream, a);
    else
      hipLaunchKernelGGL((ensemble_index_mask_kernel<K, true, false>), dim3(blocks), dim3(256), 0, stream, a);
  } else {
    if (vec)
      hipLaunchKernelGGL((ensemble_index_mask_kernel<K, false, true>), dim3(blocks), dim3(256), 0, stream, a);
    else
      hipLaunchKernelGGL((ensemble_index_mask_kernel<K, false, false>), dim3(blocks), dim3(256), 0, stream, a);
  }
}

}  // namespace
}  // namespace deva

using namespace deva;

extern "C" int deva_scores_u8(const deva_ensemble_variant* variant, int out_height, int out_width, uint8_t* out,
                              void* stream) {
  DEVA_REQUIRE(variant && out && out_height > 0 && out_width > 0, "deva_scores_u8: bad args");
  VariantArg v;
  if (int e = fill_variant(v, *variant, out_height, out_width)) return e;
  const int64_t blocks = ceil_div((int64_t)out_height * ((out_width + 3) / 4), 256);
  DEVA_REQUIRE(blocks < (1ll << 31), "deva_scores_u8: output too large");
  const dim3 grid((unsigned)blocks, (unsigned)(variant->channels < 65535 ? variant->channels : 65535));
  if (out_width % 4 == 0 && aligned(out, 4))
    hipLaunchKernelGGL(scores_u8_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, v, variant->channels,
                       out_height, out_width, out);
  else
    hipLaunchKernelGGL(scores_u8_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, v, variant->channels,
                       out_height, out_width, out);
  return check_launch("deva_scores_u8");
}

extern "C" int deva_ensemble_index_mask(const deva_ensemble_variant* variants, int n_variants, int out_height,
                                        int out_width, int quantize, const int64_t* lut, int n_lut, int64_t* out,
                                        void* stream) {
  DEVA_REQUIRE(variants && out && out_height > 0 && out_width > 0, "deva_ensemble_index_mask: bad args");
  DEVA_REQUIRE(n_variants >= 1 && n_variants <= kMaxVariants, "deva_ensemble_index_mask: 1 to %d variants (got %d)",
               kMaxVariants, n_variants);
  DEVA_REQUIRE(!lut || n_lut > 0, "deva_ensemble_index_mask: empty table");
  EnsembleArgs a = {};
  for (int k = 0; k < n_variants; ++k) {
    DEVA_REQUIRE(variants[k].channels == variants[0].channels,
                 "deva_ensemble_index_mask: variant %d has %d channels, variant 0 has %d", k, variants[k].channels,
                 variants[0].channels);
    if (int e = fill_variant(a.v[k], variants[k], out_height, out_width)) return e;
  }
  a.channels = variants[0].channels;
  a.oh = out_height;
  a.ow = out_width;
  a.lut = lut;
  a.n_lut = n_lut;
  a.out = out;
  const int64_t blocks = ceil_div((int64_t)out_height * ((out_width + 1) / 2), 256);
  DEVA_REQUIRE(blocks < (1ll << 31), "deva_ensemble_index_mask: output too large");
  const bool vec = out_width % 2 == 0 && aligned(out, 16);
  const bool quant = quantize != 0;
  const unsigned b = (unsigned)blocks;
  hipStream_t s = (hipStream_t)stream;
  switch (n_variants) {
    case 1: launch_ensemble<1>(a, quant, vec, b, s); break;
    case 2: launch_ensemble<2>(a, quant, vec, b, s); break;
    case 3: launch_ensemble<3>(a, quant, vec, b, s); break;
    case 4: launch_ensemble<4>(a, quant, vec, b, s); break;
    case 5: launch_ensemble<5>(a, quant, vec, b, s); break;
    case 6: launch_ensemble<6>(a, quant, vec, b, s); break;
    case 7: launch_ensemble<7>(a, quant, vec, b, s); break;
    default: launch_ensemble<8>(a, quant, vec, b, s); break;
  }
  return check_launch("deva_ensemble_index_mask");
}

extern "C" int deva_flip_w(const void* src, void* dst, int64_t rows, int width, int elem_bytes, void* stream) {
  DEVA_REQUIRE(src && dst && src != dst && rows > 0 && width > 0, "deva_flip_w: bad args");
  DEVA_REQUIRE(elem_bytes == 1 || elem_bytes == 3 || elem_bytes == 4 || elem_bytes == 8,
               "deva_flip_w: elements of 1, 3, 4 or 8 bytes (got %d)", elem_bytes);
  int64_t blocks = ceil_div(rows * width, 256);
  if (blocks > 65535) blocks = 65535;
  const dim3 g((unsigned)blocks), t(256);
  hipStream_t s = (hipStream_t)stream;
  if (elem_bytes == 1)
    hipLaunchKernelGGL(flip_w_kernel<uint8_t>, g, t, 0, s, (const uint8_t*)src, (uint8_t*)dst, rows, width);
  else if (elem_bytes == 3)
    hipLaunchKernelGGL(flip_w_kernel<Byte3>, g, t, 0, s, (const Byte3*)src, (Byte3*)dst, rows, width);
  else if (elem_bytes == 4)
    hipLaunchKernelGGL(flip_w_kernel<uint32_t>, g, t, 0, s, (const uint32_t*)src, (uint32_t*)dst, rows, width);
  else
    hipLaunchKernelGGL(flip_w_kernel<uint64_t>, g, t, 0, s, (const uint64_t*)src, (uint64_t*)dst, rows, width);
  return check_launch("deva_flip_w");
}
