// The proposal filter and the best-mask choice from a segmenter's low-resolution logits (contract: include/deva_lowres.h,
// rules L1-L7).  The frame-sized fp32 planes of `postprocess_masks` are never written: every pass forms the values it
// needs from the low-resolution plane.
//
//   upsample  grid (band, plane): L3 materialised (the tests' and the benchmark's yardstick, and the unfused route)
//   per batch of the filter (rules 1-4 of deva_proposal_batch on the values of L3)
//   stats     grid (band, plane): hi, lo and the box, tallied and committed as prop_stats_kernel does (proposal_device.h).
//             A plane that is not live exits.
//   decide    prop_decide_kernel itself (proposal_device.h)
//   binarise  grid (band, plane): x > t_mask as bytes into the slot.  A plane without a slot exits.
//   select    grid (band, box): the box's choice from its scores (box_choice.h), then the chosen plane as bytes
//
// A band is `tile_rows` whole output rows (lowres_plan.cpp).  Every pass walks its band in 16-byte pieces of the OUTPUT's
// aligned space, one piece per lane and step: element e sits at the 16-byte boundary below the plane plus e elements, a
// piece with all its elements inside the plane is one 16-byte store, the ragged first and last piece of a plane go
// element by element.  A piece belongs to the band that holds its first pixel, so it may reach into the rows below the
// band; the plan's `cover_rows` says how far.
//
// Two launch shapes, chosen by the plan: on the tile path the workgroup first copies the rows of `low` its band needs
// into LDS, forms the band's rows of `mid` from them in LDS (four taps each), and every output pixel takes four LDS
// taps; on the point path every output pixel forms its four values of `mid` from sixteen taps of `low` in global memory
// (the plane is 256 KB: it stays in L2).  lowres_axis and lowres_lerp are the only arithmetic of L1 / L2 in the file, and
// both paths and all passes call them: that is why fused equals unfused bit for bit.
#include <hip/hip_runtime.h>

#include "../box_choice.h"
#include "../proposal_device.h"
#include "lowres_plan.h"

namespace deva_lowres {
namespace {

using deva::box_choice;
using deva::kPropBatch;
using deva::prop_commit;
using deva::prop_decide_kernel;
using deva::prop_live;
using deva::prop_take;
using deva::PropArgs;
using deva::PropTally;

struct Geo {
  int lh, lw, ih, iw, oh, ow;
  float s1y, s1x, s2y, s2x;  // L1's scales of stage 1 (low -> M) and stage 2 (crop -> out)
  int tile_rows, cover_rows, mid_rows, low_rows;
};

// ------------------------------------------------------------------------------------------ L1, L2
struct Axis {
  int i0, i1;
  float l0, l1;
};

__device__ __forceinline__ Axis lowres_axis(float scale, int d, int n_in) {
#pragma clang fp contract(off)
  const float s = fmaxf(scale * ((float)d + 0.5f) - 0.5f, 0.0f);
  Axis a;
  a.i0 = min((int)s, n_in - 1);
  a.i1 = min(a.i0 + 1, n_in - 1);
  a.l1 = s - (float)a.i0;
  a.l0 = 1.0f - a.l1;
  return a;
}

__device__ __forceinline__ float lowres_lerp(const Axis& y, const Axis& x, float a, float b, float c, float d) {
#pragma clang fp contract(off)
  return y.l0 * (x.l0 * a + x.l1 * b) + y.l1 * (x.l0 * c + x.l1 * d);
}

// ------------------------------------------------------------------------------------------ where a value of `mid` comes from
// point path: mid[my][mx] from four taps of the plane in global memory
struct PointSource {
  const float* low;
  __device__ __forceinline__ float mid(const Geo& g, int my, int mx) const {
    const Axis y = lowres_axis(g.s1y, my, g.lh), x = lowres_axis(g.s1x, mx, g.lw);
    const float* r0 = low + y.i0 * g.lw;
    const float* r1 = low + y.i1 * g.lw;
    return lowres_lerp(y, x, r0[x.i0], r0[x.i1], r1[x.i0], r1[x.i1]);
  }
};

// tile path: rows my_lo .. of mid[:, :IW] in LDS
struct TileSource {
  const float* rows;
  int my_lo;
  __device__ __forceinline__ float mid(const Geo& g, int my, int mx) const { return rows[(my - my_lo) * g.iw + mx]; }
};

// one output pixel of L3: row axis `y` (of stage 2), column x
template <class Source>
__device__ __forceinline__ float lowres_value(const Geo& g, const Source& src, const Axis& y, int x) {
  const Axis ax = lowres_axis(g.s2x, x, g.iw);
  return lowres_lerp(y, ax, src.mid(g, y.i0, ax.i0), src.mid(g, y.i0, ax.i1), src.mid(g, y.i1, ax.i0), src.mid(g, y.i1, ax.i1));
}

// the band's rows of `low`, then of `mid`, into LDS: mid rows first ([mid_rows][IW]), low rows behind ([low_rows][LW]).
// Output rows r0 .. r0 + cover_rows - 1 read mid rows my_lo .. my_hi (L1's index is monotone in d); the plan's mid_rows
// and low_rows bound both counts, and the copies are cut to them so that nothing is written past the patch.
__device__ __forceinline__ TileSource tile_fill(const Geo& g, const float* low, int r0, float* lds) {
  const int t = threadIdx.x;
  const int r_last = min(r0 + g.cover_rows, g.oh) - 1;
  const int my_lo = lowres_axis(g.s2y, r0, g.ih).i0;
  const int n_mid = min(lowres_axis(g.s2y, r_last, g.ih).i1 - my_lo + 1, g.mid_rows);
  const int ly_lo = lowres_axis(g.s1y, my_lo, g.lh).i0;
  const int n_low = min(lowres_axis(g.s1y, my_lo + n_mid - 1, g.lh).i1 - ly_lo + 1, g.low_rows);
  float* patch = lds + g.mid_rows * g.iw;
  const float* from = low + ly_lo * g.lw;
  for (int i = t; i < n_low * g.lw; i += kBlock) patch[i] = from[i];
  __syncthreads();
  for (int r = 0; r < n_mid; ++r) {
    const Axis y = lowres_axis(g.s1y, my_lo + r, g.lh);
    const float* p0 = patch + (y.i0 - ly_lo) * g.lw;
    const float* p1 = patch + (y.i1 - ly_lo) * g.lw;
    for (int mx = t; mx < g.iw; mx += kBlock) {
      const Axis x = lowres_axis(g.s1x, mx, g.lw);
      lds[r * g.iw + mx] = lowres_lerp(y, x, p0[x.i0], p0[x.i1], p1[x.i0], p1[x.i1]);
    }
  }
  __syncthreads();
  return {lds, my_lo};
}

// ------------------------------------------------------------------------------------------ where a value goes
// fp32 plane: pieces of 4
struct FloatSink {
  static constexpr int kElems = 4;
  float* o;
  float f[4];
  __device__ __forceinline__ void begin() {}
  template <int J>
  __device__ __forceinline__ void put(float v, int i, int x) {
    f[J] = v;
  }
  __device__ __forceinline__ void flush(int p, int j0, int j1, bool full) {
    if (full) {
      *reinterpret_cast<float4*>(o + p) = make_float4(f[0], f[1], f[2], f[3]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (j >= j0 && j < j1) o[p + j] = f[j];
    }
  }
};

// byte plane x > t: pieces of 16
struct ByteSink {
  static constexpr int kElems = kPiece;
  uint8_t* o;
  float t_mask;
  uint32_t word[4];
  __device__ __forceinline__ void begin() { word[0] = word[1] = word[2] = word[3] = 0; }
  template <int J>
  __device__ __forceinline__ void put(float v, int i, int x) {
    word[J >> 2] |= (uint32_t)(v > t_mask) << (8 * (J & 3));
  }
  __device__ __forceinline__ void flush(int p, int j0, int j1, bool full) {
    if (full) {
      *reinterpret_cast<uint4*>(o + p) = make_uint4(word[0], word[1], word[2], word[3]);
    } else {
#pragma unroll
      for (int j = 0; j < kPiece; ++j)
        if (j >= j0 && j < j1) o[p + j] = (uint8_t)(word[j >> 2] >> (8 * (j & 3)));
    }
  }
};

// the tally of rules 2 and 4: nothing is stored
struct TallySink {
  static constexpr int kElems = kPiece;
  const PropArgs& a;
  PropTally s;
  __device__ __forceinline__ void begin() {}
  template <int J>
  __device__ __forceinline__ void put(float v, int i, int x) {
    prop_take(a, v, i, x, s);
  }
  __device__ __forceinline__ void flush(int, int, int, bool) {}
};

template <int J, int N, class Source, class Sink>
struct Steps {
  static __device__ __forceinline__ void run(const Geo& g, const Source& src, Sink& sink, int p, int j0, int j1, int& x, int& y, Axis& ay) {
    if (J >= j0 && J < j1) {
      sink.template put<J>(lowres_value(g, src, ay, x), p + J, x);
      if (++x == g.ow) x = 0, ++y, ay = lowres_axis(g.s2y, y, g.ih);
    }
    Steps<J + 1, N, Source, Sink>::run(g, src, sink, p, j0, j1, x, y, ay);
  }
};
template <int N, class Source, class Sink>
struct Steps<N, N, Source, Sink> {
  static __device__ __forceinline__ void run(const Geo&, const Source&, Sink&, int, int, int, int&, int&, Axis&) {}
};

// the pieces of band `band`: those whose first pixel lies in its rows.  shift: elements between the 16-byte boundary below
// the output plane and the plane (0 when nothing is stored).
template <class Source, class Sink>
__device__ __forceinline__ void band_walk(const Geo& g, int band, int shift, const Source& src, Sink& sink) {
  constexpr int E = Sink::kElems;
  const int hw = g.oh * g.ow;
  const int p_lo = band * g.tile_rows * g.ow;
  const int p_hi = min((band + 1) * g.tile_rows, g.oh) * g.ow;
  const int g_lo = p_lo == 0 ? 0 : (p_lo + shift + E - 1) / E;
  const int g_hi = (p_hi + shift + E - 1) / E;
  for (int gi = g_lo + (int)threadIdx.x; gi < g_hi; gi += kBlock) {
    const int p = gi * E - shift;  // (below 0 in the first piece of a misaligned plane)
    const int j0 = p < 0 ? -p : 0, j1 = min(E, hw - p);
    int y = (p + j0) / g.ow, x = (p + j0) - y * g.ow;
    Axis ay = lowres_axis(g.s2y, y, g.ih);
    sink.begin();
    Steps<0, E, Source, Sink>::run(g, src, sink, p, j0, j1, x, y, ay);
    sink.flush(p, j0, j1, j0 == 0 && j1 == E);
  }
}

template <bool kTile, class Sink>
__device__ __forceinline__ void band_run(const Geo& g, const float* low, int shift, Sink& sink, float* lds) {
  const int band = blockIdx.x;
  if (kTile) {
    const TileSource src = tile_fill(g, low, band * g.tile_rows, lds);
    band_walk(g, band, shift, src, sink);
  } else {
    const PointSource src = {low};
    band_walk(g, band, shift, src, sink);
  }
}

// ------------------------------------------------------------------------------------------ kernels
template <bool kTile>
__global__ void __launch_bounds__(kBlock) lowres_upsample_kernel(Geo g, const float* low, float* out) {
  extern __shared__ float lds[];
  const int k = blockIdx.y;
  float* o = out + (int64_t)k * g.oh * g.ow;
  FloatSink sink = {o, {}};
  band_run<kTile>(g, low + (int64_t)k * g.lh * g.lw, (int)(reinterpret_cast<uintptr_t>(o) >> 2 & 3), sink, lds);
}

template <bool kTile>
__global__ void __launch_bounds__(kBlock) lowres_stats_kernel(Geo g, const float* low, PropArgs a) {
  extern __shared__ float lds[];
  __shared__ int32_t red[4][6];
  const int k = blockIdx.y;
  if (!prop_live(a, k)) return;  // (never evaluated; the whole workgroup leaves)
  TallySink sink = {a, {0, 0, INT_MAX, -1, INT_MAX, -1}};
  band_run<kTile>(g, low + (int64_t)k * g.lh * g.lw, 0, sink, lds);
  prop_commit(a, k, sink.s, red);
}

template <bool kTile>
__global__ void __launch_bounds__(kBlock) lowres_binarize_kernel(Geo g, const float* low, PropArgs a) {
  extern __shared__ float lds[];
  const int k = blockIdx.y;
  const int32_t slot = a.slots[k];
  if (slot < 0 || slot >= a.capacity) return;
  uint8_t* o = a.arena + (int64_t)slot * a.hw;
  ByteSink sink = {o, a.t_mask, {}};
  band_run<kTile>(g, low + (int64_t)k * g.lh * g.lw, (int)(reinterpret_cast<uintptr_t>(o) & 15), sink, lds);
}

struct SelectArgs {
  const float* low;     // plane 0 of box 0 of this launch
  const float* scores;  // its first score, or NULL: plane 0 of every box
  int per_box;
  float t_mask;
  uint8_t* out;     // plane of box 0 of this launch
  int32_t* chosen;  // its choice, or NULL
};

template <bool kTile>
__global__ void __launch_bounds__(kBlock) lowres_select_kernel(Geo g, SelectArgs a) {
  extern __shared__ float lds[];
  const int b = blockIdx.y;
  const int pick = a.scores ? box_choice(a.scores + (int64_t)b * a.per_box, a.per_box) : 0;
  if (a.chosen && blockIdx.x == 0 && threadIdx.x == 0) a.chosen[b] = pick;
  uint8_t* o = a.out + (int64_t)b * g.oh * g.ow;
  ByteSink sink = {o, a.t_mask, {}};
  band_run<kTile>(g, a.low + ((int64_t)b * a.per_box + pick) * g.lh * g.lw, (int)(reinterpret_cast<uintptr_t>(o) & 15), sink, lds);
}

// ------------------------------------------------------------------------------------------ host
Geo geo_of(const struct deva_lowres_geometry& q, const struct deva_lowres_plan& p) {
  Geo g;
  g.lh = q.low_h, g.lw = q.low_w, g.ih = q.in_h, g.iw = q.in_w, g.oh = q.out_h, g.ow = q.out_w;
  g.s1y = axis_scale(q.low_h, q.model_size), g.s1x = axis_scale(q.low_w, q.model_size);
  g.s2y = axis_scale(q.in_h, q.out_h), g.s2x = axis_scale(q.in_w, q.out_w);
  g.tile_rows = p.tile_rows, g.cover_rows = p.cover_rows, g.mid_rows = p.mid_rows, g.low_rows = p.low_rows;
  return g;
}

int check_launch(const char* what) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("%s: %s", what, hipGetErrorString(e));
    return 1;
  }
  return 0;
}

template <class T>
T* at(void* scratch, int64_t offset) {
  return reinterpret_cast<T*>(static_cast<char*>(scratch) + offset);
}

// one of the two instances of a kernel template, by the plan's path
#define LOWRES_LAUNCH(kernel, plan, planes, stream, ...)                                                                    \
  do {                                                                                                                      \
    const dim3 grid((plan).grid_x, (unsigned)(planes));                                                                     \
    if ((plan).path == DEVA_LOWRES_PATH_TILE)                                                                               \
      hipLaunchKernelGGL((kernel<true>), grid, dim3(kBlock), (size_t)(plan).lds_bytes, stream, __VA_ARGS__);                \
    else                                                                                                                    \
      hipLaunchKernelGGL((kernel<false>), grid, dim3(kBlock), 0, stream, __VA_ARGS__);                                      \
  } while (0)

}  // namespace
}  // namespace deva_lowres

using namespace deva_lowres;

extern "C" int deva_lowres_upsample(const float* low, int batch, const struct deva_lowres_geometry* geometry, float* out, void* stream) {
  struct deva_lowres_plan plan;
  if (int e = upsample_check(low, batch, geometry, out, &plan)) return e;
  if (batch == 0) return 0;
  const Geo g = geo_of(*geometry, plan);
  const int64_t in_plane = (int64_t)g.lh * g.lw, out_plane = (int64_t)g.oh * g.ow;
  for (int first = 0; first < batch; first += kMaxGridY) {
    const int nb = batch - first < kMaxGridY ? batch - first : kMaxGridY;
    LOWRES_LAUNCH(lowres_upsample_kernel, plan, nb, (hipStream_t)stream, g, low + first * in_plane, out + first * out_plane);
  }
  return check_launch("deva_lowres_upsample");
}

extern "C" int deva_lowres_select(const float* low, const float* scores, int batch, int per_box, const struct deva_lowres_geometry* geometry,
                                  double mask_threshold, uint8_t* out, int32_t* chosen, void* stream) {
  struct deva_lowres_plan plan;
  if (int e = select_check(low, scores, batch, per_box, geometry, mask_threshold, out, chosen, &plan)) return e;
  if (batch == 0) return 0;
  const Geo g = geo_of(*geometry, plan);
  const int64_t in_plane = (int64_t)g.lh * g.lw, out_plane = (int64_t)g.oh * g.ow;
  SelectArgs a = {};
  a.per_box = per_box, a.t_mask = (float)mask_threshold;
  for (int first = 0; first < batch; first += kMaxGridY) {
    const int nb = batch - first < kMaxGridY ? batch - first : kMaxGridY;
    a.low = low + (int64_t)first * per_box * in_plane;
    a.scores = scores ? scores + (int64_t)first * per_box : nullptr;
    a.out = out + first * out_plane;
    a.chosen = chosen ? chosen + first : nullptr;
    LOWRES_LAUNCH(lowres_select_kernel, plan, nb, (hipStream_t)stream, g, a);
  }
  return check_launch("deva_lowres_select");
}

extern "C" int deva_lowres_proposal_batch(const float* low, const float* iou_preds, int batch, const struct deva_lowres_geometry* geometry,
                                          double pred_iou_thresh, double stability_score_thresh, double stability_score_offset,
                                          double mask_threshold, uint8_t* arena, int capacity, void* scratch, int64_t scratch_bytes,
                                          void* stream) {
  struct deva_lowres_plan plan;
  if (int e = proposal_check(low, iou_preds, batch, geometry, pred_iou_thresh, stability_score_thresh, stability_score_offset,
                             mask_threshold, arena, capacity, scratch, scratch_bytes, &plan))
    return e;
  const deva::ProposalPlan p = deva::proposal_plan(capacity);
  hipStream_t s = (hipStream_t)stream;
  const Geo g = geo_of(*geometry, plan);
  PropArgs a = {};  // as deva_proposal_batch fills it; `logits` stays null: there are none
  a.hw = g.oh * g.ow, a.w = g.ow;
  a.t_hi = (float)(mask_threshold + stability_score_offset);
  a.t_lo = (float)(mask_threshold - stability_score_offset);
  a.t_mask = (float)mask_threshold;
  a.t_iou = (float)pred_iou_thresh, a.t_stab = (float)stability_score_thresh;
  a.iou_on = pred_iou_thresh > 0.0, a.stab_on = stability_score_thresh > 0.0;
  a.arena = arena, a.capacity = capacity;
  a.stats = at<int32_t>(scratch, p.off_stats), a.slots = at<int32_t>(scratch, p.off_slots);
  a.count = at<int32_t>(scratch, p.off_count), a.table = at<int32_t>(scratch, p.off_table);
  const int64_t in_plane = (int64_t)g.lh * g.lw;
  for (int first = 0; first < batch; first += kPropBatch) {
    a.nb = batch - first < kPropBatch ? batch - first : kPropBatch;
    a.iou = iou_preds + first;
    const float* from = low + first * in_plane;
    LOWRES_LAUNCH(lowres_stats_kernel, plan, a.nb, s, g, from, a);
    hipLaunchKernelGGL(prop_decide_kernel, dim3(1), dim3(kPropBatch), 0, s, a);
    LOWRES_LAUNCH(lowres_binarize_kernel, plan, a.nb, s, g, from, a);
  }
  return check_launch("deva_lowres_proposal_batch");
}
