// Which kernel a deva_conv2d call runs on: the ONE place where that is decided (conv_plan.cpp).  Plain C++, no HIP:
// conv_plan() turns a descriptor into the kernels' argument block and a plan (include/deva_hip.h: deva_conv_plan --
// family, tile, K-slice groups, staging kind, split-K, grid); deva_conv2d (conv2d.hip) launches what the plan says and
// deva_conv2d_plan hands the same plan to callers, tests included.
#pragma once
#include <stdint.h>

#include "deva_hip.h"
#include "host_error.h"

namespace deva {

// argument block of the MFMA convolution kernels (conv_igemm.hip, conv_mfma.hip, conv_f16.hip) and the source of the
// other families' blocks
struct ConvArgs {
  const float* in0;
  const float* in1;
  int64_t bs0, bs1;  // batch strides (elements)
  int c0, c1, ctot;
  int H, W, OH, OW, OHW;
  int64_t HW;
  const float* w;
  const float* bias;
  int cout, cout_pad;
  int k_layout;
  int KH, KW, stride, pad;
  int K;        // KH*KW*ctot
  int n_total;  // batch*OH*OW
  int relu_in;
  const float* res;
  int64_t res_bs;
  int act;
  float* out;
  int vec_ok;        // inputs are guard-banded + 'same' stride-1 geometry: 4-pixel vector gathers allowed
  int vec_out;       // output and residual rows are 16-byte aligned, OHW % 4 == 0: output stage through LDS
  int tiles_n, tiles_m;
  int group_m;       // cout tiles per tile-order group (conv_epilogue.h: conv_tile_coords); <= 0: all of them
  int64_t ws_elems;
  int splits;        // split-K factor (gridDim.y); > 1 writes raw partial sums to ws
  int per_split;     // K steps per split
  float* ws;         // [splits][cout][n_total]
  int64_t in0_span, in1_span;  // elements from the first to one past the last element of each input
  const void* w16;   // conv_f16.hip: fp16 weights (DEVA_KLAYOUT_H8; hi / lo planes for the split kernels) or null
  int prec;          // conv_f16.hip: 1 = fp16 operands (amp), 2 = hi/lo split of both operands (fp32-accurate)
  float out_scale;   // split kernels: 2^-e of the weight scale, applied (exactly) to the accumulators
  int* flag;         // split kernels: set to 1 when an accumulator came out non-finite (an input beyond the fp16 range)
  const int* gate;   // non-null: the launch does its work only when *gate != 0 (the fp32 re-run behind a split launch)
  int ablate;        // `make PROBES=1` builds only (DEVA_SPLIT_ABLATE): timing runs with parts of the K loop switched off
};

// what the planner assumes of the kernels it steers (each .hip file asserts its own constants against these)
constexpr int kConvBK = 32;                     // K step of the fp32 MFMA kernels
constexpr int kWinoKC = 8;                      // conv_wino.hip: channels per K step
constexpr int kWinoBM = 64, kWinoBN = 64;       // conv_wino.hip: output channels x 2x2 tiles of a workgroup
constexpr int kPersistMaxWgs = 1024;  // workgroups of a gated re-run (a multiple of 8; 4 per CU fit: 35 KB of LDS each)

// cout tiles per tile-order group (conv_epilogue.h: conv_tile_coords).  With C workgroups of an XCD (resident at a time,
// ~48, or all the XCD ever gets on a small grid) covering g cout tiles x C/g pixel tiles, that XCD's L2 pulls g weight
// tiles + C/g activation tiles; a weight tile is taps * BM / (BN * stride^2) times the bytes of an activation tile, so
// g ~ sqrt(C / that ratio).
inline int conv_group_m(int taps, int stride, int bm, int bn, int64_t tiles) {
  const float ratio = (float)taps * bm / ((float)bn * stride * stride);
  const float c = (float)(tiles >= 8 * 48 ? 48 : (tiles + 7) / 8);
  int g = 1;
  while ((g + 1) * (g + 1) * ratio <= c * 1.5f) ++g;  // largest g with g^2 <= 1.5 C / ratio
  return g;
}

// Validates `d`, cuts the batch where a source spans 2^29 floats (plan->sub_batch), and for the first
// min(sub_batch, batch) images fills `a` (as the FIRST launch takes it) and `plan`.  0, or 2 with the error text set.
int conv_plan(const deva_conv_desc* d, ConvArgs* a, deva_conv_plan* plan);

// images [b0, b0 + batch) of a call as a call of their own
deva_conv_desc conv_desc_slice(const deva_conv_desc& d, int64_t b0, int64_t batch);

// the block one launch of the plan takes
inline ConvArgs conv_launch_args(const ConvArgs& a, const deva_conv_launch& l) {
  ConvArgs p = a;
  p.tiles_m = l.tiles_m;
  p.tiles_n = l.tiles_n;
  p.group_m = l.group_m;
  p.splits = l.splits;
  p.per_split = l.per_split;
  return p;
}

// from the block of an f16 / split launch to that of the fp32 kernels
inline void conv_args_fp32(ConvArgs& a) {
  a.w16 = nullptr;
  a.prec = 0;
  a.out_scale = 1.0f;
  a.flag = nullptr;
}

}  // namespace deva
