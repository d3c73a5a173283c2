// The launchers of the convolution translation units.  Each takes the kernels' argument block and ONE launch of a plan
// (conv_plan.h: where every choice is made) and turns it into a template instantiation; none of them decides anything,
// and a plan that names an instantiation this build does not hold is an error (2, with a message).
// conv2d.hip: deva_conv2d; conv_igemm.hip: the round-1 implicit-GEMM kernel and the split-K reduction; conv_mfma.hip: the
// lean-loop kernel generation; conv_f16.hip: f16 matrix pipes; conv_wino.hip: Winograd; conv_cout1.hip: single-channel heads.
#pragma once
#include "common.h"
#include "conv_plan.h"

namespace deva {

// conv_cout1.hip
struct Cout1Args {
  const float* in0;
  const float* in1;
  int64_t bs0, bs1;
  int c0, ctot;
  int H, W, OH, OW, OHW;
  int64_t HW;
  const float* w;
  const float* bias;
  int cout_pad, k_layout;
  int KH, KW, stride, pad;
  int n_total;
  int relu_in;
  const float* res;
  int64_t res_bs;
  int act;
  float* out;
};
int launch_conv_cout1(const ConvArgs& a, const deva_conv_launch& l, hipStream_t st);          // DEVA_CONV_COUT1_TABLE
int launch_conv3x3_cout1_rows(const ConvArgs& a, const deva_conv_launch& l, hipStream_t st);  // DEVA_CONV_COUT1_ROWS

// conv_igemm.hip: DEVA_CONV_IGEMM (+ the reduction behind a split-K launch)
int launch_conv_igemm(const ConvArgs& a, const deva_conv_launch& l, hipStream_t st);
// conv_igemm.hip: out = act(sum_s ws[s] + bias + residual) for a split-K launch (p.splits > 1)
int launch_splitk_reduce(const ConvArgs& p, hipStream_t st);
// conv_mfma.hip: DEVA_CONV_Q4, lean-loop kernels for weights in the k-quad layout (+ the reduction)
int launch_conv_q4(const ConvArgs& a, const deva_conv_launch& l, hipStream_t st);
// conv_mfma.hip: DEVA_CONV_Q4 with l.persistent, the gated fp32 re-run behind a split launch as a persistent kernel
int launch_conv_q4_gated(const ConvArgs& a, const deva_conv_launch& l, hipStream_t st);
// conv_wino.hip: DEVA_CONV_WINO, Winograd F(2x2, 3x3) on the fp32 matrix pipes; u: deva_conv_desc.weight_wino
int launch_conv_wino(const ConvArgs& a, const float* u, const deva_conv_launch& l, hipStream_t st);
// conv_f16.hip: DEVA_CONV_F16 (a.prec == 1) and DEVA_CONV_SPLIT (a.prec == 2) (+ the reduction)
int launch_conv_f16(const ConvArgs& a, const deva_conv_launch& l, hipStream_t st);

}  // namespace deva
