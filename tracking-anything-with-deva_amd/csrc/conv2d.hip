// deva_conv2d: validate and plan (conv_plan.cpp, where every choice is made), then launch what the plan says -- once, or
// once per sub-batch where a source spans 2^29 floats.
#include "conv_args.h"

#include <algorithm>
#include <cstdlib>

namespace deva {
namespace {

int launch_fp32(const ConvArgs& a, const deva_conv_launch& l, hipStream_t st) {
  if (l.family == DEVA_CONV_IGEMM) return launch_conv_igemm(a, l, st);
  return l.persistent ? launch_conv_q4_gated(a, l, st) : launch_conv_q4(a, l, st);
}

int launch_plan(ConvArgs a, const deva_conv_desc* d, const deva_conv_plan& plan, hipStream_t st) {
  const deva_conv_launch& l = plan.first;
  switch (l.family) {
    case DEVA_CONV_COUT1_TABLE: return launch_conv_cout1(a, l, st);
    case DEVA_CONV_COUT1_ROWS: return launch_conv3x3_cout1_rows(a, l, st);
    case DEVA_CONV_WINO: return launch_conv_wino(a, d->weight_wino, l, st);
    case DEVA_CONV_F16: return launch_conv_f16(a, l, st);
    case DEVA_CONV_Q4:
    case DEVA_CONV_IGEMM: return launch_fp32(a, l, st);
    case DEVA_CONV_SPLIT: break;
    default: set_error("deva_conv2d: the plan names no kernel family (%d)", l.family); return 2;
  }
  // split: the fp32 kernels run behind it, gated on the flag it raises for inputs beyond the fp16 range
  if (const int rc = launch_conv_f16(a, l, st)) return rc;
#ifdef DEVA_CONV_PROBES  // `make PROBES=1`: what the gated launch costs (tools/convlab)
  {
    static const bool nogate = getenv("DEVA_SPLIT_NOGATE") != nullptr;
    if (nogate) return 0;
  }
#endif
  a.gate = a.flag;
  conv_args_fp32(a);
  return launch_fp32(a, plan.rerun, st);
}

}  // namespace
}  // namespace deva

extern "C" int deva_conv2d(const deva_conv_desc* d, void* stream) {
  using namespace deva;
  hipStream_t st = (hipStream_t)stream;
  ConvArgs a;
  deva_conv_plan plan;
  if (const int rc = conv_plan(d, &a, &plan)) return rc;
  if (const int rc = launch_plan(a, d, plan, st)) return rc;
  const int64_t per = plan.sub_batch;
  for (int64_t b0 = per; b0 < d->batch; b0 += per) {  // (the tail may be shorter: planned with its own batch)
    const deva_conv_desc sub = conv_desc_slice(*d, b0, std::min<int64_t>(per, d->batch - b0));
    if (const int rc = conv_plan(&sub, &a, &plan)) return rc;
    if (const int rc = launch_plan(a, &sub, plan, st)) return rc;
  }
  return 0;
}
