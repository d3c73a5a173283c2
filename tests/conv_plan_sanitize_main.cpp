// Stand-alone driver of the HIP-free convolution code (csrc/conv_plan.cpp, csrc/conv_pack.cpp) for a host build with
// -fsanitize=address,undefined (tests/test_plan_sanitize_cpu.py compiles and runs it): the planner over the product
// of its boundary values with made-up addresses, the packers into buffers of exactly the size they ask for.  Exit 0 = no
// sanitizer report and every invariant below held.
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "deva_hip.h"

namespace deva {
static char g_err[512];
void set_error(const char* fmt, ...) {  // (the library's lives in runtime.hip)
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
}  // namespace deva

static long g_plans = 0, g_refused = 0, g_failed = 0;

static const float* fake(uint64_t slot, uint64_t off = 0) { return reinterpret_cast<const float*>((slot << 40) + off); }

static void fail(const char* what, const deva_conv_desc& d, const deva_conv_plan& p) {
  if (++g_failed <= 10)
    fprintf(stderr, "INVARIANT %s: c0 %d c1 %d cout %d k %d s %d batch %d %dx%d layout %d amp %d -> family %d tile %dx%d wk %d splits %d x %d grid %u,%u block %u sub %d\n",
            what, d.c0, d.c1, d.cout, d.kh, d.stride, d.batch, d.height, d.width, d.k_layout, d.amp, p.first.family, p.first.bm, p.first.bn,
            p.first.wk, p.first.splits, p.first.per_split, p.first.grid_x, p.first.grid_y, p.first.block, p.sub_batch);
}

static void check_launch(const deva_conv_desc& d, const deva_conv_plan& p, const deva_conv_launch& l, int64_t n_total) {
  if (l.family <= DEVA_CONV_NONE || l.family > DEVA_CONV_IGEMM) return fail("family", d, p);
  if (l.grid_x < 1 || l.grid_y < 1 || (l.block != 256 && l.block != 512 && l.block != 1024)) fail("grid", d, p);
  if (l.splits < 1 || (int)l.grid_y != l.splits || l.per_split < 1) fail("splits", d, p);
  if (l.splits > 1) {
    const int bk = l.family == DEVA_CONV_F16 ? 64 : 32;
    const int64_t ksteps = ((int64_t)d.kh * d.kw * (d.c0 + d.c1) + bk - 1) / bk;
    if ((int64_t)l.splits * l.per_split < ksteps || (int64_t)(l.splits - 1) * l.per_split >= ksteps) fail("split cover", d, p);
    if (!d.workspace || (int64_t)l.splits * d.cout * n_total > d.workspace_elems) fail("workspace", d, p);
  }
  if (l.bm > 0 && l.family != DEVA_CONV_WINO && !l.persistent &&
      (int64_t)l.grid_x != ((int64_t)d.cout + l.bm - 1) / l.bm * ((n_total + l.bn - 1) / l.bn))
    fail("tiles", d, p);
}

static void plan_one(const deva_conv_desc& d) {
  deva_conv_plan p;
  memset(&p, 0xff, sizeof(p));
  const int rc = deva_conv2d_plan(&d, &p);
  ++g_plans;
  if (rc == 2) {  // a refusal leaves an all-zero plan
    ++g_refused;
    if (p.first.family != DEVA_CONV_NONE || p.rerun.family != DEVA_CONV_NONE || p.sub_batch != 0 || p.aliased != 0) fail("refused plan", d, p);
    return;
  }
  if (rc != 0) return fail("return code", d, p);
  if (p.sub_batch < 1 || p.sub_batch > d.batch) return fail("sub_batch", d, p);
  const int64_t oh = (d.height + 2 * d.pad - d.kh) / d.stride + 1, ow = (d.width + 2 * d.pad - d.kw) / d.stride + 1;
  const int64_t n_total = (int64_t)p.sub_batch * oh * ow;
  check_launch(d, p, p.first, n_total);
  if ((p.first.family == DEVA_CONV_SPLIT) != (p.rerun.family != DEVA_CONV_NONE)) fail("rerun", d, p);
  if (p.rerun.family != DEVA_CONV_NONE) check_launch(d, p, p.rerun, n_total);
}

static deva_conv_desc desc(int c0, int c1, int cout, int k, int stride, int batch, int h, int w) {
  deva_conv_desc d = {};
  d.in0 = fake(1);
  d.in1 = c1 ? fake(2) : nullptr;  // c1 = 0 goes with a null in1
  d.in0_batch_stride = (int64_t)c0 * h * w;
  d.in1_batch_stride = (int64_t)c1 * h * w;
  d.c0 = c0, d.c1 = c1, d.batch = batch, d.height = h, d.width = w;
  d.weight = fake(3);
  d.cout = cout, d.cout_pad = (cout + 31) / 32 * 32;
  d.kh = d.kw = k, d.stride = stride, d.pad = k / 2;
  d.out = const_cast<float*>(fake(4));
  d.split_flag = reinterpret_cast<int32_t*>(const_cast<float*>(fake(8)));
  return d;
}

static void walk_planner() {
  const int couts[] = {1, 32, 33, 127, 128, 256}, c0s[] = {32, 33, 64, 480, 512, 992, 1024, 7168, 7169}, c1s[] = {0, 1, 32};
  const int ks[] = {1, 3, 7}, strides[] = {1, 2}, batches[] = {1, 3};
  const int maps[][2] = {{8, 8}, {64, 64}, {8, 1008}, {8, 1016}, {128, 191}, {128, 192}, {128, 256}, {128, 257}, {4095, 4}, {4096, 4}, {129, 127}, {128, 128},
                         {318, 128}, {320, 128}, {8, 1664}, {8, 1672}, {8, 2040}, {8, 2048}, {8, 1528}, {8, 1536}};
  for (int cout : couts) for (int c0 : c0s) for (int c1 : c1s) for (int k : ks) for (int stride : strides)
    for (int batch : batches) for (const auto& m : maps) {
      deva_conv_desc d = desc(c0, c1, cout, k, stride, batch, m[0], m[1]);
      const int chunk = (k > 1 && (c0 + c1) % 32 == 0) ? DEVA_KLAYOUT_CHUNK32 : DEVA_KLAYOUT_TAP_MAJOR;
      for (int q4 = 0; q4 < 2; ++q4) for (int amp = 0; amp < 3; ++amp) for (int opt = 0; opt < 8; ++opt) {
        d.k_layout = chunk | (q4 ? DEVA_KLAYOUT_Q4 : 0);
        d.amp = amp;
        d.weight_f16 = amp ? fake(7) : nullptr;
        d.weight_wino = (opt & 1) ? fake(9) : nullptr;
        d.in_guard_elems = (opt & 2) ? 8192 : 0;
        d.workspace = (opt & 4) ? const_cast<float*>(fake(6)) : nullptr;
        d.workspace_elems = (opt & 4) ? (16ll << 20) : 0;
        d.residual = (opt & 1) ? fake(5, (opt & 2) ? 4 : 0) : nullptr;  // aligned and 4 bytes off
        d.residual_batch_stride = (int64_t)cout * ((m[0] + 2 * d.pad - k) / stride + 1) * ((m[1] + 2 * d.pad - k) / stride + 1);
        plan_one(d);
      }
    }
  // batch strides of 0 and of 2^29 - 1, sources around the 2^29-float limit, batch * OHW just under 2^31, overlapping operands
  for (int cout : {1, 64, 256}) for (int k : {1, 3}) for (int64_t s0 : {0ll, (1ll << 29) - 1, 1ll << 29}) for (int64_t s1 : {0ll, (1ll << 29) - 1})
    for (int batch : {1, 2, 5, 81, 2047}) for (int c1 : {0, 512}) {
      deva_conv_desc d = desc(256, c1, cout, k, 1, batch, 1024, 1024);  // batch 2047: 2^31 - 2^20 pixels
      d.k_layout = (k > 1 ? DEVA_KLAYOUT_CHUNK32 : DEVA_KLAYOUT_TAP_MAJOR) | (cout > 1 ? DEVA_KLAYOUT_Q4 : 0);
      d.in0_batch_stride = s0, d.in1_batch_stride = s1;
      d.in_guard_elems = 8192;
      d.workspace = const_cast<float*>(fake(6)), d.workspace_elems = 16ll << 20;
      for (int amp : {0, 2}) {
        d.amp = amp, d.weight_f16 = amp ? fake(7) : nullptr;
        plan_one(d);
        d.out = const_cast<float*>(fake(1, 64));  // on top of in0
        plan_one(d);
        d.out = const_cast<float*>(fake(4));
      }
      d.height = 2048, d.width = 1024;  // one image of 2^21 pixels x 256 channels = 2^29 floats: refused on k-quad weights
      plan_one(d);
    }
}

// every weight is non-zero, so a packed buffer must hold exactly cout * cin * taps non-zero elements (planes: per plane, hi)
template <typename T>
static long nonzero(const std::vector<T>& v) {
  long n = 0;
  for (const T& x : v) n += x != 0;
  return n;
}

static void walk_packers() {
  const int layers[][3] = {{33, 1, 1}, {32, 3, 1}, {64, 3, 1}, {33, 1, 33}, {32, 3, 33}, {64, 3, 33}, {64, 1, 33}};  // cin, k, cout
  for (const auto& l : layers) {
    const int cin = l[0], k = l[1], cout = l[2], taps = k * k;
    std::vector<float> w((size_t)cout * cin * taps);
    for (size_t i = 0; i < w.size(); ++i) w[i] = 0.5f + (float)(i % 97) * 0.03125f;
    for (int q4 = 0; q4 < 2; ++q4) {
      int layout = -1, cpad = -1;
      const int64_t n = deva_conv_pack(w.data(), nullptr, cout, cin, k, k, q4, &layout, &cpad);
      std::vector<float> out((size_t)(n > 0 ? n : 0));
      if (n <= 0 || deva_conv_pack(w.data(), out.data(), cout, cin, k, k, q4, &layout, &cpad) != n || nonzero(out) != (long)w.size()) {
        fprintf(stderr, "deva_conv_pack cin %d k %d cout %d q4 %d\n", cin, k, cout, q4);
        ++g_failed;
      }
    }
    {
      int cpad = -1;
      const int64_t n = deva_conv_pack_f16(w.data(), nullptr, cout, cin, k, k, &cpad);
      if ((n > 0) != (cin % 64 == 0)) ++g_failed;
      if (n > 0) {
        std::vector<uint16_t> out((size_t)n);
        if (deva_conv_pack_f16(w.data(), out.data(), cout, cin, k, k, &cpad) != n || nonzero(out) != (long)w.size()) ++g_failed;
      }
    }
    {
      int cpad = -1, e = -999;
      const int64_t n = deva_conv_pack_split(w.data(), nullptr, cout, cin, k, k, &cpad, &e);
      if ((n > 0) != (cin % 32 == 0 || taps == 1)) ++g_failed;
      if (n > 0) {
        std::vector<uint16_t> out((size_t)n);
        if (deva_conv_pack_split(w.data(), out.data(), cout, cin, k, k, &cpad, &e) != n || nonzero(out) < (long)w.size() || e < -120 || e > 120) ++g_failed;
      }
    }
  }
}

int main() {
  walk_planner();
  walk_packers();
  printf("%ld plans (%ld refused by the descriptor checks), %ld failures\n", g_plans, g_refused, g_failed);
  return g_failed ? 1 : 0;
}
