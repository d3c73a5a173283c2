// Host-side weight packing of the convolutions (model load, not the frame path).  Plain C++, no HIP: the layouts are
// those the kernels of conv_igemm.hip / conv_mfma.hip / conv_f16.hip read (include/deva_hip.h).
#include <math.h>
#include <stdint.h>

#include "deva_hip.h"
#include "host_error.h"

// Host-side weight packing (model load, not the frame path): [cout][cin][kh][kw] -> the layout deva_conv2d reads.
extern "C" int64_t deva_conv_pack(const float* w_oihw, float* out, int cout, int cin, int kh, int kw, int want_q4,
                                  int* k_layout, int* cout_pad_out) {
  using namespace deva;
  if (!w_oihw || cout <= 0 || cin <= 0 || kh <= 0 || kw <= 0 || !k_layout || !cout_pad_out) {
    set_error("deva_conv_pack: bad arguments");
    return -1;
  }
  const int taps = kh * kw;
  const int K = taps * cin;
  const int cout_pad = (cout + 31) / 32 * 32;
  const bool chunk = taps > 1 && cin % 32 == 0;
  const bool q4 = want_q4 && cout > 1;  // the single-channel heads (conv_cout1.hip) read column 0 of [K][cout_pad]
  const int64_t rows = q4 ? (int64_t)(K + 3) / 4 * 4 : K;
  const int64_t elems = rows * cout_pad;
  *k_layout = (chunk ? DEVA_KLAYOUT_CHUNK32 : DEVA_KLAYOUT_TAP_MAJOR) | (q4 ? DEVA_KLAYOUT_Q4 : 0);
  *cout_pad_out = cout_pad;
  if (!out) return elems;
  for (int64_t i = 0; i < elems; ++i) out[i] = 0.0f;
  for (int m = 0; m < cout; ++m)
    for (int c = 0; c < cin; ++c)
      for (int t = 0; t < taps; ++t) {
        const int64_t k = chunk ? ((int64_t)(c / 32) * taps + t) * 32 + c % 32 : (int64_t)t * cin + c;
        const int64_t at = q4 ? ((k >> 2) * cout_pad + m) * 4 + (k & 3) : k * cout_pad + m;
        out[at] = w_oihw[((int64_t)m * cin + c) * taps + t];
      }
  return elems;
}

// fp16 weights of the opt-in amp path (host side, model load): element (k, m) at ((k/8)*cout_pad + m)*8 + k%8, IEEE
// binary16 bits, round to nearest even; K order: tap-major for 1x1, 64-channel slabs otherwise
// (k = ((c/64)*taps + tap)*64 + c%64; needs cin % 64 == 0, else -1: the layer stays fp32).
extern "C" int64_t deva_conv_pack_f16(const float* w_oihw, uint16_t* out, int cout, int cin, int kh, int kw, int* cout_pad_out) {
  using namespace deva;
  if (!w_oihw || cout <= 0 || cin <= 0 || kh <= 0 || kw <= 0 || !cout_pad_out) {
    set_error("deva_conv_pack_f16: bad arguments");
    return -1;
  }
  const int taps = kh * kw;
  if (cin % 64 != 0) return -1;
  const int K = taps * cin;
  const int cout_pad = (cout + 31) / 32 * 32;
  const int64_t elems = (int64_t)K * cout_pad;
  *cout_pad_out = cout_pad;
  if (!out) return elems;
  for (int64_t i = 0; i < elems; ++i) out[i] = 0;
  for (int m = 0; m < cout; ++m)
    for (int c = 0; c < cin; ++c)
      for (int t = 0; t < taps; ++t) {
        const int64_t k = taps > 1 ? ((int64_t)(c / 64) * taps + t) * 64 + c % 64 : c;
        const _Float16 h = (_Float16)w_oihw[((int64_t)m * cin + c) * taps + t];
        uint16_t bits;
        __builtin_memcpy(&bits, &h, 2);
        out[((k >> 3) * cout_pad + m) * 8 + (k & 7)] = bits;
      }
  return elems;
}

// hi / lo fp16 planes of the split path (host side, model load): with s = 2^e, e such that the largest |w| * s lies in
// [2^13, 2^14) (e = 0 for an all-zero layer), hi = fp16(w s), lo = fp16(w s - hi) (round to nearest even; w s and the
// difference are exact in fp32), element (k, plane, m) at (((k/8)*2 + plane)*cout_pad + m)*8 + k%8; K order: tap-major
// for 1x1 (any cin: K is padded with zero rows to a multiple of 32), 32-channel slabs otherwise
// (k = ((c/32)*taps + tap)*32 + c%32; needs cin % 32 == 0, else -1: the layer stays on the fp32 kernels).
// *scale_log2 = e; deva_conv2d multiplies the accumulators by 2^-e.
extern "C" int64_t deva_conv_pack_split(const float* w_oihw, uint16_t* out, int cout, int cin, int kh, int kw, int* cout_pad_out,
                                        int* scale_log2) {
  using namespace deva;
  if (!w_oihw || cout <= 0 || cin <= 0 || kh <= 0 || kw <= 0 || !cout_pad_out || !scale_log2) {
    set_error("deva_conv_pack_split: bad arguments");
    return -1;
  }
  const int taps = kh * kw;
  if (cin % 32 != 0 && taps > 1) return -1;
  const int K = (taps * cin + 31) / 32 * 32;  // 1x1 layers with a channel tail (513, 257): zero rows up to the next K step
  const int cout_pad = (cout + 31) / 32 * 32;
  const int64_t elems = (int64_t)K * 2 * cout_pad;
  *cout_pad_out = cout_pad;
  float wmax = 0.0f;
  const int64_t n = (int64_t)cout * cin * taps;
  for (int64_t i = 0; i < n; ++i) {
    const float v = fabsf(w_oihw[i]);
    if (!(v <= 3.0e38f)) {
      set_error("deva_conv_pack_split: non-finite weight");
      return -1;
    }
    if (v > wmax) wmax = v;
  }
  int e = 0;
  if (wmax > 0.0f) {
    int x;
    frexpf(wmax, &x);  // wmax = f * 2^x, f in [0.5, 1)
    e = 14 - x;
    if (e > 120) e = 120;
    if (e < -120) e = -120;
  }
  *scale_log2 = e;
  if (!out) return elems;
  for (int64_t i = 0; i < elems; ++i) out[i] = 0;
  for (int m = 0; m < cout; ++m)
    for (int c = 0; c < cin; ++c)
      for (int t = 0; t < taps; ++t) {
        const int64_t k = taps > 1 ? ((int64_t)(c / 32) * taps + t) * 32 + c % 32 : c;
        const float ws = ldexpf(w_oihw[((int64_t)m * cin + c) * taps + t], e);
        const _Float16 hi = (_Float16)ws;
        const _Float16 lo = (_Float16)(ws - (float)hi);
        uint16_t bh, bl;
        __builtin_memcpy(&bh, &hi, 2);
        __builtin_memcpy(&bl, &lo, 2);
        out[(((k >> 3) * 2 + 0) * cout_pad + m) * 8 + (k & 7)] = bh;
        out[(((k >> 3) * 2 + 1) * cout_pad + m) * 8 + (k & 7)] = bl;
      }
  return elems;
}
