/* C ABI of libdeva_jpeg.so: the entropy-coded data of a baseline JPEG file coded on the device from an RGB plane (gfx950
 * only).
 *
 * The overlay of the `demo` dataset is the one per-frame product a user looks at, and a baseline JPEG suits the device:
 * the transform is 8 x 8 blocks with no dependence between them, and restart markers make the entropy-coded data a
 * concatenation of byte-aligned pieces that are coded independently.  The bytes are a function of the pixels and of three
 * parameters (`quality`, `subsampling`, `restart`) alone: the numpy statement (tests/jpeg_case.py) implements the rules
 * below and the device agrees with it byte for byte.  All arithmetic is in integers, so no result depends on summation
 * order or on contraction.  The host puts the markers around the data (deva/hip/jpeg.py); nothing of that is done here.
 *
 * J1. Colour.  uint8 [H][W][3] RGB on the device, contiguous, at any base alignment; 1 <= H, W <= DEVA_JPEG_MAX_SIDE and
 *     H * W * 3 <= DEVA_JPEG_MAX_BYTES.  JFIF full range in 16-bit fixed point with arithmetic shifts:
 *     Y = (19595 R + 38470 G + 7471 B + 32768) >> 16, Cb = ((-11059 R - 21709 G + 32768 B + 32767) >> 16) + 128,
 *     Cr = ((32768 R - 27439 G - 5329 B + 32767) >> 16) + 128.  All three lie in 0 .. 255.
 * J2. Padding.  The three planes are padded to a multiple of the MCU (16 for subsampling 420, 8 for 444) by repeating
 *     the last column and the last row.
 * J3. Chroma.  At 420, Cb and Cr are (a + b + c + d + 2) >> 2 over each 2 x 2 of the padded planes.
 * J4. DCT.  Samples are level-shifted by -128.  The 8 x 8 DCT-II is two integer matrix passes with
 *     M[k][n] = round(8192 s_k cos((2n + 1) k pi / 16)), s_0 = sqrt(1/8), s_k = 1/2 otherwise.  Rows: t = (M x + 1024) >> 11
 *     (|M x| < 2^22); columns: u = M t (|u| < 2^28), so u carries a scale of 2^15.
 * J5. Quantisation.  The Annex K luminance and chrominance tables of ITU-T T.81, scaled as libjpeg scales them:
 *     s = 5000 / q for q < 50, else 200 - 2 q; Q = clamp((base s + 50) / 100, 1, 255); quality q is 1 .. 100.  The
 *     coefficient is sign(u) ((|u| + (Q << 14)) / (Q << 15)), an exact integer division.
 * J6. Entropy coding.  Zigzag order, the "typical" Huffman tables of Annex K.3; the DC difference is taken against the
 *     previous block of the same component; ZRL for every 16 zeros of a run above 15; EOB unless coefficient 63 is
 *     non-zero.  Bits are packed most significant first.
 * J7. MCU order.  MCUs in raster order; inside an MCU Y (row major, four at 420), then Cb, then Cr.  One interleaved scan.
 * J8. Restart intervals.  `restart` is a number of MCUs, at most 65535; 0 means one MCU row.  Every interval's bits are
 *     padded with 1-bits to a byte.  Behind every interval but the last, FF D0+m follows, m the interval's number modulo
 *     8, and the three DC predictors return to 0.
 * J9. Stuffing.  A data byte FF (the padded byte included) is followed by 00.  The markers of J8 are not data.
 * J10. The host makes everything that is not entropy-coded data: SOI, the JFIF APP0, two DQT, SOF0, four DHT, DRI, the
 *     SOS header and EOI.  Nothing is written at or beyond `capacity` bytes of `out`; the true total is always reported.
 *     int64 info[4] on the device: [0] the total bytes of the data, [1] the 8 x 8 blocks coded, [2] 1 if the total
 *     exceeds `capacity` (the data in `out` is then cut at `capacity`), else 0, [3] the interval count.  All work goes on
 *     `stream`, nothing synchronises, and no kernel waits on another workgroup.
 *
 * Four kernels.  `transform_kernel`: one workgroup per tile of 1024 pixels of one MCU row, J1-J5, int16 coefficients in
 * zigzag order into the caller's scratch.  `interval_kernel`: one workgroup per restart interval, a lane per block,
 * 256 blocks a step: bit counts, a workgroup scan, the codes ORed into a bit buffer in LDS, the stuffing pass, 16-byte
 * stores into the interval's worst-case slot.  `offsets_kernel`: the byte counts scanned to offsets, and info.
 * `place_kernel`: one workgroup per interval copies its slot behind the intervals before it, below `capacity`.
 * deva_jpeg_place runs the last two again on a scratch that deva_jpeg_scan filled, into a larger `out`. */
#ifndef DEVA_JPEG_H
#define DEVA_JPEG_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DEVA_JPEG_ABI_VERSION 1
#define DEVA_JPEG_MAX_SIDE 16384          /* H, W */
#define DEVA_JPEG_MAX_BYTES (1 << 29)     /* H * W * 3 */
#define DEVA_JPEG_MAX_RESTART 65535       /* MCUs of an interval (the DRI field) */
#define DEVA_JPEG_420 420                 /* `subsampling`: chroma halved both ways, MCU 16 x 16, 6 blocks */
#define DEVA_JPEG_444 444                 /* none, MCU 8 x 8, 3 blocks */

int deva_jpeg_version(void);
const char* deva_jpeg_last_error(void);

/* (struct tags only: the functions have the same names) */
struct deva_jpeg_limits {
  int32_t max_side;          /* DEVA_JPEG_MAX_SIDE */
  int32_t max_bytes;         /* DEVA_JPEG_MAX_BYTES */
  int32_t max_restart;       /* DEVA_JPEG_MAX_RESTART */
  int32_t block_bits;        /* the longest coded block: 20 + 63 * 26 bits */
  int32_t block;             /* lanes of a workgroup = blocks an interval's workgroup codes in one step */
  int32_t lds_bytes;         /* LDS of a workgroup of interval_kernel */
};
int deva_jpeg_limits(struct deva_jpeg_limits* limits);

struct deva_jpeg_plan {
  int32_t mcu;               /* 16 or 8 */
  int32_t mcus_x;            /* ceil(W / mcu) */
  int32_t mcus_y;            /* ceil(H / mcu) */
  int32_t blocks_per_mcu;    /* 6 or 3 */
  int32_t restart;           /* MCUs of an interval: `restart`, or mcus_x for 0 (what DRI holds) */
  int32_t intervals;         /* ceil(mcus_x * mcus_y / restart) */
  int32_t blocks;            /* mcus_x * mcus_y * blocks_per_mcu */
  int32_t block;             /* lanes of a workgroup */
  int64_t coef_bytes;        /* blocks * 128 */
  int64_t slot_bytes;        /* an interval's slot in the scratch: its worst case, rounded up to 16, and 16 */
  int64_t scratch_bytes;     /* what deva_jpeg_scan asks of `scratch` */
  int64_t worst_case;        /* a capacity no plane of this size exceeds */
};
/* the sizes for a plane, host only: no device is touched, nothing is dereferenced but the arguments */
int deva_jpeg_plan(int height, int width, int subsampling, int restart, struct deva_jpeg_plan* plan);

/* J5: the two tables of `quality` as a DQT holds them, luminance then chrominance, 64 bytes each in zigzag order; host only */
int deva_jpeg_quant(int quality, uint8_t* tables);

/* J1-J10: plane uint8 [height][width][3] -> out[0, min(total, capacity)), info int64 [4]; all on the device.
 * scratch: 16-byte aligned, plan.scratch_bytes; out: any alignment (may be NULL with capacity 0); info: 8-byte aligned */
int deva_jpeg_scan(const uint8_t* plane, int height, int width, int quality, int subsampling, int restart, void* scratch,
                   int64_t scratch_bytes, uint8_t* out, int64_t capacity, int64_t* info, void* stream);

/* the data of the plane that deva_jpeg_scan last coded into `scratch` (same height, width, subsampling, restart), placed
 * again into `out` under `capacity`, and info written again */
int deva_jpeg_place(int height, int width, int subsampling, int restart, void* scratch, int64_t scratch_bytes, uint8_t* out,
                    int64_t capacity, int64_t* info, void* stream);

#ifdef __cplusplus
}
#endif
#endif
