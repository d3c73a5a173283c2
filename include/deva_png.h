/* C ABI of libdeva_png.so: the zlib (deflate) stream of a PNG file coded on the device from a byte plane (gfx950 only).
 *
 * An id map after PNG's `Up` filter is almost all zeros, and long stretches of equal bytes are what deflate codes best
 * with nothing but matches at distance 1.  The coder below takes exactly that and nothing else, so its bytes are a
 * function of the pixels alone: the numpy statement (tests/png_case.py) implements these rules and the device agrees
 * with it byte for byte.  The host wraps the stream into a PNG file (signature, IHDR, PLTE, one IDAT, IEND and their
 * CRCs: deva/hip/png.py); nothing of that is done here.
 *
 * Z1. Input.  One plane on the device, contiguous, at any base alignment: uint8 [H][W] (bpp = 1) or uint8 [H][W][3]
 *     (bpp = 3).  1 <= H, W <= DEVA_PNG_MAX_SIDE and H * W * bpp <= DEVA_PNG_MAX_BYTES.  Row bytes n = W * bpp.
 * Z2. Filter.  Every row uses PNG filter type 2 (`Up`).  Its string is the byte 2 followed by row[y] - row[y-1] mod 256
 *     (row -1 is all zero): n + 1 bytes.
 * Z3. Runs.  Runs are the maximal stretches of equal bytes within one row string (the filter byte included, so a
 *     leading data byte 2 joins it).  Runs never cross rows.  A run of value b and length L is coded as the literal b,
 *     then floor((L - 1) / 258) matches of length 258 at distance 1; with r = (L - 1) mod 258, one match of length r at
 *     distance 1 follows if r >= 3, and r literals b otherwise.  There are no other matches.
 * Z4. Codes.  Deflate's fixed Huffman code (RFC 1951, 3.2.6): literals 0-143 take 8 bits, 144-255 take 9; length
 *     symbols take 7 or 8 bits plus their extra bits; distance 1 is the 5-bit code 0.  Codes are packed most
 *     significant bit first into the LSB-first bit stream, extra bits LSB first.
 * Z5. Segments.  Rows are cut into segments of `rows_per_segment` (R, from deva_png_plan) rows; the last may be short.
 *     A segment is one fixed-code block with BFINAL = 0, the tokens of its rows and end-of-block, followed by an empty
 *     stored block (the bits 000, zero bits up to the byte boundary, then 00 00 FF FF): every segment is a whole number
 *     of bytes.
 * Z6. Framing.  78 01, the segments in row order, the final block (fixed code, BFINAL = 1, end-of-block only: 03 00),
 *     the Adler-32 of all row strings, big-endian.
 * Z7. Capacity.  Nothing is written at or beyond `capacity` bytes of `out`.  The true total is always reported.
 *     `worst_case` of the plan is a capacity no input exceeds: every byte of every row string a 9-bit literal, and each
 *     segment's overhead.
 * Z8. Record.  int64 info[4] on the device: [0] the total bytes of the stream, [1] the Adler-32, [2] 1 if the total
 *     exceeds `capacity` (the stream in `out` is then cut at `capacity`), else 0, [3] the segment count.  All work goes
 *     on `stream`, nothing synchronises, and no kernel waits on another workgroup.
 *
 * Three kernels.  `segment_kernel`: one workgroup per segment codes it into the segment's worst-case slot of the
 * caller's scratch and records its byte count and its two Adler sums.  `offsets_kernel`: one workgroup scans the byte
 * counts to offsets, combines the Adler sums, and writes info, the two header bytes and the six trailing bytes.
 * `place_kernel`: one workgroup per segment copies its slot behind the segments before it, below `capacity`.
 * deva_png_place runs the last two again on a scratch that deva_png_deflate filled, into a larger `out`: how a caller
 * whose capacity was exceeded gets the whole stream without coding twice. */
#ifndef DEVA_PNG_H
#define DEVA_PNG_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DEVA_PNG_ABI_VERSION 1
#define DEVA_PNG_MAX_SIDE 16384          /* H, W */
#define DEVA_PNG_MAX_BYTES (1 << 29)     /* H * W * bpp */
#define DEVA_PNG_ROWS_PER_SEGMENT 8      /* R */
#define DEVA_PNG_STEP 1024               /* bytes of a row string a workgroup takes in one step */

int deva_png_version(void);
const char* deva_png_last_error(void);

/* (struct tags only: the functions have the same names, so say `struct deva_png_limits`, `struct deva_png_plan`) */
struct deva_png_limits {
  int32_t max_side;          /* DEVA_PNG_MAX_SIDE */
  int32_t max_bytes;         /* DEVA_PNG_MAX_BYTES */
  int32_t rows_per_segment;  /* DEVA_PNG_ROWS_PER_SEGMENT */
  int32_t step;              /* DEVA_PNG_STEP */
  int32_t block;             /* lanes of a workgroup */
  int32_t lds_bytes;         /* LDS of a workgroup of segment_kernel */
};
int deva_png_limits(struct deva_png_limits* limits);

struct deva_png_plan {
  int32_t rows_per_segment;  /* R */
  int32_t segments;          /* ceil(H / R) */
  int32_t row_bytes;         /* n = W * bpp */
  int32_t steps_per_row;     /* ceil((n + 1) / DEVA_PNG_STEP) */
  int32_t block;             /* lanes of a workgroup */
  int32_t reserved;          /* 0 */
  int64_t slot_bytes;        /* a segment's slot in the scratch: its worst case, rounded up to 16 */
  int64_t scratch_bytes;     /* what deva_png_deflate asks of `scratch` */
  int64_t worst_case;        /* Z7 */
};
/* the sizes for a plane, host only: no device is touched, nothing is dereferenced but the arguments */
int deva_png_plan(int height, int width, int bpp, struct deva_png_plan* plan);

/* Z1-Z8: plane uint8 [height][width][bpp] -> out[0, min(total, capacity)), info int64 [4]; all on the device.
 * scratch: 16-byte aligned, plan.scratch_bytes; out: any alignment (may be NULL with capacity 0); info: 8-byte aligned */
int deva_png_deflate(const uint8_t* plane, int height, int width, int bpp, void* scratch, int64_t scratch_bytes, uint8_t* out,
                     int64_t capacity, int64_t* info, void* stream);

/* the stream of the plane that deva_png_deflate last coded into `scratch` (same height, width, bpp), placed again into
 * `out` under `capacity`, and info written again */
int deva_png_place(int height, int width, int bpp, void* scratch, int64_t scratch_bytes, uint8_t* out, int64_t capacity,
                   int64_t* info, void* stream);

#ifdef __cplusplus
}
#endif
#endif
