/* C ABI of libdeva_rle.so: COCO run-length masks decoded on the device into byte or float planes, with the nearest
 * resize of a frame reader fused in (a sixth library next to libdeva_hip.so, libdeva_metrics.so, libdeva_vos_metrics.so,
 * libdeva_pair_metrics.so and libdeva_regions.so).  Every entry point is prefixed deva_rle_ and no symbol is defined in
 * any two of the six libraries.
 *
 * All functions that return int return 0 on success and non-zero on failure; the text of the last failure of the
 * calling thread is behind deva_rle_last_error().  Every argument check is made before any launch.  Nothing is
 * allocated, nothing is copied and nothing is synchronised: the run array is the caller's, on the host (to be checked)
 * and on the device (to be read).
 *
 * Rules.  tests/rle_case.py is their executable statement.
 *   D1  layout.  A mask of size H x W is a list of counts c_0, c_1, ...  Runs alternate 0, 1, 0, ... along the
 *       column-major scan, so pixel (y, x) is position p = x * H + y.  With s_k = c_0 + ... + c_{k-1}, pixel p has the
 *       value k & 1 for the one k with s_k <= p < s_k + c_k.  Counts of zero are legal anywhere: first, in the middle,
 *       last.  Several runs then share a start, and the run that owns p is the last one whose start is <= p.
 *   D2  validity, checked on the host before any launch: every count >= 0; the counts of a mask sum to H * W;
 *       1 <= H * W < 2^31 (and so for the output size); one source size and one output size per call; the masks and
 *       the run total of a call within what deva_rle_limits reports.  A violation is an error that names the mask;
 *       nothing is launched and the output is untouched.
 *   D3  resize.  Output pixel (y', x') takes source pixel (sy, sx) by the nearest rule of
 *       F.interpolate(mode='nearest'), computed as ATen does: the scale is in / out in fp32,
 *       sy = min(int(floorf(y' * scale)), in - 1), and sx likewise.  Equal sizes mean the identity.  No source-size
 *       plane is written.
 *   D4  output.  [n][OH][OW] row-major contiguous, uint8 with values 0 / 1 (DEVA_RLE_U8) or float with 0.0 / 1.0
 *       (DEVA_RLE_F32).  Every element is written, so the buffer may be uninitialised; nothing outside it is written.
 *   D5  records (the binding computes them on the host from the counts): per mask the number of runs, the area and
 *       the box of the ones, xyxy inclusive at source size, -1, -1, -1, -1 for an empty mask.
 *   D6  streams.  Every launch goes to the stream it is handed.
 *
 * The run array.  One int32 array per call of `words` = n + 1 + first[n] words:
 *       first[0 .. n]   first[k]: where mask k's starts begin in `starts`; first[0] = 0, first[n] = their total
 *       starts[...]     mask k with r_k runs holds r_k + 1 words: s_0 = 0, s_1, ..., s_{r_k} = H * W
 * so a count is a difference of neighbours, D2 reads "first[k+1] - first[k] >= 2, s_0 = 0, never descending, the last one
 * H * W", and a walk down the starts needs no end test: the last one is above every position.
 *
 * The kernel.  A workgroup owns a tile of DEVA_RLE_TILE x DEVA_RLE_TILE output pixels.  A lane takes one output column of
 * the tile and a quarter of its rows: it finds the run that owns the first source pixel it needs by one binary search
 * (an upper bound: D1), walks the starts down the column and writes 0 / 1 bytes into the tile in LDS, every row shifted
 * by what its address in the output lacks to 16 bytes.  The tile then leaves in 16-byte stores wherever 16 bytes of a
 * row are aligned and inside the tile, element by element at the ragged ends.  No plane is read back and no workgroup
 * waits on another.
 */
#ifndef DEVA_RLE_H
#define DEVA_RLE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DEVA_RLE_ABI_VERSION 1

#define DEVA_RLE_TILE 64
#define DEVA_RLE_U8 0
#define DEVA_RLE_F32 1
#define DEVA_RLE_MAX_MASKS 65536
#define DEVA_RLE_MAX_WORDS 67108864 /* of the run array of one call: 2^26 words, 256 MB */

int deva_rle_version(void);
const char* deva_rle_last_error(void);

/* (struct tags only: the functions have the same names, so say `struct deva_rle_limits`, `struct deva_rle_plan`) */
struct deva_rle_limits {
  int32_t max_masks;   /* masks of one call */
  int32_t max_words;   /* words of one call's run array: n + 1 + runs + n */
  int32_t tile;        /* DEVA_RLE_TILE */
  int32_t block;       /* lanes of a workgroup */
};
int deva_rle_limits(struct deva_rle_limits* limits);

struct deva_rle_plan {
  int32_t tiles_x;     /* ceil(OW / tile) */
  int32_t tiles_y;     /* ceil(OH / tile) */
  uint32_t grid;       /* workgroups: one per tile and mask, capped (a grid-stride loop) */
  int32_t lds_bytes;   /* the tile with its shift margin */
  float scale_y;       /* D3: H / OH in fp32 */
  float scale_x;       /* W / OW */
  int64_t out_bytes;   /* n x OH x OW elements */
};
/* the launch decision, host only: no device is touched, nothing is dereferenced but `plan` */
int deva_rle_plan(int n, int height, int width, int out_height, int out_width, int dtype, struct deva_rle_plan* plan);

/* D2 on a run array in host memory; host only.  n == 0 is valid with words == 1. */
int deva_rle_check(const int32_t* runs, int64_t words, int n, int height, int width);

/* runs_host: the run array in host memory, checked (D2) and not kept; runs_device: the same words on the device, in place
 * by the time the stream reaches the launch; out: n x OH x OW elements of `dtype` on the device, aligned to its element.
 * n == 0 is a no-op that returns 0. */
int deva_rle_decode(const int32_t* runs_host, const int32_t* runs_device, int64_t words, int n, int height, int width,
                    int out_height, int out_width, int dtype, void* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
