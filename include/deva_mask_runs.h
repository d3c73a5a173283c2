/* C ABI of libdeva_mask_runs.so: a stack of mask planes [N][H][W] (bytes or float logits, overlapping or not) encoded
 * on the device into COCO run boundaries, with the area and box of every mask (a seventh library next to
 * libdeva_hip.so, libdeva_metrics.so, libdeva_vos_metrics.so, libdeva_pair_metrics.so, libdeva_regions.so and
 * libdeva_rle.so).  Every entry point is prefixed deva_runs_ and no symbol is defined in any two of the seven libraries.
 *
 * All functions that return int return 0 on success and non-zero on failure; the text of the last failure of the
 * calling thread is behind deva_runs_last_error().  Every argument check is made before any launch.  Nothing is
 * allocated and nothing is synchronised: planes, scratch and outputs are the caller's, and every kernel goes to the
 * stream that is handed in.
 *
 * Rules.  tests/runs_case.py is their executable statement.
 *   E1  predicate.  The input is [N][H][W], row-major, of one of two element types.  DEVA_RUNS_U8 (a torch.bool plane
 *       goes in as bytes): the pixel is 1 iff the byte is not 0.  DEVA_RUNS_F32 with a `threshold`: the pixel is 1 iff
 *       value > threshold, so NaN gives 0 and -0.0 against a threshold of 0 gives 0.
 *   E2  order.  Positions are column-major, p = x * H + y.  The value before p = 0 is 0.
 *   E3  output: the contract of deva_mask_rle_count / deva_mask_rle_write.  bounds_k is the ascending list of the p
 *       with pixel_k(p) != pixel_k(p - 1); n[k] = len(bounds_k), int32 [N] on the device; `bounds` is int32 on the
 *       device with the lists back to back in mask order.  The counts of mask k are diff([0, *bounds_k, H * W]): a
 *       leading 0 for a mask that starts with a 1, [H * W] for an empty one.
 *   E4  stats.  int32 [N][5]: area, x_min, y_min, x_max, y_max, the conventions of deva_frame_result's `stats`:
 *       inclusive coordinates; an empty mask keeps area 0, the minima INT32_MAX and the maxima -1.  Optional (NULL: not
 *       wanted).  Exact integer adds.
 *   E5  capacity.  base[k] = first + n[0] + ... + n[k-1] in int64, computed on the device (`first`: an int64 on the
 *       device, the `total` of the call before when several calls fill one `bounds`; NULL means 0); `total` (int64,
 *       device) always holds the full sum first + n[0] + ... + n[N-1].  A boundary whose slot is at or beyond `capacity`
 *       is not written, and nothing is ever written at or beyond `capacity`: the call is safe with any capacity, and the
 *       caller learns from `total` whether it was enough.
 *   E6  limits.  1 <= H * W < 2^31; the masks and the scratch of one call within what deva_runs_limits reports;
 *       deva_runs_scratch(n, h, w) gives the bytes of the caller's scratch (12 per segment: one int32 offset and one
 *       64-bit word as two int32; the scratch is 4-byte aligned), -1 beyond the limits.  A violation is an error that
 *       names the argument; nothing is launched and the outputs stay untouched.
 *   E7  addresses.  Any base address (a multiple of the element size) and any width are accepted.  16-byte loads are
 *       used only for pieces that are 16-byte aligned and lie wholly inside a row; anything else goes element by element.
 *       The results are the same either way.
 *
 * The kernels.  A mask is cut into tiles of DEVA_RUNS_TILE x DEVA_RUNS_TILE pixels and its scan order into segments: the
 * DEVA_RUNS_TILE rows of tile row ty in column x are segment x * tiles_y + ty, so segments ascend with p.
 *   count  a workgroup owns a tile (a grid-stride loop over mask x tile): it loads the tile row by row (E7), keeps one
 *          64-bit word of pixel bits per row in LDS, forms per row the word that differs from the row above (the row
 *          above the tile: the tile above's last row; for the top tile row the plane's last row one column to the left,
 *          E2) and takes every column's 64 boundary bits by one ballot.  The word goes to the scratch, its popcount
 *          beside it; the stats come off the row words.
 *   scan   one workgroup per mask turns the popcounts into offsets in place, DEVA_RUNS_SCAN_CHUNK segments at a time,
 *          and writes n[k]; one workgroup then turns n into `base` and `total`, DEVA_RUNS_MASK_CHUNK masks at a time.
 *   write  reads one bit per pixel from the scratch (never the planes again), gives each set bit its rank inside its
 *          word and stores p at base[k] + offset + rank under E5.
 * No kernel waits on another workgroup.
 */
#ifndef DEVA_MASK_RUNS_H
#define DEVA_MASK_RUNS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DEVA_RUNS_ABI_VERSION 1

#define DEVA_RUNS_TILE 64
#define DEVA_RUNS_U8 0
#define DEVA_RUNS_F32 1
#define DEVA_RUNS_MAX_MASKS 65536
#define DEVA_RUNS_MAX_SCRATCH 1073741824 /* bytes of one call's scratch: 2^30 */
#define DEVA_RUNS_SCAN_CHUNK 2048        /* segments of one step of the per-mask scan */
#define DEVA_RUNS_MASK_CHUNK 256         /* masks of one step of the cross-mask scan */

int deva_runs_version(void);
const char* deva_runs_last_error(void);

/* (struct tags only: the functions have the same names, so say `struct deva_runs_limits`, `struct deva_runs_plan`) */
struct deva_runs_limits {
  int32_t max_masks;    /* masks of one call */
  int32_t tile;         /* DEVA_RUNS_TILE */
  int32_t block;        /* lanes of a workgroup */
  int32_t scan_chunk;   /* DEVA_RUNS_SCAN_CHUNK */
  int32_t mask_chunk;   /* DEVA_RUNS_MASK_CHUNK */
  int32_t reserved;
  int64_t max_scratch;  /* bytes of one call's scratch */
};
int deva_runs_limits(struct deva_runs_limits* limits);

struct deva_runs_plan {
  int32_t tiles_x;        /* ceil(W / tile) */
  int32_t tiles_y;        /* ceil(H / tile) */
  int32_t segments;       /* of one mask: W * tiles_y */
  int32_t scan_chunks;    /* steps of the per-mask scan: ceil(segments / scan_chunk) */
  int32_t mask_chunks;    /* steps of the cross-mask scan: ceil(n / mask_chunk) */
  uint32_t count_grid;    /* workgroups of the count pass: one per tile and mask, capped (a grid-stride loop) */
  uint32_t write_grid;    /* workgroups of the write pass: one per `block` segments, capped */
  int32_t reserved;
  int64_t scratch_bytes;  /* what deva_runs_scratch gives */
};
/* the launch decision, host only: no device is touched, nothing is dereferenced but `plan` */
int deva_runs_plan(int n, int height, int width, struct deva_runs_plan* plan);

/* bytes of the caller's scratch for n masks of height x width; -1 beyond the limits (E6) */
int64_t deva_runs_scratch(int n, int height, int width);

/* planes: n x height x width elements of `dtype` on the device, aligned to the element; threshold: E1, read for
 * DEVA_RUNS_F32 only; scratch: deva_runs_scratch(n, height, width) bytes on the device, 4-byte aligned; n_out int32 [n],
 * base int64 [n], total int64 [1], all on the device; first: int64 [1] on the device or NULL (E5); stats: int32 [n][5] on
 * the device or NULL (E4).  n == 0 is a no-op that returns 0. */
int deva_runs_count(const void* planes, int dtype, float threshold, int n, int height, int width, void* scratch,
                    int64_t scratch_bytes, int32_t* n_out, int64_t* base, int64_t* total, const int64_t* first, int32_t* stats,
                    void* stream);

/* after deva_runs_count of the same n, height, width on the same stream, with its scratch and base untouched:
 * bounds int32 [capacity] on the device (may be NULL when capacity is 0).  n == 0 is a no-op that returns 0. */
int deva_runs_write(int n, int height, int width, const void* scratch, int64_t scratch_bytes, const int64_t* base,
                    int32_t* bounds, int64_t capacity, void* stream);

#ifdef __cplusplus
}
#endif
#endif
