/* C ABI of libdeva_rle_overlap.so: the overlap of every mask of one list of COCO run-length masks ("detections") with
 * every mask of another ("ground truth"), taken from the run lengths themselves on the device: the integers behind
 * pycocotools' mask.iou (an eighth library next to libdeva_hip.so, libdeva_metrics.so, libdeva_vos_metrics.so,
 * libdeva_pair_metrics.so, libdeva_regions.so, libdeva_rle.so and libdeva_mask_runs.so).  Every entry point is prefixed
 * deva_overlap_ and no symbol is defined in any two of the eight libraries.
 *
 * All functions that return int return 0 on success and non-zero on failure; the text of the last failure of the
 * calling thread is behind deva_overlap_last_error().  Every argument check is made before any launch.  Nothing is
 * allocated, nothing is copied and nothing is synchronised: run arrays, boxes, scratch and outputs are the caller's, and
 * every kernel goes to the stream that is handed in.
 *
 * Rules.  tests/overlap_case.py is their executable statement.
 *   O1  input.  Two run arrays in exactly the layout of deva_rle.h ("The run array": first[0 .. n], then per mask its
 *       starts s_0 = 0, ..., s_r = H * W), one of D masks and one of G masks, all of one common H x W.  A mask is the
 *       pixels of rule D1 of deva_rle.h: position p has the value k & 1 for the last run k whose start is <= p, so
 *       counts of zero are legal anywhere.
 *   O2  validity, checked on the host copies before any launch: rule D2 of deva_rle.h on either side (first[0] = 0,
 *       every mask with at least two starts, s_0 = 0, never descending, the last one H * W; 1 <= H * W < 2^31; the
 *       masks and the words of a side within what deva_overlap_limits reports).  A violation is an error that names
 *       the side ("dt" or "gt") and the mask; nothing is launched and the outputs are untouched.
 *   O3  output.  inter[d][g], uint32, at inter[d * pitch + g] with pitch >= G (a call may fill a block of a larger
 *       table): the number of positions that are 1 in detection d and in ground-truth mask g.  area_d[D] and area_g[G],
 *       uint32: the number of ones of every mask.  H * W < 2^31, so all fit.  Every one of these elements is written,
 *       so the buffers may be uninitialised; nothing outside them is written, the pitch's gap included.
 *   O4  exactness.  All values are exact integers, summed with integer adds: they do not depend on the grid, on the
 *       schedule or on whether a mask's runs were held in LDS.
 *   O5  cost.  No plane is formed and no pixel is visited: the work is a function of the run counts, not of H * W.
 *   O6  boxes.  Optional (both NULL: not given), int32 [n][4] per side on the device: x0, y0, x1, y1 inclusive, -1 four
 *       times for an empty mask, as rule D5 of deva_rle.h records them.  A box must contain every one of its mask.  A
 *       pair whose boxes share no pixel is written 0 and its runs are not read.
 *   O7  empty sides.  D == 0 or G == 0 is a no-op that returns 0: nothing is launched and nothing is written.
 *   O8  scratch.  deva_overlap_scratch(words_g, G) bytes, 4-byte aligned: one int32 per start of the ground-truth side.
 *       -1 beyond the limits.
 *   O9  streams.  Every launch goes to the stream it is handed.
 *
 * The kernels.  Two launches.
 *   scan   a workgroup per mask of either side (a grid-stride loop): the lengths of the one-runs, scanned
 *          DEVA_OVERLAP_SCAN_CHUNK starts at a time, give ones_before[k], the ones in front of start k, for the
 *          ground-truth side (the scratch) and the area of every mask of both sides.
 *   pairs  a workgroup owns one g and DEVA_OVERLAP_D_CHUNK consecutive d (a grid-stride loop).  It drops the d whose
 *          boxes miss g's (O6) and, if any is left, copies g's starts and ones_before into LDS when g has at most
 *          DEVA_OVERLAP_LDS_RUNS runs; a mask of more runs takes the same code on global memory.  The starts of the
 *          chunk's d lie back to back in the run array: every lane takes a contiguous stretch of them, finds the run
 *          of g that owns its first one-run's first position by one binary search (an upper bound: O1) and then walks
 *          g's starts forward, a merge; a gap of more than a few runs is crossed by a search over what is left.  With
 *          P_g(p) = ones_before[k] + (k odd ? p - s_k : 0) for the owner k of p, a one-run [a, b) of d adds
 *          P_g(b) - P_g(a).  A lane's sums go to the chunk's D_CHUNK counters in LDS by integer atomic adds, and since
 *          no pair is split over workgroups every inter[d][g] leaves by one plain store.
 * No kernel waits on another workgroup.
 */
#ifndef DEVA_RLE_OVERLAP_H
#define DEVA_RLE_OVERLAP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DEVA_OVERLAP_ABI_VERSION 1

#define DEVA_OVERLAP_MAX_MASKS 65536    /* of one side of one call, as DEVA_RLE_MAX_MASKS */
#define DEVA_OVERLAP_MAX_WORDS 67108864 /* of one side's run array, as DEVA_RLE_MAX_WORDS */
#define DEVA_OVERLAP_D_CHUNK 8          /* detections a workgroup of the pair pass owns */
#define DEVA_OVERLAP_LDS_RUNS 1983      /* runs of a ground-truth mask that is held in LDS: 1984 starts, 15.5 KB with ones_before */
#define DEVA_OVERLAP_SCAN_CHUNK 1024    /* starts of one step of the scan */
#define DEVA_OVERLAP_DT 0
#define DEVA_OVERLAP_GT 1

int deva_overlap_version(void);
const char* deva_overlap_last_error(void);

/* (struct tags only: the functions have the same names, so say `struct deva_overlap_limits`, `struct deva_overlap_plan`) */
struct deva_overlap_limits {
  int32_t max_masks;   /* masks of one side of one call */
  int32_t max_words;   /* words of one side's run array: n + 1 + runs + n */
  int32_t block;       /* lanes of a workgroup */
  int32_t d_chunk;     /* DEVA_OVERLAP_D_CHUNK */
  int32_t lds_runs;    /* DEVA_OVERLAP_LDS_RUNS */
  int32_t scan_chunk;  /* DEVA_OVERLAP_SCAN_CHUNK */
};
int deva_overlap_limits(struct deva_overlap_limits* limits);

struct deva_overlap_plan {
  uint32_t scan_grid;     /* workgroups of the scan: one per mask of either side, capped (a grid-stride loop) */
  uint32_t pair_grid;     /* workgroups of the pair pass: one per g and chunk of d, capped */
  int32_t d_chunks;       /* ceil(D / d_chunk) */
  int32_t lds_bytes;      /* of a workgroup of the pair pass */
  int64_t scratch_bytes;  /* what deva_overlap_scratch gives */
};
/* the launch decision, host only: no device is touched, nothing is dereferenced but `plan`.  words_g: of the
 * ground-truth side's run array. */
int deva_overlap_plan(int d, int g, int64_t words_g, struct deva_overlap_plan* plan);

/* bytes of the caller's scratch (O8); -1 beyond the limits */
int64_t deva_overlap_scratch(int64_t words_g, int g);

/* O2 on one side's run array in host memory; host only.  side: DEVA_OVERLAP_DT or DEVA_OVERLAP_GT, for the text.
 * n == 0 is valid with words == 1. */
int deva_overlap_check(const int32_t* runs, int64_t words, int n, int height, int width, int side);

/* dt_host, gt_host: the run arrays in host memory, checked (O2) and not kept; dt_device, gt_device: the same words on
 * the device, in place by the time the stream reaches the launches; box_d [d][4], box_g [g][4]: O6, both or neither;
 * scratch: O8; inter, pitch: O3 (pitch in elements); area_d [d], area_g [g].  All but the host arrays on the device,
 * 4-byte aligned. */
int deva_overlap_intersections(const int32_t* dt_host, const int32_t* dt_device, int64_t dt_words, int d, const int32_t* gt_host,
                               const int32_t* gt_device, int64_t gt_words, int g, int height, int width, const int32_t* box_d,
                               const int32_t* box_g, void* scratch, int64_t scratch_bytes, uint32_t* inter, int64_t pitch,
                               uint32_t* area_d, uint32_t* area_g, void* stream);

#ifdef __cplusplus
}
#endif
#endif
