/* C ABI of libdeva_metrics.so: the scoring side of a VIPSeg run (evaluation, not inference; libdeva_hip.so and
 * include/deva_hip.h stay the inference library).  Every entry point is prefixed deva_metrics_ and no symbol is
 * defined in both libraries.
 *
 * All functions that return int return 0 on success and non-zero on failure; the text of the last failure of the
 * calling thread is behind deva_metrics_last_error().  Every argument check is made before any launch.
 */
#ifndef DEVA_METRICS_H
#define DEVA_METRICS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DEVA_METRICS_ABI_VERSION 1

int deva_metrics_version(void);
const char* deva_metrics_last_error(void);

/* ------------------------------------------------------------------------------------------
 * The joint count of one frame.
 *
 * Everything that the reference's three scoring scripts compute per pixel depends only on the pair (ground-truth
 * segment, predicted segment) at that pixel: the re-id pass of stuff_merging.py:52-57, the per-segment `pan == id`
 * passes of eval_stq_vipseg.py:132-147, the np.unique calls of segmentation_and_tracking_quality.py:32,142 and of
 * eval_vpq_vipseg.py:147,190.  deva_metrics_panoptic_counts makes that table in one pass over the two planes.
 *
 * Rules:
 *   C1  A pixel's id is, by the plane's encoding,
 *         DEVA_METRICS_RGB8     uint8 [H][W][3] as the PNG holds it: r + 256 g + 65536 b (eval_vpq_vipseg.py:131-132)
 *         DEVA_METRICS_I32      int32 [H][W]: the value
 *         DEVA_METRICS_I64      int64 [H][W]: the value (what deva_index_mask and deva_frame_result's labels give)
 *       A negative value and a value above 2^31 - 1 are ids that no table lists.
 *   C2  A side's table is `n` distinct ids in ascending order, each in 1 .. 2^31 - 1, int32 in device memory.  The
 *       slot of an id is 0 for id 0, 2 + i for table[i], and 1 for any other id.  (An unsorted table cannot be seen
 *       from the host: whoever builds it checks it.  A 0 in a table is never matched.)
 *   C3  DEVA_METRICS_INDEX16 (prediction only) is the tracker's own form: the int16 [H][W] channel plane of
 *       deva_frame_result and pred_lut, uint16 [channels], from channel to slot.  The slot of a pixel is
 *       pred_lut[channel]; several channels may share a slot; an entry >= P, a negative channel and a channel
 *       >= channels give slot 1.  There is no search and pred_ids is not read.
 *   C4  G = n_gt + 2, P = n_pred + 2, and counts[g][p], uint32 [G][P], is the number of pixels whose ground-truth slot
 *       is g and whose predicted slot is p.  The table is initialised by the call; its sum is H * W.  Integer adds:
 *       the result is exact and does not depend on the order of the adds.
 *
 * Refused before any launch: an unknown encoding (ground truth: RGB8 or I32); n_gt or n_pred outside 0 .. 1022 (G, P
 * at most 1024); height or width < 1 or H * W above 2^30; a null plane or counts; a null table with n > 0; a null
 * pred_lut or channels outside 1 .. 32767 with INDEX16; a plane that is not 16-byte aligned, a table or counts that is
 * not 4-byte aligned, a pred_lut that is not 2-byte aligned; counts overlapping any input.
 *
 * deva_metrics_panoptic_plan is the launch decision, host only (no device is touched, nothing is dereferenced but
 * `plan`): every lane takes strips of DEVA_METRICS_STRIP consecutive pixels; the id tables are held in LDS; with
 * path DEVA_METRICS_PATH_LDS the runs are added to a per-workgroup copy of the table in LDS and its non-zero bins
 * are flushed with one integer atomic each, which is taken while 4 (G P + n_gt + n_pred) <= DEVA_METRICS_LDS_LIMIT;
 * with DEVA_METRICS_PATH_GLOBAL they are added to counts directly.  lds_bytes is the dynamic LDS of the launch.
 */
#define DEVA_METRICS_RGB8 0
#define DEVA_METRICS_I32 1
#define DEVA_METRICS_I64 2
#define DEVA_METRICS_INDEX16 3

#define DEVA_METRICS_MAX_IDS 1022
#define DEVA_METRICS_STRIP 16
#define DEVA_METRICS_LDS_LIMIT 65536
#define DEVA_METRICS_PATH_LDS 0
#define DEVA_METRICS_PATH_GLOBAL 1

typedef struct deva_metrics_plan {
  int32_t path;
  uint32_t grid, block;
  uint32_t lds_bytes;
} deva_metrics_plan;

int deva_metrics_panoptic_plan(int height, int width, int n_gt, int n_pred, deva_metrics_plan* plan);
int deva_metrics_panoptic_counts(const void* gt, int gt_encoding, const int32_t* gt_ids, int n_gt,
                                 const void* pred, int pred_encoding, const int32_t* pred_ids, int n_pred,
                                 const uint16_t* pred_lut, int channels, int height, int width,
                                 uint32_t* counts, void* stream);

#ifdef __cplusplus
}
#endif
#endif
