/* C ABI of libdeva_lowres.so: the proposal filter and the best-mask choice of a promptable segmenter taken straight from
 * its LOW-RESOLUTION mask logits (gfx950 only).
 *
 * A SAM-class mask decoder gives planes of 256 x 256 logits.  Its `postprocess_masks` brings them to frame size with two
 * chained bilinear resizes (low -> model_size x model_size, crop to the resized frame, -> the frame), and only then are
 * they thresholded, counted and boxed (deva_proposal_batch, deva_box_mask_select of deva_hip.h).  The frame-sized fp32
 * planes exist only to be compared with three thresholds.  This library forms every frame-sized value on the fly from
 * the low-resolution plane, which stays in cache, and writes byte planes only: what deva_proposal_batch and
 * deva_box_mask_select leave, without the planes they read.
 *
 * `postprocess_masks` belongs to segment_anything, which is not part of the reference's tree: as with
 * deva_proposal_batch, the rules below ARE the contract, and the CPU statement (tests/lowres_case.py) is written from
 * them.  The device agrees with that statement bit for bit.
 *
 * L1. One axis of one resize, n_in -> n_out, destination index d.  Every operation is a rounded fp32 one, and no
 *     operation of L1 or L2 is contracted into a fused multiply-add:
 *       scale = fp32(n_in) / fp32(n_out)                 (one division, on the host, once per call)
 *       s  = max(scale * (fp32(d) + 0.5f) - 0.5f, 0.0f)
 *       i0 = min((int)s, n_in - 1),  i1 = min(i0 + 1, n_in - 1)
 *       l1 = s - fp32(i0),  l0 = 1.0f - l1
 * L2. One resized value, in the order written:
 *       v = l0y * (l0x * a + l1x * b) + l1y * (l0x * c + l1x * d)
 *     with the taps a = src[y0][x0], b = src[y0][x1], c = src[y1][x0], d = src[y1][x1].
 * L3. The two stages: mid = resize(low [LH][LW] -> [M][M]), each value rounded to fp32; out = resize(mid[:IH, :IW] ->
 *     [OH][OW]).  Stage 2's n_in are IH and IW, so its clamp is at the crop's edge, not at M.  M is `model_size` (1024
 *     for SAM); (IH, IW) is `in_h`, `in_w`: the frame after the segmenter's longest-side resize.  The caller passes it;
 *     it is not derived in here.
 * L4. NaN and infinities follow IEEE through L2 (0 * inf is NaN), as in ATen.
 * L5. deva_lowres_proposal_batch: rules 1-4 of deva_proposal_batch (deva_hip.h) applied to the values of L3 -- live by
 *     predicted IoU, hi / lo, stability, bytes, box -- with the same thresholds, rounded the same way.  Afterwards the
 *     arena and the scratch (table, count, slots) hold byte for byte what deva_proposal_batch leaves when it is given
 *     the materialised planes of L3 (deva_lowres_upsample).  A plane that is not live is never evaluated.  It works on
 *     the arena and the scratch that deva_proposal_begin prepared and that deva_proposal_finish / _gather read, so a
 *     frame may mix it with deva_proposal_batch.
 * L6. deva_lowres_select: rules S1-S3 of deva_box_mask_select on the planes of L3.  Only the chosen candidate of a box
 *     is evaluated.  With scores == NULL and per_box == 1 it is a plain threshold.
 * L7. Limits; every check runs before the first launch: 1 <= IH, IW <= M <= 4096; 1 <= LH, LW <= 4096; an output
 *     plane has at most 2^30 pixels; any batch >= 0 (batch * per_box <= 2^30); offsets are 64-bit; output bytes go to
 *     any alignment.  All work goes on `stream`, nothing synchronises, and no kernel waits on another workgroup.
 *
 * Not ATen bit for bit.  ATen computes the source index of L1 with the same formula but in its own order and, on the
 * device, with contracted multiply-adds; its CPU code is vectorised differently again.  The statement differs from
 * `F.interpolate(F.interpolate(low, (M, M))[..., :IH, :IW], (OH, OW))` (bilinear, align_corners=False) in the last bits
 * of the source index: a few 1e-4 on logits of N(0, 8^2) at 1080p, and a sign flip in about one value of six million
 * (DESIGN section 26 has the measured bound, tests/lowres_case.py holds it).  Bit identity with ATen is not a goal, as
 * the order among tied boxes is not torchvision's (deva_proposal_finish, rule 5): this statement is fixed, and the
 * device is held to it.
 *
 * Two launch shapes, chosen on the host from the geometry alone (deva_lowres_plan), never in a kernel:
 *   tile   a workgroup owns a band of `tile_rows` whole output rows.  It loads the low-resolution rows the band needs
 *          into LDS, forms the band's rows of `mid` in LDS once (four taps each), and takes every output pixel from
 *          four LDS taps.
 *   point  where the band's part of `mid` would not fit the LDS budget or would hold more than three values per output
 *          pixel (strong minification): each lane evaluates its 16 low-resolution taps directly.
 * Both evaluate L1 / L2 with the same device function, so the fused filter equals the materialised one bit for bit. */
#ifndef DEVA_LOWRES_H
#define DEVA_LOWRES_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DEVA_LOWRES_ABI_VERSION 1
#define DEVA_LOWRES_MAX_SIDE 4096          /* LH, LW, M */
#define DEVA_LOWRES_MAX_PIXELS (1 << 30)   /* OH * OW */
#define DEVA_LOWRES_MAX_PER_BOX 16
#define DEVA_LOWRES_LDS_BUDGET 61440       /* bytes of LDS the patch of a workgroup of the tile path may take (60 KB) */
#define DEVA_LOWRES_MAX_TILE_ROWS 16
#define DEVA_LOWRES_PATH_TILE 0
#define DEVA_LOWRES_PATH_POINT 1

int deva_lowres_version(void);
const char* deva_lowres_last_error(void);

/* (struct tags only: the functions have the same names, so say `struct deva_lowres_limits`, `struct deva_lowres_plan`) */
struct deva_lowres_limits {
  int32_t max_side;       /* DEVA_LOWRES_MAX_SIDE */
  int32_t max_pixels;     /* DEVA_LOWRES_MAX_PIXELS */
  int32_t max_per_box;    /* DEVA_LOWRES_MAX_PER_BOX */
  int32_t block;          /* lanes of a workgroup */
  int32_t lds_budget;     /* DEVA_LOWRES_LDS_BUDGET */
  int32_t max_tile_rows;  /* DEVA_LOWRES_MAX_TILE_ROWS */
};
int deva_lowres_limits(struct deva_lowres_limits* limits);

/* the geometry of L3 */
struct deva_lowres_geometry {
  int32_t low_h, low_w;  /* LH, LW */
  int32_t model_size;    /* M */
  int32_t in_h, in_w;    /* IH, IW */
  int32_t out_h, out_w;  /* OH, OW */
  int32_t reserved;      /* 0 */
};

struct deva_lowres_plan {
  int32_t path;        /* DEVA_LOWRES_PATH_TILE or _POINT */
  int32_t tile_rows;   /* whole output rows a workgroup owns (both paths) */
  int32_t tile_cols;   /* OW */
  int32_t cover_rows;  /* output rows its LDS patch covers: tile_rows plus the rows its last 16-byte piece may reach into */
  int32_t mid_rows;    /* rows of `mid` (IW values each) in LDS; 0 on the point path */
  int32_t low_rows;    /* rows of `low` (LW values each) in LDS; 0 on the point path */
  int32_t lds_bytes;   /* 4 * (mid_rows * IW + low_rows * LW); 0 on the point path */
  int32_t block;       /* lanes of a workgroup */
  uint32_t grid_x;     /* bands of a plane: ceil(OH / tile_rows) */
  uint32_t grid_y_max; /* planes of one launch at most */
  int64_t mid_values;  /* values of `mid` a band forms: mid_rows * IW on the tile path, 4 per output pixel on the point path */
  int64_t out_values;  /* output pixels of a band: tile_rows * OW */
};
/* the launch decision for a geometry, host only: no device is touched, nothing is dereferenced but the arguments */
int deva_lowres_plan(const struct deva_lowres_geometry* geometry, struct deva_lowres_plan* plan);

/* L3 materialised: low fp32 [batch][LH][LW] -> out fp32 [batch][OH][OW], both on the device, 4-byte aligned */
int deva_lowres_upsample(const float* low, int batch, const struct deva_lowres_geometry* geometry, float* out, void* stream);

/* L6: low fp32 [batch][per_box][LH][LW], scores fp32 [batch][per_box] (or NULL with per_box == 1) -> out uint8
 * [batch][OH][OW] at any alignment, chosen int32 [batch] (may be NULL); all on the device */
int deva_lowres_select(const float* low, const float* scores, int batch, int per_box, const struct deva_lowres_geometry* geometry,
                       double mask_threshold, uint8_t* out, int32_t* chosen, void* stream);

/* L5: low fp32 [batch][LH][LW], iou_preds fp32 [batch]; thresholds, arena, capacity and scratch as deva_proposal_batch
 * takes them (scratch: deva_proposal_scratch(capacity) bytes, prepared by deva_proposal_begin); the planes are OH x OW */
int deva_lowres_proposal_batch(const float* low, const float* iou_preds, int batch, const struct deva_lowres_geometry* geometry,
                               double pred_iou_thresh, double stability_score_thresh, double stability_score_offset,
                               double mask_threshold, uint8_t* arena, int capacity, void* scratch, int64_t scratch_bytes,
                               void* stream);

#ifdef __cplusplus
}
#endif
#endif
