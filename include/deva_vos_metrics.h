/* C ABI of libdeva_vos_metrics.so: the DAVIS measures of a video-object-segmentation run -- region similarity J,
 * boundary accuracy F and J&F (evaluation, not inference; libdeva_hip.so stays the inference library and
 * libdeva_metrics.so the VIPSeg scorer).  Every entry point is prefixed deva_vos_ and no symbol is defined in any two of
 * the three libraries.
 *
 * All functions that return int return 0 on success and non-zero on failure; the text of the last failure of the
 * calling thread is behind deva_vos_last_error().  Every argument check is made before any launch.  Nothing is
 * allocated and nothing is synchronised: the scratch is the caller's, sized by deva_vos_boundary_scratch_bytes.
 */
#ifndef DEVA_VOS_METRICS_H
#define DEVA_VOS_METRICS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DEVA_VOS_ABI_VERSION 1

int deva_vos_version(void);
const char* deva_vos_last_error(void);

/* ------------------------------------------------------------------------------------------
 * The seven counts of one frame.
 *
 * The public DAVIS toolkits (davis2017-evaluation, vos-benchmark) make one boolean plane per object and frame, take its
 * boundary map (seg2bmap), dilate it with a disk and count.  Everything J and F need from a frame is seven integers per
 * object; deva_vos_boundary_counts makes them for up to 64 objects at once from the two label planes, with one bit per
 * object in a 64-bit word per pixel.  The rules below were written from those toolkits' published behaviour (neither is
 * part of this repository); they are the contract, and tests/vos_case.py is their executable statement.
 *
 * Rules:
 *   R1  slots.  `ids` is int32 in device memory: n_objects distinct ascending ids in 1 .. 2^31 - 1, n_objects in
 *       1 .. 64 (an unsorted table cannot be seen from the host: whoever builds it checks it).  Object i is id ids[i]
 *       on both sides.  A pixel whose value is not in the list (0, 255, anything else, negative) belongs to no object.
 *         DEVA_VOS_U8       uint8 [H][W]: the palette index of a DAVIS PNG
 *         DEVA_VOS_I32      int32 [H][W]: the value
 *         DEVA_VOS_I64      int64 [H][W]: the value (prediction only)
 *         DEVA_VOS_INDEX16  int16 [H][W] (prediction only): the tracker's channel plane and pred_lut, uint16 [channels],
 *                           from channel to object index; several channels may share an object; an entry >= n_objects,
 *                           a negative channel and a channel >= channels mean no object (rule C3 of deva_metrics.h).
 *                           There is no search.
 *       DEVA_VOS_BINARY, or-ed into either side's encoding, makes every non-zero value of that plane object 0 (the
 *       DAVIS 2016 / saliency form, PNGs of 0 / 255); n_objects must be 1 and neither ids' values nor pred_lut are used
 *       for that side.
 *   R2  boundary map: seg2bmap at the mask's own size.  For the boolean plane s of an object, pixel (y, x) is a
 *       boundary pixel if s(y, x) differs from
 *         s(y, x + 1)      when x < W - 1 (every row, the last included),
 *         s(y + 1, x)      when y < H - 1 (every column, the last included),
 *         s(y + 1, x + 1)  when both.
 *       Pixel (H - 1, W - 1) never is one.  The pixel need not belong to the object: the pixel left of a left edge is a
 *       boundary pixel.  With label planes a pixel can therefore be a boundary pixel of its own object and of the
 *       objects of its three neighbours.
 *   R3  radius.  For bound_th >= 1 the radius is bound_th itself, which must be an integer; otherwise it is
 *       ceil(bound_th * sqrt((double)(H * H + W * W))), all in double (the toolkits' default is 0.008: 480 x 854 gives
 *       8, 1080 x 1920 gives 18, 2160 x 3840 gives 36).  A negative or non-finite bound_th and a radius above
 *       DEVA_VOS_MAX_RADIUS are refused.
 *   R4  match.  A boundary pixel p of object i on one side is matched if the other side has a boundary pixel q of
 *       object i with (qx - px)^2 + (qy - py)^2 <= r^2, in integers: dilation with the disk x^2 + y^2 <= r^2.  Nothing
 *       outside the image ever matches.
 *   R5  record.  counts is uint32 [n_objects][8], initialised by the call:
 *         [0] |gt_i AND pred_i|    [1] |gt_i|                [2] |pred_i|
 *         [3] boundary pixels of gt_i                        [4] boundary pixels of pred_i
 *         [5] matched boundary pixels of gt_i                [6] matched boundary pixels of pred_i
 *         [7] 0
 *       Integer adds: the result is exact and does not depend on the order of the adds.
 *   R6  (host arithmetic, deva/inference/vos_quality.py)  J = [0] / ([1] + [2] - [0]), 1 for an empty union;
 *       precision = [6] / [4], recall = [5] / [3] with (1, 0) for no predicted boundary, (0, 1) for no ground-truth
 *       boundary, (1, 1) for neither; F = 2 P R / (P + R), 0 when P + R = 0.
 *
 * Refused before any launch: an unknown encoding (ground truth: U8 or I32; prediction: U8, I32, I64, INDEX16; either
 * with DEVA_VOS_BINARY); n_objects outside 1 .. 64; DEVA_VOS_BINARY with n_objects != 1; a radius outside
 * 0 .. DEVA_VOS_MAX_RADIUS; height or width < 1 or H * W above 2^30; a null plane, ids, scratch or counts; a null
 * pred_lut or channels outside 1 .. 32767 with INDEX16; a plane or scratch that is not 16-byte aligned, an ids or
 * counts that is not 4-byte aligned, a pred_lut that is not 2-byte aligned; scratch_bytes below
 * deva_vos_boundary_scratch_bytes; counts overlapping any input or the scratch.
 *
 * Two launches.  The first reads both planes once, finds every pixel's slot (the id table in LDS, or pred_lut), forms
 * the two boundary words of R2 from the pixel and its E / S / SE neighbours, stores them side by side in the scratch
 * (16 bytes per pixel) and adds fields 0 - 2 through a per-workgroup table in LDS.  The second gives every wave 64
 * consecutive pixels; a lane whose words are not both zero searches the box of radius inner_radius of the disk of R4 by
 * itself, and for every pixel with a bit still unmatched the wave's 64 lanes search the box of radius
 * DEVA_VOS_MIDDLE_RADIUS and then the whole box together; lane i keeps fields 3 - 6 of object i in registers.  The radius
 * never has to fit anything in LDS.
 *
 * deva_vos_boundary_plan is the launch decision, host only (no device is touched, nothing is dereferenced but `plan`).
 */
#define DEVA_VOS_U8 0
#define DEVA_VOS_I32 1
#define DEVA_VOS_I64 2
#define DEVA_VOS_INDEX16 3
#define DEVA_VOS_BINARY 256

#define DEVA_VOS_MAX_OBJECTS 64
#define DEVA_VOS_MAX_RADIUS 128
#define DEVA_VOS_FIELDS 8
#define DEVA_VOS_STRIP 8
#define DEVA_VOS_INNER_RADIUS 3
#define DEVA_VOS_MIDDLE_RADIUS 8

typedef struct deva_vos_plan {
  uint32_t label_grid;    /* workgroups of the first launch: one lane per strip of DEVA_VOS_STRIP pixels of a row */
  uint32_t match_grid;    /* workgroups of the second launch: a wave per 64 consecutive pixels, at most 1024 */
  uint32_t block;         /* lanes of a workgroup, both launches */
  uint32_t lds_bytes;     /* dynamic LDS of the first launch (the second has 1 KB of its own) */
  int32_t inner_radius;   /* the box every boundary pixel's own lane searches: min(radius, DEVA_VOS_INNER_RADIUS) */
  int32_t radius;
  int64_t scratch_bytes;  /* 16 H W */
} deva_vos_plan;

int deva_vos_boundary_radius(int height, int width, double bound_th, int* radius);
int deva_vos_boundary_scratch_bytes(int height, int width, int64_t* bytes);
int deva_vos_boundary_plan(int height, int width, int n_objects, int radius, deva_vos_plan* plan);
int deva_vos_boundary_counts(const void* gt, int gt_encoding, const void* pred, int pred_encoding, const int32_t* ids,
                             int n_objects, const uint16_t* pred_lut, int channels, int height, int width, int radius,
                             void* scratch, int64_t scratch_bytes, uint32_t* counts, void* stream);

#ifdef __cplusplus
}
#endif
#endif
