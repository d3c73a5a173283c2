/* C ABI of libdeva_regions.so: connected components of byte planes on the device, and on top of them the clean-up a
 * SAM-style mask generator applies when `min_mask_region_area` is set: fill the small holes of every mask, then drop its
 * small islands (a fifth library next to libdeva_hip.so, libdeva_metrics.so, libdeva_vos_metrics.so and
 * libdeva_pair_metrics.so).  Every entry point is prefixed deva_regions_ and no symbol is defined in any two of the five
 * libraries.
 *
 * All functions that return int return 0 on success and non-zero on failure; the text of the last failure of the
 * calling thread is behind deva_regions_last_error().  Every argument check is made before any launch.  Nothing is
 * allocated and nothing is synchronised: the scratch is the caller's, sized by deva_regions_scratch_bytes.
 */
#ifndef DEVA_REGIONS_H
#define DEVA_REGIONS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DEVA_REGIONS_ABI_VERSION 1

int deva_regions_version(void);
const char* deva_regions_last_error(void);

/* ------------------------------------------------------------------------------------------
 * Labels.
 *
 * deva_regions_label: planes uint8 [n][H][W] -> labels int32 [n][H][W].  A pixel belongs to the labelled kind when
 * (byte != 0) != of_zeros: the mask with of_zeros = 0, its complement with of_zeros = 1.  Connectivity is 8 for either
 * kind.  A pixel of the other kind gets 0; a pixel of the labelled kind gets 1 + the smallest row-major position
 * y * W + x among the pixels of its component.  The labels are not compacted to 1 .. C: in this form a labelling is
 * unique, so any two correct ones agree bit for bit.  `labels` itself is the union-find array: `scratch` is not read
 * and may be null.
 *
 * The clean-up.  tests/region_case.py is the executable statement of the rules.
 *
 * Rules:
 *   R1  planes.  A pixel is mask iff its byte is non-zero.  Every byte of every plane is written back as 0 or 1.
 *   R2  holes pass.  Take the components of the complement, 8-connected; the outer background counts as one.  A
 *       component is small when its area is strictly below min_area.  If none is small the pass changes nothing;
 *       otherwise every small component becomes mask.  So: a ring whose corners only touch diagonally encloses
 *       nothing; a background of fewer than min_area pixels around a frame-filling mask is filled; a full plane is
 *       unchanged, and so is an empty one of at least min_area pixels (a smaller empty plane is one small component
 *       of the complement and fills, as it does in the reference's helper).
 *   R3  islands pass, on the result of R2 (filling a hole can join islands).  Take the components of the mask,
 *       8-connected, small as above.  If none is small the pass changes nothing.  Otherwise all small components are
 *       removed, unless every component is small: then only the largest is kept, among equal areas the one whose
 *       first pixel comes first in row-major order.
 *   R4  changed.  1 iff either pass found a small component, even where the plane ends up equal to its input: a
 *       single island below min_area is "changed" and kept.
 *   R5  records.  int32 [n][8], initialised by the call:
 *         [0] changed   [1] pixels filled by R2   [2] pixels removed by R3   [3] area after
 *         [4] x0  [5] y0  [6] x1  [7] y1   the box after, inclusive; 0, 0, 0, 0 for an empty plane (rule 4 of
 *                                          deva_proposal_batch, deva_hip.h)
 *       Integer adds, minima and maxima: the same record whatever the order of the workgroups.
 *   R6  min_area <= 0 is refused.  n == 0 is a no-op that returns 0.
 *   R7  areas are exact int32 counts (a plane has at most 2^30 pixels).
 *
 * Refused before any launch: height or width < 1 or H * W above 2^30; n < 0 or above DEVA_REGIONS_MAX_PLANES;
 * min_area <= 0; with n > 0 a null planes, labels, records or (clean) scratch; labels, records that are not 4-byte
 * aligned, a scratch that is not 16-byte aligned; a scratch that does not hold one plane (the message names the bytes
 * needed); an output overlapping the planes or the scratch; the scratch overlapping the planes.
 *
 * Scratch.  A plane in flight costs plane_bytes = 2 x round256(4 H W) + 256: its labels, the area of every component in
 * the slot of its first pixel, and the plane's decision words.  deva_regions_clean takes whatever scratch it is given
 * as a budget: planes_per_pass = min(n, scratch_bytes / plane_bytes) planes are cleaned together, and the n planes are
 * walked in ceil(n / planes_per_pass) passes on the one stream, nothing synchronising with the host in between.  The
 * result does not depend on the budget.  deva_regions_scratch_bytes(H, W, n) is n x plane_bytes: one pass.
 *
 * Launches (deva_regions_plan is the decision, host only: no device is touched, nothing is dereferenced but `plan`).
 * Per labelling: a local stage labels tiles of DEVA_REGIONS_TILE x DEVA_REGIONS_TILE pixels in LDS; a border stage
 * unites across the tile edges, diagonal neighbours at tile corners included; a flatten stage points every pixel at
 * its component's first pixel and (clean) counts areas into that pixel's slot.  deva_regions_label is these three.
 * deva_regions_clean runs per pass: init, then for R2 and again for R3 the three stages, a decide stage (is any
 * component small, is any not, the largest) and a rewrite stage (which in R3 also reduces area and box), then the
 * records: 12 launches.  No kernel waits on another workgroup: merging is union-find by atomic minimum, which only
 * ever lowers a label, and whatever needs a finished plane is a launch of its own.
 */
#define DEVA_REGIONS_TILE 32
#define DEVA_REGIONS_FIELDS 8
#define DEVA_REGIONS_MAX_PLANES 65536

/* (a struct tag only: the launch decision's function has the same name, so say `struct deva_regions_plan`) */
struct deva_regions_plan {
  int32_t tile;            /* DEVA_REGIONS_TILE: edge of a tile of the local stage */
  int32_t block;           /* lanes of a workgroup, every launch */
  int32_t tiles_x;         /* ceil(W / tile) */
  int32_t tiles_y;         /* ceil(H / tile) */
  int32_t planes_per_pass; /* min(n, budget / plane_bytes); 0 with n == 0 */
  int32_t passes;          /* ceil(n / planes_per_pass); 0 with n == 0 */
  uint32_t local_grid;     /* workgroups of the local stage of a full pass: one per tile, capped (a grid-stride loop) */
  uint32_t border_grid;    /* of the border stage: a lane per pixel beside a tile edge; 0 when a plane is one tile */
  uint32_t pixel_grid;     /* of flatten, decide and rewrite: a lane per pixel */
  uint32_t reserved;
  int64_t plane_bytes;     /* 2 x round256(4 H W) + 256 */
  int64_t scratch_bytes;   /* planes_per_pass x plane_bytes: what a call with this budget touches */
};

int deva_regions_scratch_bytes(int height, int width, int n, int64_t* bytes);
int deva_regions_plan(int height, int width, int n, int64_t budget_bytes, struct deva_regions_plan* plan);
int deva_regions_label(const uint8_t* planes, int n, int height, int width, int of_zeros, int32_t* labels, void* scratch,
                       int64_t scratch_bytes, void* stream);
int deva_regions_clean(uint8_t* planes, int n, int height, int width, int min_area, int32_t* records, void* scratch,
                       int64_t scratch_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
