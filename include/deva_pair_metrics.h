/* C ABI of libdeva_pair_metrics.so: the counts behind the unsupervised DAVIS protocol, where the tracker invents its own
 * ids and region similarity J and boundary accuracy F are wanted for EVERY (proposal, ground-truth object) pair of a
 * frame before proposals are assigned to objects (evaluation, not inference; a fourth library next to libdeva_hip.so,
 * libdeva_metrics.so and libdeva_vos_metrics.so).  Every entry point is prefixed deva_pair_ and no symbol is defined in
 * any two of the four libraries.
 *
 * All functions that return int return 0 on success and non-zero on failure; the text of the last failure of the
 * calling thread is behind deva_pair_last_error().  Every argument check is made before any launch.  Nothing is
 * allocated and nothing is synchronised: the scratch is the caller's, sized by deva_pair_scratch_bytes.
 */
#ifndef DEVA_PAIR_METRICS_H
#define DEVA_PAIR_METRICS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DEVA_PAIR_ABI_VERSION 1

int deva_pair_version(void);
const char* deva_pair_last_error(void);

/* ------------------------------------------------------------------------------------------
 * The pair table of one frame.
 *
 * deva_vos_boundary_counts (deva_vos_metrics.h) assumes that object i has the same id on both sides.  Here the two sides
 * have a table each, and what comes out is everything J and F of any (ground-truth object g, proposal p) pair need:
 * two integers per object and side, three per pair.  tests/pair_case.py is the executable statement of the rules.
 *
 * Rules:
 *   P1  slots.  Ground-truth object g is the id gt_ids[g], proposal p is the id pred_ids[p].  Each table is int32 in
 *       device memory: distinct ascending ids in 1 .. 2^31 - 1, 1 .. 64 entries (an unsorted table cannot be seen
 *       from the host: whoever builds it checks it).  The two tables are independent of each other.  A pixel whose
 *       value is in neither table belongs to nothing.  The encodings and their numbers are those of
 *       DEVA_VOS_U8 / I32 / I64 / INDEX16: ground truth U8 or I32, prediction all four.
 *         DEVA_PAIR_INDEX16  int16 [H][W] (prediction only): the tracker's channel plane and pred_lut, uint16
 *                            [channels], from channel to proposal index; several channels may share a proposal; an
 *                            entry >= n_pred, a negative channel and a channel >= channels mean none.  pred_ids is not
 *                            read and may be null.
 *       There is no binary form: DEVA_VOS_BINARY (256) in either encoding is refused.
 *   P2  boundary map: seg2bmap at the mask's own size.  For the boolean plane s of an object, pixel (y, x) is a
 *       boundary pixel if s(y, x) differs from
 *         s(y, x + 1)      when x < W - 1 (every row, the last included),
 *         s(y + 1, x)      when y < H - 1 (every column, the last included),
 *         s(y + 1, x + 1)  when both.
 *       Pixel (H - 1, W - 1) never is one.  The pixel need not belong to the object: the pixel left of a left edge is a
 *       boundary pixel.  With label planes a pixel can therefore be a boundary pixel of its own object and of the
 *       objects of its three neighbours.
 *   P3  radius.  An integer 0 .. DEVA_PAIR_MAX_RADIUS given by the caller (the Python wrapper derives it with
 *       deva_vos_boundary_radius, rule R3 of deva_vos_metrics.h).
 *   P4  match.  A boundary pixel q of ground-truth object g is matched BY PROPOSAL p if p has a boundary pixel q' with
 *       (q'x - qx)^2 + (q'y - qy)^2 <= r^2, in integers: dilation with the disk x^2 + y^2 <= r^2.  A boundary pixel of
 *       proposal p is matched by object g in the same way.  Nothing outside the image ever matches.
 *   P5  records.  Both outputs are initialised by the call; integer adds: exact, and independent of the order.
 *         singles  uint32 [n_gt + n_pred][2], ground truth first:  [0] area   [1] boundary pixels
 *         pairs    uint32 [n_gt][n_pred][4]:
 *           [0] |gt_g AND pred_p|
 *           [1] boundary pixels of gt_g matched by p
 *           [2] boundary pixels of pred_p matched by g
 *           [3] 0
 *       With the same table on both sides, record i of deva_vos_boundary_counts is
 *         { pairs[i][i][0], singles[i][0], singles[n+i][0], singles[i][1], singles[n+i][1], pairs[i][i][1], pairs[i][i][2] }.
 *
 * Refused before any launch: an unknown encoding (ground truth: U8 or I32; prediction: U8, I32, I64, INDEX16; no
 * BINARY); n_gt or n_pred outside 1 .. 64; a radius outside 0 .. DEVA_PAIR_MAX_RADIUS; height or width < 1 or H * W
 * above 2^30; a null plane, gt_ids, scratch, singles or pairs; a null pred_ids without INDEX16; a null pred_lut or
 * channels outside 1 .. 32767 with INDEX16; a plane or scratch that is not 16-byte aligned, a table or output that is
 * not 4-byte aligned, a pred_lut that is not 2-byte aligned; scratch_bytes below deva_pair_scratch_bytes; an output
 * overlapping any input, the scratch or the other output; the scratch overlapping an input.
 *
 * Two launches.  The first reads both planes once, finds every pixel's two slots (the tables in LDS, or pred_lut),
 * forms the two boundary words of P2 and stores them side by side in the scratch (16 bytes per pixel); areas and the
 * joint (g, p) intersection counts go through a per-workgroup table in LDS.  The second gives every wave 64
 * consecutive pixels: a pixel whose words are not both zero ORs the other side's words over the disk of P4 -- by
 * itself when the radius is at most DEVA_PAIR_INNER_RADIUS, else with the wave's 64 lanes together -- and adds 1 to
 * [g][p] for every bit g of its own word and every bit p of the word it saw, through ballots over the objects present
 * among the 64 pixels into a per-workgroup table in LDS.  The search of a pixel never stops early: a pair table needs
 * every proposal in reach, not only the pixel's own object.
 *
 * deva_pair_plan is the launch decision, host only (no device is touched, nothing is dereferenced but `plan`).
 */
#define DEVA_PAIR_U8 0
#define DEVA_PAIR_I32 1
#define DEVA_PAIR_I64 2
#define DEVA_PAIR_INDEX16 3

#define DEVA_PAIR_MAX_OBJECTS 64
#define DEVA_PAIR_MAX_RADIUS 128
#define DEVA_PAIR_SINGLE_FIELDS 2
#define DEVA_PAIR_FIELDS 4
#define DEVA_PAIR_STRIP 8
#define DEVA_PAIR_INNER_RADIUS 3

/* (a struct tag only: the launch decision's function has the same name, so say `struct deva_pair_plan`) */
struct deva_pair_plan {
  uint32_t label_grid;      /* workgroups of the first launch: one lane per strip of DEVA_PAIR_STRIP pixels of a row */
  uint32_t match_grid;      /* workgroups of the second launch: a wave per 64 consecutive pixels, at most 1024 */
  uint32_t block;           /* lanes of a workgroup, both launches */
  uint32_t label_lds_bytes; /* dynamic LDS of the first launch: both tables, the areas, the joint counts */
  uint32_t match_lds_bytes; /* dynamic LDS of the second: boundary pixels of 2 x 64 slots, 2 tables [n_gt][n_pred] */
  int32_t inner_radius;     /* min(radius, DEVA_PAIR_INNER_RADIUS) */
  int32_t wave_search;      /* 1: radius > DEVA_PAIR_INNER_RADIUS, the wave's lanes search a pixel's disk together */
  int32_t radius;
  int64_t scratch_bytes;    /* 16 H W */
};

int deva_pair_scratch_bytes(int height, int width, int64_t* bytes);
int deva_pair_plan(int height, int width, int n_gt, int n_pred, int radius, struct deva_pair_plan* plan);
int deva_pair_counts(const void* gt, int gt_encoding, const int32_t* gt_ids, int n_gt, const void* pred, int pred_encoding,
                     const int32_t* pred_ids, int n_pred, const uint16_t* pred_lut, int channels, int height, int width,
                     int radius, void* scratch, int64_t scratch_bytes, uint32_t* singles, uint32_t* pairs, void* stream);

#ifdef __cplusplus
}
#endif
#endif
