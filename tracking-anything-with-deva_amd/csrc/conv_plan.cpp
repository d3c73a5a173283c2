// The convolution dispatch policy: descriptor -> (argument block, plan).  Host code without HIP; every threshold below
// was measured on an MI355X and carries the place it was measured at.  To change the policy, edit here and update the
// boundary table of tests/test_geometry_rules_cpu.py, which pins both sides of each rule.
#include "conv_plan.h"

#include <math.h>
#include <stdlib.h>

#include <algorithm>

namespace deva {
namespace {

constexpr int BK = kConvBK;

int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

#if defined(DEVA_CONV_PROBES) || defined(DEVA_WINO_TUNE)
int env_int(const char* name, int unset) {
  const char* e = getenv(name);
  return e ? atoi(e) : unset;
}
#endif

struct Tile {
  int bm, bn, waves, wk;
};

void set_tile(deva_conv_launch* l, int family, const Tile& t, const ConvArgs& a) {
  l->family = family;
  l->bm = t.bm;
  l->bn = t.bn;
  l->waves = t.waves;
  l->wk = t.wk;
  l->tiles_m = (int)ceil_div(a.cout, t.bm);
  l->tiles_n = (int)ceil_div(a.n_total, t.bn);
}

void set_grid(deva_conv_launch* l) {
  l->grid_x = (unsigned)(l->tiles_m * l->tiles_n);
  l->grid_y = (unsigned)l->splits;
  l->block = (unsigned)(64 * l->waves * l->wk);
}

// Split-K when a layer has too few tiles to fill the 256 CUs (small frames / single objects): partial sums go to the
// caller's workspace, a second kernel reduces them deterministically.  One rule for the three MFMA families; what differs
// between them is in here, and each family keeps its own measured constants.
struct SplitK {
  int64_t target;      // workgroups to aim for
  int64_t tile_limit;  // only layers with fewer tiles split ...
  int min_steps;       // ... and only with at least this many K steps
  int steps_floor;     // K steps every split keeps
  int wk;              // K-slice groups every workgroup already holds
  int quantum;         // per_split is a multiple of this (row reuse: whole (slab, dy) groups of three dx taps per slice group)
};

void plan_splitk(const SplitK& r, const ConvArgs& a, int ksteps, deva_conv_launch* l) {
  l->splits = 1;
  l->per_split = ksteps;
  const int64_t blocks = (int64_t)l->tiles_m * l->tiles_n;
  if (!a.ws || blocks >= r.tile_limit || ksteps < r.min_steps || r.target <= 0) return;
  int64_t sp = ceil_div(r.target, blocks * r.wk);
  if (sp > ksteps / r.steps_floor) sp = ksteps / r.steps_floor;
  if (sp > 16) sp = 16;
  const int64_t fit = a.ws_elems / ((int64_t)a.cout * a.n_total);  // the workspace holds [splits][cout][n_total]
  if (sp > fit) sp = fit;
  if (sp < 2) return;
  // every split owns at least one K step
  int per = (int)ceil_div(ksteps, sp);
  per = (per + r.quantum - 1) / r.quantum * r.quantum;
  sp = ceil_div(ksteps, per);
  if (sp < 2) return;
  l->splits = (int)sp;
  l->per_split = per;
}

bool is_chunk32(const ConvArgs& a) { return (a.k_layout & 0xf) == DEVA_KLAYOUT_CHUNK32; }
bool is_1x1(const ConvArgs& a) { return a.KH == 1 && a.KW == 1; }
bool is_3x3_pad1(const ConvArgs& a) { return a.KH == 3 && a.KW == 3 && a.pad == 1; }

// ---- single output channel: VALU kernels (conv_cout1.hip) -- a dot product per pixel on small maps (shrinkage head,
// CBAM gate), a row-reusing 3x3 kernel on large guard-banded maps (mask-logit head); anything else stays on the MFMA tile
int plan_cout1(const ConvArgs& a, int in_guard_elems, deva_conv_launch* l) {
  const bool rows3x3 = a.cout == 1 && a.vec_ok && is_3x3_pad1(a) && a.OW % 4 == 0 && a.n_total >= 16384 && a.ctot <= 1024 &&
                       (int64_t)in_guard_elems >= a.W + 8;
  if (!rows3x3 && !(a.cout == 1 && a.K <= 7168 && a.n_total < 16384)) return 0;  // 8 bytes of LDS table per reduction index
  l->wk = 1;
  l->waves = 4;
  l->splits = 1;
  l->per_split = (int)ceil_div(a.K, BK);
  l->block = 256;
  l->grid_y = 1;
  if (rows3x3) {
    l->family = DEVA_CONV_COUT1_ROWS;
    l->kind = a.OH % 2 == 0 ? 0 : 1;
    const int strips = l->kind == 0 ? (a.n_total / a.OHW) * (a.OH / 2) * (a.OW / 4) : a.n_total / 4;
    l->grid_x = (unsigned)ceil_div(strips, 64);
    return 0;
  }
  DEVA_REQUIRE(a.ctot < 65536 && a.KH < 256 && a.KW < 256, "deva_conv2d(cout=1): channel / kernel size beyond the 16 / 8-bit table fields");
  l->family = DEVA_CONV_COUT1_TABLE;
  // short reductions: a wave of pixels x 4 k-groups; long ones on small maps: 8 pixels x 32 k-groups (the map is
  // L2-resident, 32-byte runs are fine) so that ~100 k values per thread remain
  l->kind = a.K <= 512 ? 0 : a.n_total >= 8192 ? 1 : 2;
  l->grid_x = (unsigned)ceil_div(a.n_total, l->kind == 0 ? 64 : l->kind == 1 ? 16 : 8);
  return 0;
}

// ---- fp32 Winograd F(2x2, 3x3): big 3x3 stride-1 layers only (conv_wino.hip)
bool plan_wino(const ConvArgs& a, deva_conv_launch* l) {
  if (!a.vec_ok || a.KH != 3 || a.KW != 3 || a.stride != 1 || a.pad != 1 || (a.W & 1) || a.W < 4) return false;  // (odd heights: a last tile row of one output row)
  if (a.c0 % kWinoKC || a.ctot % kWinoKC || a.cout < 32) return false;
  if (a.in0_span >= (1ll << 29) || a.in1_span >= (1ll << 29)) return false;  // 32-bit byte offsets inside a source (buffer loads)
  if (a.res && (int64_t)(a.n_total / a.OHW) * a.res_bs >= (1ll << 29)) return false;  // ... and inside the residual
  const int batch = a.n_total / a.OHW;
  const int n_tiles = batch * ((a.H + 1) / 2) * (a.W / 2);
  const int cout_pad = (a.cout + kWinoBM - 1) / kWinoBM * kWinoBM;
  int by_tiles = (int64_t)batch * a.HW > 16ll * cout_pad;  // activation elements per channel > transformed weights per channel
#if defined(DEVA_CONV_PROBES) || defined(DEVA_WINO_TUNE)  // (`make EXTRA=-DDEVA_WINO_TUNE`: the threshold alone, kernels as shipped)
  static const int min_blocks = env_int("DEVA_WINO_MIN_BLOCKS", 160);
  static const int by_tiles_probe = env_int("DEVA_WINO_BY_TILES", -1);
  if (by_tiles_probe >= 0) by_tiles = by_tiles_probe;
#else
  const int min_blocks = 160;
#endif
  const int64_t blocks = (int64_t)(cout_pad / kWinoBM) * ceil_div(n_tiles, kWinoBN);
  if (blocks < min_blocks) return false;  // one workgroup per CU: fewer than ~2/3 of the CUs and the direct kernels' split-K wins
  l->family = DEVA_CONV_WINO;
  l->bm = kWinoBM;
  l->bn = kWinoBN;
  l->waves = 8;
  l->wk = 1;
  l->kind = by_tiles;
  l->tiles_m = cout_pad / kWinoBM;
  l->tiles_n = (int)ceil_div(n_tiles, kWinoBN);
  l->splits = 1;
  l->per_split = a.ctot / kWinoKC;
  l->grid_x = (unsigned)blocks;
  l->grid_y = 1;
  l->block = 512;
  return true;
}

// ---- opt-in f16 matrix pipes (conv_f16.hip): fp16 operands (a.prec == 1), or the fp32-accurate hi/lo split (a.prec == 2)
bool plan_f16(const ConvArgs& a, deva_conv_launch* l) {
  const int bkh = a.prec == 2 ? 32 : 64;
  if (!a.w16 || !a.vec_ok || a.stride != 1 || a.cout < 64) return false;
  // whole K steps per source; the split 1x1 kind also takes a partial LAST step (the second source's tail, or the only
  // source's: sensory_compress 512 + 1, g4_conv 256 + 1): deva_conv_pack_split pads those weights with zeros
  const bool tail_ok = a.prec == 2 && is_1x1(a) && (a.c1 > 0 ? a.c0 % bkh == 0 : true);
  if (!tail_ok && (a.c0 % bkh || a.c1 % bkh)) return false;
  int kind;
  if (is_1x1(a)) {
    kind = DEVA_CONV_KIND_1X1;
  } else if (is_3x3_pad1(a)) {
    kind = DEVA_CONV_KIND_ROWS;
  } else {
    return false;
  }
  const int64_t blocks128 = ceil_div(a.cout, 128) * ceil_div(a.n_total, 128);
  Tile t = {64, 64, 4, 1};
  if (a.prec == 2) {
    // 128x128 tiles, 8 waves (wave tile 64x32), two workgroups per CU.  Measured against it on the layers of the 480p / 5-object
    // and the 1080p / 11-object frames (tools/convlab, DEVA_SPLIT_TILE in `make PROBES=1` builds; profiles/r05/lab): 256x128
    // tiles (wave tile 128x32, one workgroup per CU) -1..4 %, 128x128 on four waves (wave tile 64x64) +-1 %: under real
    // operand data the kernels run at the chip's power limit (all-zero activations: +25..34 % at an unchanged instruction
    // stream), so fewer LDS bytes per MFMA buy nothing.
    // (few tiles but a long K loop -- the 512 -> 512 3x3 image part of the fusers at 30x54: 52 tiles, 144 steps -- also takes
    // the 128x128 tile: its split-K fills the chip, 45 against 72 us on 64x64 tiles)
    // ... unless the 128x128 tiles would leave a quarter or more of the CUs without a workgroup where 64x64 tiles give every
    // CU one (the batch-1 layers of the key encoder at 1/16 of a 1080p frame: 128 tiles of 128x128)
    const int64_t blocks64 = ceil_div(a.cout, 64) * ceil_div(a.n_total, 64);
    const bool half_empty = blocks128 >= 64 && blocks128 < 192 && blocks64 >= 256;
    if (a.cout >= 128 && !half_empty && (blocks128 >= 64 || (blocks128 >= 32 && a.K >= 128 * 32))) t = {128, 128, 8, 1};
#ifdef DEVA_CONV_PROBES  // `make PROBES=1`: A/B runs of the tile policy (tools/convlab)
    static const int forced = env_int("DEVA_SPLIT_TILE", 0);
    if (forced == 256 && a.cout >= 256) t = {256, 128, 8, 1};
    if (forced == 128 && a.cout >= 128) t = {128, 128, 8, 1};
    if (forced == 1284 && a.cout >= 128) t = {128, 128, 4, 1};
    if (forced == 64) t = {64, 64, 4, 1};
#endif
  } else if (a.cout >= 128 && blocks128 >= 64) {
    t = {128, 128, 8, 1};
  }
  set_tile(l, a.prec == 2 ? DEVA_CONV_SPLIT : DEVA_CONV_F16, t, a);
  l->kind = kind;
  l->group_m = conv_group_m(a.KH * a.KW, a.stride, t.bm, t.bn, (int64_t)l->tiles_m * l->tiles_n);
  // few tiles, long K: deterministic split-K like the fp32 kernels
  const int steps_min = 384 / bkh;  // K steps a split must keep (6 at 64-deep steps)
  plan_splitk({512, 192, 2 * steps_min, steps_min, 1, kind == DEVA_CONV_KIND_ROWS ? 3 : 1}, a, (int)ceil_div(a.K, bkh), l);
  set_grid(l);
  return true;
}

// ---- lean-loop fp32 kernels for weights in the k-quad layout (conv_mfma.hip)
Tile q4_tile(const ConvArgs& a) {
#ifdef DEVA_CONV_PROBES  // `make PROBES=1`: A/B runs of the tile policy (tools/convlab)
  static const int forced = env_int("DEVA_CONV_TILE", 0);
  const bool c64 = a.cout >= 64, c33 = a.cout > 32;
  switch (forced) {
    case 128: if (c64) return {128, 128, 8, 1}; break;
    case 64: if (c33) return {64, 64, 4, 1}; break;
    case 642: if (c33) return {64, 64, 4, 2}; break;
    case 644: if (c33) return {64, 64, 4, 4}; break;
    case 1282: if (c64) return {128, 128, 8, 2}; break;
    case 12864: if (c64) return {128, 64, 4, 1}; break;
    case 64128: if (c33) return {64, 128, 4, 1}; break;
    default: break;
  }
#endif
  if (a.cout <= 32) return {32, 128, 4, 1};
  // Tile policy (warm sweeps over the layers of the 480p frame, tools/convlab/sweep.sh, profiles/r04a):
  //  * 128x128 (8 waves, wave tile 64x32) from 64 tiles up -- unless it would leave most CUs empty while 64x64 tiles
  //    fill the chip; with at most one tile per CU the workgroup carries two K-slice groups (16 waves per CU);
  //  * 64x64 (4 waves) otherwise; layers with few tiles and a long K loop run 2 or 4 K-slice groups per workgroup.
  const int64_t blocks128 = ceil_div(a.cout, 128) * ceil_div(a.n_total, 128);
  const int64_t blocks64 = ceil_div(a.cout, 64) * ceil_div(a.n_total, 64);
  const int ksteps = (int)ceil_div(a.K, BK);
  const bool vec_kind = a.vec_ok && a.c0 % BK == 0 && (is_1x1(a) || (a.ctot % BK == 0 && is_3x3_pad1(a) && is_chunk32(a)));
  if (a.cout >= 128 && blocks128 >= 64 && !(blocks128 < 192 && blocks64 >= 256))
    return {128, 128, 8, (vec_kind && blocks128 <= 256 && ksteps >= 16) ? 2 : 1};
  if (ksteps >= 32 && blocks64 >= 64 && blocks64 <= 208) return {64, 64, 4, 4};
  if ((ksteps >= 16 && blocks64 <= 208) || (ksteps >= 32 && blocks64 <= 512)) return {64, 64, 4, 2};
  return {64, 64, 4, 1};
}

int plan_q4(const ConvArgs& a, deva_conv_launch* l) {
  const bool uniform = a.ctot % BK == 0 && a.c0 % BK == 0;  // tap and source uniform per K step
  int kind;
  if (a.vec_ok && is_1x1(a) && a.c0 % BK == 0) {
    kind = DEVA_CONV_KIND_1X1;
  } else if (a.vec_ok && uniform && is_3x3_pad1(a) && is_chunk32(a)) {  // (every tile has 32-pixel wave columns)
    kind = DEVA_CONV_KIND_ROWS;
  } else if (uniform) {
    kind = DEVA_CONV_KIND_UNIFORM;
  } else {
    kind = DEVA_CONV_KIND_GENERIC;
  }
  DEVA_REQUIRE(!is_chunk32(a) || uniform, "deva_conv2d: 32-channel-slab weights need c0 and c1 to be multiples of 32");
  Tile t = q4_tile(a);
  if (t.bm == 128 && t.wk > 1 && kind >= DEVA_CONV_KIND_UNIFORM) t.wk = 1;  // scalar kinds: no K-slice build at 1024 threads
  set_tile(l, DEVA_CONV_Q4, t, a);
  l->kind = kind;
  const int64_t blocks = (int64_t)l->tiles_m * l->tiles_n;
  const int ksteps = (int)ceil_div(a.K, BK);
  l->group_m = conv_group_m(a.KH * a.KW, a.stride, t.bm, t.bn, blocks);
  // measured (tools/convlab sweep, profiles/r04a): from ~190 tiles up the split (+ its reduction pass) loses; the
  // reduction launch costs ~7 us, so a layer that already has >= 128 tiles is split only when its K loop is long
  SplitK rule = {512, 192, blocks >= 128 ? 32 : 8, 4 * t.wk, t.wk, kind == DEVA_CONV_KIND_ROWS ? 3 * t.wk : 1};
#ifdef DEVA_CONV_PROBES
  static const int forced = env_int("DEVA_CONV_SPLIT_TARGET", -1);  // blocks to aim for; 0 = no split-K at all
  static const int forced_group = env_int("DEVA_CONV_GROUP_M", -1);  // cout tiles per tile-order group; 0 = all
  if (forced_group >= 0) l->group_m = forced_group;
  if (forced >= 0) {
    rule.target = rule.tile_limit = forced;
    rule.min_steps = 0;
  }
#endif
  plan_splitk(rule, a, ksteps, l);
  set_grid(l);
  return 0;
}

// The fp32 re-run behind a split launch, gated on the flag the split kernel raises: persistent 64x64 tiles for the two
// kinds the split kernels take (1x1 and 3x3 stride 1 on guard-banded inputs); false = not one of those, the regular
// kernels run with the gate.  No split-K, no K slices: when the gate opens, the result is the fp32 kernels' in their
// plain K order (bit-identical to every unsplit WK = 1 variant).  What it costs is its dispatch.
bool plan_q4_gated(const ConvArgs& a, deva_conv_launch* l) {
  if (!a.vec_ok || a.cout <= 32 || a.c0 % BK) return false;
  int kind;
  if (is_1x1(a)) {
    kind = DEVA_CONV_KIND_1X1;
  } else if (a.ctot % BK == 0 && is_3x3_pad1(a) && is_chunk32(a)) {
    kind = DEVA_CONV_KIND_ROWS;
  } else {
    return false;
  }
  set_tile(l, DEVA_CONV_Q4, {64, 64, 4, 1}, a);
  l->kind = kind;
  l->persistent = 1;
  l->splits = 1;
  l->per_split = (int)ceil_div(a.K, BK);
  const int64_t tiles = (int64_t)l->tiles_m * l->tiles_n;
  l->group_m = conv_group_m(a.KH * a.KW, a.stride, 64, 64, tiles);
  l->grid_x = (unsigned)(tiles < kPersistMaxWgs ? tiles : kPersistMaxWgs);
  l->grid_y = 1;
  l->block = 256;
  return true;
}

// ---- the round-1 kernel for plain [K][cout_pad] weights (conv_igemm.hip); all tiles run 32-deep K steps
Tile igemm_tile(const ConvArgs& a) {
#ifdef DEVA_CONV_PROBES  // `make PROBES=1`: A/B runs of the tile policy (tools/conv_microbench.py)
  static const int forced = env_int("DEVA_CONV_TILE", 0);
  if (forced == 64 && a.cout > 32) return {64, 64, 4, 1};
  if (forced == 128 && a.cout >= 128) return {128, 128, 8, 1};
#endif
  if (a.cout <= 32) return {32, 128, 4, 1};
  // measured: the 8-wave 128x128 tile beats the 64x64 tile from ~64 tiles up (split-K tops the grid up)
  // ... except where the 128-wide tiles would need split-K while the 64-wide ones fill the chip on their own
  // (1x1 256->1024 on a 30x54 map: 20 vs 29 us)
  const int64_t blocks128 = ceil_div(a.cout, 128) * ceil_div(a.n_total, 128);
  const int64_t blocks64 = ceil_div(a.cout, 64) * ceil_div(a.n_total, 64);
  if (a.cout >= 128 && blocks128 >= 64 && !(blocks128 < 256 && blocks64 >= 256 && a.K <= 512)) return {128, 128, 8, 1};
  return {64, 64, 4, 1};
}

int plan_igemm(const ConvArgs& a, deva_conv_launch* l) {
  int mode;
  if (is_1x1(a) && a.c0 % BK == 0) {
    mode = 0;
  } else if (a.ctot % BK == 0 && a.c0 % BK == 0) {
    mode = 1;
  } else {
    mode = 2;
  }
  DEVA_REQUIRE(a.k_layout != DEVA_KLAYOUT_CHUNK32 || mode == 1, "deva_conv2d: 32-channel-slab weights need c0 and c1 to be multiples of 32");
  set_tile(l, DEVA_CONV_IGEMM, igemm_tile(a), a);
  // (every tile has 32-pixel wave columns, which the row reuse needs)
  const bool row = a.vec_ok && mode == 1 && is_3x3_pad1(a) && a.k_layout == DEVA_KLAYOUT_CHUNK32;
  const bool vec = a.vec_ok && mode != 2;
  l->kind = mode | (vec ? DEVA_CONV_IGEMM_VEC : 0) | (row ? DEVA_CONV_IGEMM_ROW : 0);
  l->group_m = 0;
  const int64_t blocks = (int64_t)l->tiles_m * l->tiles_n;
  // measured on the batch-1 key-encoder layers (profiles/r02d_conv_small_layers.txt): the reduction launch costs
  // ~7 us, so a layer that already has >= 128 tiles is split only when its K loop is long (>= 32 steps)
  SplitK rule = {512, 256, blocks >= 128 ? 32 : 8, 4, 1, row ? 3 : 1};
#ifdef DEVA_CONV_PROBES
  static const int forced = env_int("DEVA_CONV_SPLIT_TARGET", -1);  // 0 = no split-K at all
  if (forced >= 0) rule.target = forced;
#endif
  plan_splitk(rule, a, (int)ceil_div(a.K, BK), l);
  set_grid(l);
  return 0;
}

int validate(const deva_conv_desc* d) {
  DEVA_REQUIRE(d != nullptr, "deva_conv2d: null descriptor");
  DEVA_REQUIRE(d->in0 && d->weight && d->out, "deva_conv2d: null tensor");
  DEVA_REQUIRE(d->c0 > 0 && d->c1 >= 0 && (d->c1 == 0 || d->in1), "deva_conv2d: bad channel split");
  DEVA_REQUIRE(d->batch > 0 && d->height > 0 && d->width > 0 && d->cout > 0, "deva_conv2d: bad shape");
  DEVA_REQUIRE(d->cout_pad % 32 == 0 && d->cout_pad >= d->cout, "deva_conv2d: cout_pad must be cout rounded up to 32");
  DEVA_REQUIRE(d->kh > 0 && d->kw > 0 && d->stride > 0 && d->pad >= 0, "deva_conv2d: bad kernel geometry");
  DEVA_REQUIRE((d->k_layout & ~DEVA_KLAYOUT_Q4) == DEVA_KLAYOUT_TAP_MAJOR || (d->k_layout & ~DEVA_KLAYOUT_Q4) == DEVA_KLAYOUT_CHUNK32,
               "deva_conv2d: unknown k_layout %d", d->k_layout);
  // the single-channel heads (conv_cout1.hip) read column 0 of [K][cout_pad]: deva_conv_pack never interleaves them
  DEVA_REQUIRE(!(d->cout == 1 && (d->k_layout & DEVA_KLAYOUT_Q4)), "deva_conv2d: k-quad interleaved weights need cout > 1");
  DEVA_REQUIRE(d->amp >= 0 && d->amp <= 2, "deva_conv2d: amp must be 0 (fp32), 1 (fp16 operands) or 2 (fp16 hi/lo split)");
  DEVA_REQUIRE(d->amp != 2 || !d->weight_f16 || d->split_flag, "deva_conv2d: the split path needs a device flag (split_flag)");
  return 0;
}

// The vector-gather kernels address their inputs with 32-bit byte offsets from the tensor bases: a batch whose inputs
// span 2 GiB or more (many objects at 4K) runs as consecutive sub-batches.  -> images per launch
int64_t sub_batch(const deva_conv_desc* d) {
  const int64_t hw = (int64_t)d->height * d->width;
  const int64_t lim = (1ll << 29) - 1;
  const int64_t span0 = (int64_t)(d->batch - 1) * d->in0_batch_stride + (int64_t)d->c0 * hw;
  const int64_t span1 = d->c1 ? (int64_t)(d->batch - 1) * d->in1_batch_stride + (int64_t)d->c1 * hw : 0;
  int64_t per = d->batch;
  if ((span0 > lim || span1 > lim) && d->batch > 1) {
    if (d->in0_batch_stride > 0) per = std::min(per, (lim - (int64_t)d->c0 * hw) / d->in0_batch_stride + 1);
    if (d->c1 && d->in1_batch_stride > 0) per = std::min(per, (lim - (int64_t)d->c1 * hw) / d->in1_batch_stride + 1);
  }
  return per >= 1 ? per : d->batch;  // (one image beyond the limit: not cut; the k-quad kernels refuse it below)
}

}  // namespace

deva_conv_desc conv_desc_slice(const deva_conv_desc& d, int64_t b0, int64_t batch) {
  const int64_t oh = (d.height + 2 * d.pad - d.kh) / d.stride + 1, ow = (d.width + 2 * d.pad - d.kw) / d.stride + 1;
  deva_conv_desc sub = d;
  sub.batch = (int32_t)batch;
  sub.in0 = d.in0 + b0 * d.in0_batch_stride;
  if (d.in1) sub.in1 = d.in1 + b0 * d.in1_batch_stride;
  if (d.residual) sub.residual = d.residual + b0 * d.residual_batch_stride;
  sub.out = d.out + b0 * (int64_t)d.cout * oh * ow;
  return sub;
}

int conv_plan(const deva_conv_desc* d, ConvArgs* args, deva_conv_plan* plan) {
  if (const int rc = validate(d)) return rc;
  const int64_t per = sub_batch(d);
  if (per < d->batch) {
    const deva_conv_desc sub = conv_desc_slice(*d, 0, per);
    const int rc = conv_plan(&sub, args, plan);
    plan->sub_batch = (int32_t)per;
    return rc;
  }
  *plan = deva_conv_plan{};
  plan->sub_batch = d->batch;
  ConvArgs& a = *args;
  a.in0 = d->in0;
  a.in1 = d->c1 ? d->in1 : nullptr;
  a.bs0 = d->in0_batch_stride;
  a.bs1 = d->in1_batch_stride;
  a.c0 = d->c0;
  a.c1 = d->c1;
  a.ctot = d->c0 + d->c1;
  a.H = d->height;
  a.W = d->width;
  a.OH = (d->height + 2 * d->pad - d->kh) / d->stride + 1;
  a.OW = (d->width + 2 * d->pad - d->kw) / d->stride + 1;
  DEVA_REQUIRE(a.OH > 0 && a.OW > 0, "deva_conv2d: empty output");
  a.OHW = a.OH * a.OW;
  a.HW = (int64_t)d->height * d->width;
  a.w = d->weight;
  a.bias = d->bias;
  a.cout = d->cout;
  a.cout_pad = d->cout_pad;
  a.k_layout = d->k_layout;
  a.KH = d->kh;
  a.KW = d->kw;
  a.stride = d->stride;
  a.pad = d->pad;
  a.K = d->kh * d->kw * a.ctot;
  const int64_t n_total = (int64_t)d->batch * a.OHW;
  DEVA_REQUIRE(n_total < (1ll << 31) && a.HW < (1ll << 31), "deva_conv2d: tensor too large for 32-bit pixel index");
  a.n_total = (int)n_total;
  a.relu_in = d->relu_in;
  a.res = d->residual;
  a.res_bs = d->residual_batch_stride;
  a.act = d->act;
  a.out = d->out;
  a.tiles_n = 0;
  a.tiles_m = 0;
  a.group_m = 0;
  a.vec_out = a.OHW % 4 == 0 && aligned(d->out, 16) &&
              (!d->residual || (aligned(d->residual, 16) && d->residual_batch_stride % 4 == 0));
  // 4-pixel vector gathers: stride-1 'same' geometry, quads never straddle images, and the caller
  // vouches for readable guard bands around both inputs
  a.vec_ok = (d->stride == 1 && a.OH == a.H && a.OW == a.W && a.OHW % 4 == 0 && a.OW >= 4 &&
              (int64_t)d->in_guard_elems >= (int64_t)d->pad * (a.W + 1) + 4)
                 ? 1
                 : 0;
  a.per_split = 0;
  a.splits = 1;
  a.ws = d->workspace;
  a.ws_elems = d->workspace ? d->workspace_elems : 0;
  a.w16 = d->amp ? d->weight_f16 : nullptr;
  a.prec = a.w16 ? d->amp : 0;
  a.out_scale = 1.0f;
  a.flag = nullptr;
  a.gate = nullptr;
  a.ablate = 0;
  a.in0_span = (int64_t)(d->batch - 1) * a.bs0 + (int64_t)a.c0 * a.HW;
  a.in1_span = a.in1 ? (int64_t)(d->batch - 1) * a.bs1 + (int64_t)a.c1 * a.HW : 0;

  if (const int rc = plan_cout1(a, d->in_guard_elems, &plan->first)) return rc;
  if (plan->first.family) return 0;
  if (d->weight_wino && !a.w16 && a.cout > 1 && plan_wino(a, &plan->first)) return 0;
  deva_conv_launch* fp32 = &plan->first;
  if (a.w16 && a.cout > 1 && a.in0_span < (1ll << 29) && a.in1_span < (1ll << 29)) {
    // opt-in f16 matrix pipes: eligible shapes only, everything else -- and inputs too large for 32-bit buffer offsets --
    // stays on the fp32 kernels
    // amp == 2: the gated fp32 re-run reads in0 / in1 / residual AFTER the split kernel has written `out`.  An output that
    // overlaps one of them (an in-place residual add, say, which is fine on the plain fp32 path: every element is read
    // before it is written by the same thread) would make the re-run add the residual twice: such calls take the fp32
    // kernels directly (include/deva_hip.h)
    if (a.prec == 2) {
      const auto overlaps = [&](const float* q, int64_t elems) {  // (addresses as integers: callers without a device make them up)
        const uintptr_t o0 = reinterpret_cast<uintptr_t>(a.out), q0 = reinterpret_cast<uintptr_t>(q);
        const uint64_t out_bytes = 4ull * d->batch * a.cout * a.OHW;
        return q && elems > 0 && q0 < o0 + out_bytes && o0 < q0 + 4ull * (uint64_t)elems;
      };
      const int64_t res_elems = d->residual ? (int64_t)(d->batch - 1) * a.res_bs + (int64_t)a.cout * a.OHW : 0;
      plan->aliased = overlaps(a.in0, a.in0_span) || overlaps(a.in1, a.in1_span) || overlaps(d->residual, res_elems);
      DEVA_REQUIRE(d->split_scale_log2 >= -120 && d->split_scale_log2 <= 120, "deva_conv2d: split_scale_log2 out of range");
      a.out_scale = ldexpf(1.0f, -d->split_scale_log2);
      a.flag = d->split_flag;
    }
    if (!plan->aliased && plan_f16(a, &plan->first)) {
      if (a.prec != 2) return 0;
      fp32 = &plan->rerun;  // split: the fp32 kernels run behind it, gated on the flag it raises for inputs beyond the fp16 range
    }
  }
  if (fp32 == &plan->first) conv_args_fp32(a);
  if (a.k_layout & DEVA_KLAYOUT_Q4) {
    // buffer addressing: 32-bit byte offsets from the tensor bases
    DEVA_REQUIRE(a.in0_span < (1ll << 29) && a.in1_span < (1ll << 29),
                 "deva_conv2d: one image of a source spans 2 GiB or more (32-bit buffer offsets; larger BATCHES run as sub-batches)");
    if (fp32 == &plan->rerun && plan_q4_gated(a, fp32)) return 0;
    return plan_q4(a, fp32);
  }
  return plan_igemm(a, fp32);
}

}  // namespace deva

extern "C" int deva_conv2d_plan(const deva_conv_desc* d, deva_conv_plan* plan) {
  DEVA_REQUIRE(plan != nullptr, "deva_conv2d_plan: null plan");
  deva::ConvArgs a;
  const int rc = deva::conv_plan(d, &a, plan);
  if (rc) *plan = deva_conv_plan{};  // a refusal leaves no half-written plan
  return rc;
}
