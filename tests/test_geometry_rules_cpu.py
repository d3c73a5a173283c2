"""Conditions on the INPUTS of the geometry tests, checked without a GPU, and the convolution dispatch policy itself, pinned
at its thresholds.  Every question about what deva_conv2d launches is put to the library (ops.conv_plan ->
deva_conv2d_plan, the function deva_conv2d plans with; csrc/conv_plan.cpp): the generated convolution sweep of
tests/test_gpu_a_conv.py reaches every kernel family on both sides of its rule (so the generator cannot drift into
friendly shapes), the plan agrees with the cases the Winograd tests pin, BOUNDARIES holds one pair of shapes on either
side of each threshold with the expected launch written out by hand, and the arithmetic by which deva_conv2d cuts a
batch whose source spans 2^29 floats into sub-batches (include/deva_hip.h)."""
import math
import os
from collections import Counter
from types import SimpleNamespace

import pytest
import torch

import emu_ops
import test_gpu_a_conv as conv_tests
from deva.hip import CONV_IGEMM_ROW, CONV_IGEMM_VEC, KLAYOUT_CHUNK32, KLAYOUT_TAP_MAJOR, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fp32_launch(case):
    """the fp32 kernel a sweep case runs on, by the library's plan for guard-banded inputs: (kernel, K-slice groups per
    workgroup, global split-K)"""
    cid, family, mode, c0, c1, cout, k, stride, pad, batch, H, W = case[:12]
    launch = ops.conv_plan(c0, c1, cout, k, stride=stride, pad=pad, batch=batch, height=H, width=W).first
    assert launch.family in ('q4', 'cout1_rows', 'cout1_table', 'igemm'), (cid, launch)
    return launch.family if launch.family.startswith('cout1') else f'tile{launch.tile[0]}', launch.wk, launch.splits > 1


def test_the_sweep_reaches_both_sides_of_every_gated_rule():
    cases = conv_tests.SWEEP
    assert 100 <= len(cases) <= 140 and len({c[0] for c in cases}) == len(cases)
    for mode in ('amp', 'split', 'wino'):
        taken = Counter(conv_tests.sweep_takes(c)[mode] for c in cases if c[2] == mode)
        assert taken[True] >= 8 and taken[False] >= 8, (mode, taken)
    # the Winograd rule refuses for each of its reasons: odd width, a pixel count of 4k + 2, width < 4, too few workgroups
    wino = [c for c in cases if c[2] == 'wino' and not conv_tests.sweep_takes(c)['wino']]
    assert any(c[11] % 2 for c in wino) and any(c[11] < 4 for c in wino)
    assert any(c[11] % 2 == 0 and c[11] >= 4 and (c[10] * c[11]) % 4 == 0 for c in wino), 'no case below the 160 workgroups'
    # the crossed options
    assert Counter(c[9] for c in cases).keys() == {1, 3}
    assert {c[14] for c in cases} == {'none', 'full', 'bcast'} and len({c[15] for c in cases}) == 4
    assert sum(c[12] for c in cases) >= 6 and 30 <= sum(c[13] for c in cases) <= 90
    assert sum(c[17] for c in cases) >= 15, 'cases that write through an unaligned output view'
    for cls in conv_tests.GEO_CLASSES:
        assert sum(f'-{cls}-' in c[0] for c in cases) >= 8, cls


def test_the_sweep_reaches_every_fp32_kernel_family():
    """by the library's plan: the three MFMA tiles, 2 and 4 K-slice groups, global split-K on and off, the two
    single-channel kernels and the MFMA tile behind them; both sides of the 128-vs-64 switch on the SAME layer"""
    runs = {c[0]: _fp32_launch(c) for c in conv_tests.SWEEP if c[2] == 'fp32'}
    kernels, wks, splits = Counter(p[0] for p in runs.values()), Counter(p[1] for p in runs.values()), Counter(p[2] for p in runs.values())
    for kernel, least in (('tile32', 8), ('tile64', 8), ('tile128', 6), ('cout1_rows', 2), ('cout1_table', 6)):
        assert kernels[kernel] >= least, (kernel, kernels)
    assert wks[2] >= 4 and wks[4] >= 3 and splits[True] >= 6 and splits[False] >= 20, (wks, splits)
    fam = {f: Counter(runs[c[0]][0] for c in conv_tests.SWEEP if c[1] == f) for f in ('tile128', 'tile128_switch', 'cout1_rows', 'cout1_mfma')}
    assert fam['tile128']['tile128'] >= 6 and fam['tile128_switch'] == Counter(tile64=3), fam
    # 16 384 pixels with a width that is not 4k, and K > 7168 on a small map: the single-channel layer runs on the MFMA tile
    assert fam['cout1_rows']['tile32'] >= 1 and fam['cout1_mfma'] == Counter(tile32=2), fam
    assert Counter(runs[c[0]][2] for c in conv_tests.SWEEP if c[1] == 'splitk')[True] >= 4
    assert Counter(runs[c[0]][2] for c in conv_tests.SWEEP if c[1] == 'no_splitk') == Counter({False: 2})


def test_wino_takes_agrees_with_the_pinned_winograd_cases():
    """every case of WINO_CASES asserts on the GPU that the Winograd kernel ran (not bit-identical to the direct kernels),
    and test_conv_wino_small_layers_stay_on_the_direct_kernels that three shapes do not: the plan must say the same"""
    def takes(c0, c1, cout, batch, H, W):
        pc = SimpleNamespace(kh=3, kw=3, cout=cout, weight_wino=True)
        x0 = torch.empty(batch, c0, H, W, device='meta')
        x1 = torch.empty(batch, c1, H, W, device='meta') if c1 else None
        return emu_ops.wino_takes(pc, x0, x1, 1, 1, batch)
    for name, c0, c1, cout, batch, H, W, *_ in conv_tests.WINO_CASES:
        assert takes(c0, c1, cout, batch, H, W), name
    for shape in ((1, 64, 30, 54), (4, 64, 31, 54), (64, 64, 30, 53)):
        assert not takes(shape[1], 0, 64, shape[0], shape[2], shape[3]), shape


# The thresholds of the dispatch policy (csrc/conv_plan.cpp), one pair of shapes on either side of each.  Expected launches
# are written out BY HAND from the rules (n = batch * OH * OW pixels, tiles = ceil(cout / BM) * ceil(n / BN), K steps =
# ceil(K / 32); split-K aims at 512 workgroups, keeps a floor of K steps per split and at most 16 splits): a change of the
# policy fails here, and its author updates the rows.  Inputs are guard-banded (ops.GUARD), weights k-quad interleaved as
# ops.pack_conv gives them unless a row says otherwise.
# (label, arguments of ops.conv_plan, (family, (BM, BN), K-slice groups, staging kind, splits, K steps per split))
_ROWS, _VEC1X1 = 1, 0  # staging kinds of the q4 / f16 / split families: row reuse (3x3), vector gather (1x1)


def _conv(c0, cout, k, H, W, **kw):
    return dict(dict(c0=c0, c1=0, cout=cout, kh=k, pad=k // 2, height=H, width=W), **kw)


BOUNDARIES = [
    # the issue's example: 18 K steps on one tile -> two K-slice groups; 512 / (1 * 2) splits capped at 18 / (4 * 2) = 2;
    # 9 steps per split rounded up to whole (slab, dy) groups per slice group (3 * 2 = 6): 12
    ('example 64->64 3x3 8x8', _conv(64, 64, 3, 8, 8), ('q4', (64, 64), 2, _ROWS, 2, 12)),
    ('example 64->64 1x1 8x8', _conv(64, 64, 1, 8, 8), ('q4', (64, 64), 1, _VEC1X1, 1, 2)),
    # cout 32 | 33: the 32x128 tile
    ('cout 32', _conv(64, 32, 1, 8, 8), ('q4', (32, 128), 1, _VEC1X1, 1, 2)),
    ('cout 33', _conv(64, 33, 1, 8, 8), ('q4', (64, 64), 1, _VEC1X1, 1, 2)),
    # cout 127 | 128 on 128 x 192 pixels (192 pixel tiles of 128): the 128x128 tile needs cout >= 128
    ('cout 127', _conv(64, 127, 1, 128, 192), ('q4', (64, 64), 1, _VEC1X1, 1, 2)),
    ('cout 128', _conv(64, 128, 1, 128, 192), ('q4', (128, 128), 1, _VEC1X1, 1, 2)),
    # 128-tiles 63 | 64 (cout 128; 8064 and 8128 pixels: 252 and 254 tiles of 64x64, below the 256 that would win)
    ('63 tiles of 128', _conv(64, 128, 1, 8, 1008), ('q4', (64, 64), 1, _VEC1X1, 1, 2)),
    ('64 tiles of 128', _conv(64, 128, 1, 8, 1016), ('q4', (128, 128), 1, _VEC1X1, 1, 2)),
    # 128-tiles 191 | 192: below 192 the 128x128 tiles leave CUs empty where >= 256 tiles of 64x64 fill the chip
    ('191 tiles of 128', _conv(64, 128, 1, 128, 191), ('q4', (64, 64), 1, _VEC1X1, 1, 2)),
    ('192 tiles of 128', _conv(64, 128, 1, 128, 192), ('q4', (128, 128), 1, _VEC1X1, 1, 2)),
    # 128-tiles 256 | 257 with 16 K steps: two K-slice groups up to one tile per CU
    ('256 tiles of 128', _conv(512, 128, 1, 128, 256), ('q4', (128, 128), 2, _VEC1X1, 1, 16)),
    ('257 tiles of 128', _conv(512, 128, 1, 128, 257), ('q4', (128, 128), 1, _VEC1X1, 1, 16)),
    # 64-tiles 208 | 209 (36 K steps): four K-slice groups up to 208 tiles, two up to 512; >= 192 tiles: no split-K
    ('208 tiles of 64', _conv(128, 64, 3, 8, 1664), ('q4', (64, 64), 4, _ROWS, 1, 36)),
    ('209 tiles of 64', _conv(128, 64, 3, 8, 1672), ('q4', (64, 64), 2, _ROWS, 1, 36)),
    # K steps 15 | 16 on one 64x64 tile: 15 -> no slices, 512 splits capped at 15 / 4 = 3 of 5 steps;
    # 16 -> two slice groups, 256 splits capped at 16 / 8 = 2 of 8 steps
    ('15 K steps', _conv(480, 64, 1, 8, 8), ('q4', (64, 64), 1, _VEC1X1, 3, 5)),
    ('16 K steps', _conv(512, 64, 1, 8, 8), ('q4', (64, 64), 2, _VEC1X1, 2, 8)),
    # ... and on the 128x128 tile (192 tiles: no split-K)
    ('15 K steps, 128 tile', _conv(480, 128, 1, 128, 192), ('q4', (128, 128), 1, _VEC1X1, 1, 15)),
    ('16 K steps, 128 tile', _conv(512, 128, 1, 128, 192), ('q4', (128, 128), 2, _VEC1X1, 1, 16)),
    # K steps 31 | 32 on 64 tiles of 64x64: 31 -> two slice groups, 512 / (64 * 2) = 4 splits capped at 31 / 8 = 3 of 11 steps;
    # 32 -> four slice groups, 512 / (64 * 4) = 2 splits of 16 steps
    ('31 K steps', _conv(992, 64, 1, 64, 64), ('q4', (64, 64), 2, _VEC1X1, 3, 11)),
    ('32 K steps', _conv(1024, 64, 1, 64, 64), ('q4', (64, 64), 4, _VEC1X1, 2, 16)),
    # single output channel: the row-reusing 3x3 kernel from 16 384 pixels (a width of 4k: 16 380 = 4095 x 4 is the largest
    # count below), the table kernel below them (kind 0: K <= 512)
    ('cout 1, 16380 pixels', _conv(32, 1, 3, 4095, 4), ('cout1_table', (0, 0), 1, 0, 1, 9)),
    ('cout 1, 16384 pixels', _conv(32, 1, 3, 4096, 4), ('cout1_rows', (0, 0), 1, 0, 1, 9)),
    # the table kernel's own limit, n < 16384, at 16383 | 16384 pixels: 129 x 127 = 16 383 (not 4k pixels: no vector gathers,
    # so not the rows kernel either) -> table kind 0 (K = 288 <= 512), 9 K steps, 256 workgroups of 64 pixels; a 1x1 layer on
    # 128 x 128 = 16 384 pixels is neither kernel's: the 32x128 MFMA tile on plain weights, 1x1 mode + vector gather, 128
    # tiles with one K step: no split-K
    ('cout 1, 16383 pixels', _conv(32, 1, 3, 129, 127), ('cout1_table', (0, 0), 1, 0, 1, 9)),
    ('cout 1, 16384 pixels, 1x1', _conv(32, 1, 1, 128, 128), ('igemm', (32, 128), 1, 0 | CONV_IGEMM_VEC, 1, 1)),
    # ... and the table kernel up to K = 7168 (kind 2: 8 pixels x 32 k-groups); beyond, the 32x128 MFMA tile on plain
    # weights, per-element decode (mode 2): 225 K steps, 16 splits of 15
    ('cout 1, K 7168', _conv(7168, 1, 1, 8, 8), ('cout1_table', (0, 0), 1, 2, 1, 224)),
    ('cout 1, K 7169', _conv(7169, 1, 1, 8, 8), ('igemm', (32, 128), 1, 2, 15, 15)),
    # Winograd: 159 | 160 workgroups of 64 channels x 64 tiles of 2x2 outputs (cout 64, width 128: 64 tiles per row pair)
    ('159 Winograd workgroups', _conv(64, 64, 3, 318, 128, weights=('wino',)), ('q4', (64, 64), 1, _ROWS, 1, 18)),
    ('160 Winograd workgroups', _conv(64, 64, 3, 320, 128, weights=('wino',)), ('wino', (64, 64), 1, 1, 1, 8)),
    # the legacy kernels (plain weights) split below 256 tiles: 36 K steps, 512 / 255 -> 3 splits of 12 (whole dx groups);
    # kind = mode 1 + vector gather + row reuse
    ('legacy, 255 tiles', _conv(128, 64, 3, 8, 2040, k_layout=KLAYOUT_CHUNK32), ('igemm', (64, 64), 1, 1 | CONV_IGEMM_VEC | CONV_IGEMM_ROW, 3, 12)),
    ('legacy, 256 tiles', _conv(128, 64, 3, 8, 2048, k_layout=KLAYOUT_CHUNK32), ('igemm', (64, 64), 1, 1 | CONV_IGEMM_VEC | CONV_IGEMM_ROW, 1, 36)),
    # ... and only from 8 K steps (fewer than 128 tiles): 8 / 4 = 2 splits of 4; kind = mode 0 + vector gather
    ('legacy, 7 K steps', _conv(224, 64, 1, 8, 8, k_layout=KLAYOUT_TAP_MAJOR), ('igemm', (64, 64), 1, 0 | CONV_IGEMM_VEC, 1, 7)),
    ('legacy, 8 K steps', _conv(256, 64, 1, 8, 8, k_layout=KLAYOUT_TAP_MAJOR), ('igemm', (64, 64), 1, 0 | CONV_IGEMM_VEC, 2, 4)),
    # the f16 planner, rule 1: a split keeps 384 channels' worth of K steps, so split-K starts at twice that -- 24 steps of 32
    # for the hi/lo split (2 splits of 12), 12 steps of 64 for fp16 operands (2 splits of 6)
    ('split, 23 K steps', _conv(736, 64, 1, 8, 8, weights=('split',), split=True), ('split', (64, 64), 1, _VEC1X1, 1, 23)),
    ('split, 24 K steps', _conv(768, 64, 1, 8, 8, weights=('split',), split=True), ('split', (64, 64), 1, _VEC1X1, 2, 12)),
    ('amp, 11 K steps', _conv(704, 64, 1, 8, 8, weights=('f16',), amp=True), ('f16', (64, 64), 1, _VEC1X1, 1, 11)),
    ('amp, 12 K steps', _conv(768, 64, 1, 8, 8, weights=('f16',), amp=True), ('f16', (64, 64), 1, _VEC1X1, 2, 6)),
    # ... rule 2: only below 192 tiles
    ('split, 191 tiles', _conv(768, 64, 1, 8, 1528, weights=('split',), split=True), ('split', (64, 64), 1, _VEC1X1, 2, 12)),
    ('split, 192 tiles', _conv(768, 64, 1, 8, 1536, weights=('split',), split=True), ('split', (64, 64), 1, _VEC1X1, 1, 24)),
]


@pytest.mark.parametrize('row', BOUNDARIES, ids=[r[0] for r in BOUNDARIES])
def test_dispatch_policy_at_its_boundaries(row):
    label, args, want = row
    plan = ops.conv_plan(**args)
    first = plan.first
    assert (first.family, first.tile, first.wk, first.kind, first.splits, first.per_split) == want, (label, plan)
    assert first.grid[1] == first.splits and plan.sub_batch == 1 and not plan.aliased
    if first.family == 'cout1_table':  # a wave of pixels (kind 0), 16 (kind 1) or 8 (kind 2) per workgroup
        assert first.grid[0] == math.ceil(args['height'] * args['width'] / {0: 64, 1: 16, 2: 8}[first.kind]), (label, plan)
    if first.tile != (0, 0) and first.family != 'wino':
        n = args['height'] * args['width']
        assert first.grid[0] == math.ceil(args['cout'] / first.tile[0]) * math.ceil(n / first.tile[1]), (label, plan)
        assert first.block == 64 * first.waves * first.wk
    # behind a hi/lo split launch: the gated fp32 re-run, persistent for the kinds the split kernels take
    assert (plan.rerun is not None) == (first.family == 'split')
    if plan.rerun is not None:
        r = plan.rerun
        assert (r.family, r.tile, r.wk, r.kind, r.persistent, r.splits) == ('q4', (64, 64), 1, first.kind, True, 1), (label, plan)
        assert r.grid == (min(first.grid[0], 1024), 1)


# the first batch that is cut, on the decoder's 256-channel 3x3 layers at 1/4 scale: 128x128 tiles, 72 K steps
@pytest.mark.parametrize('H,W,first', [(480, 864, 81), (1088, 1920, 17), (2160, 3840, 5)])
def test_dispatch_policy_at_the_first_cut_batch(H, W, first):
    h, w = H // 4, W // 4
    for batch, sub in ((first - 1, first - 1), (first, first - 1)):
        plan = ops.conv_plan(256, 0, 256, 3, pad=1, batch=batch, height=h, width=w)
        assert plan.sub_batch == sub, (batch, plan)
        l = plan.first  # the launch of the first sub_batch images
        assert (l.family, l.tile, l.wk, l.kind, l.splits, l.per_split) == ('q4', (128, 128), 1, _ROWS, 1, 72)
        assert l.grid == (2 * math.ceil(sub * h * w / 128), 1)


def test_dispatch_policy_of_a_split_call_whose_output_aliases_an_operand():
    """amp == 2 with `out` on top of the residual (an in-place add): the fp32 kernels alone, no gated re-run"""
    args = _conv(768, 64, 1, 8, 8, weights=('split',), split=True, residual=True)
    apart, onto = ops.conv_plan(**args), ops.conv_plan(**args, addresses=dict(residual=4 << 40, out=4 << 40))
    assert apart.family == 'split' and not apart.aliased and apart.rerun is not None
    assert onto.aliased and onto.rerun is None
    # 24 K steps on one 64x64 tile: two K-slice groups, 256 splits capped at 24 / 8 = 3 of 8 steps
    assert (onto.first.family, onto.first.tile, onto.first.wk, onto.first.splits, onto.first.per_split) == ('q4', (64, 64), 2, 3, 8)


SPAN_LIMIT = 1 << 29  # floats one launch of deva_conv2d addresses inside a source (include/deva_hip.h: SIZE LIMITS)


# the decoder's 256-channel maps at 1/4 scale, contiguous over the objects of a pass: floats per object, and the first
# object count whose batch spans 2^29 floats
@pytest.mark.parametrize('H,W,per_object,first', [(480, 864, 6_635_520, 81), (1088, 1920, 33_423_360, 17),
                                                  (2160, 3840, 132_710_400, 5)])
def test_conv_sub_batches_at_the_span_limit(H, W, per_object, first):
    """deva_conv2d addresses a source with 32-bit byte offsets: below 2^29 floats per launch.  From `first` objects per
    pass the library cuts the batch into sub-batches of `first - 1` images; it refuses nothing a frame can produce."""
    h, w = H // 4, W // 4
    hw = h * w
    assert 256 * hw == per_object
    assert math.ceil(SPAN_LIMIT / per_object) == first
    assert emu_ops.conv_sub_batches(first - 1, 256, h, w, per_object) == [first - 1]
    for batch in (first, 2 * first - 1, 200):
        parts = emu_ops.conv_sub_batches(batch, 256, h, w, per_object)
        assert sum(parts) == batch and parts[0] == first - 1 and len(parts) == math.ceil(batch / (first - 1))
        assert all((p - 1) * per_object + 256 * hw < SPAN_LIMIT for p in parts)
    # two sources (the fuser's concatenations): the tighter one decides; a broadcast source (stride 0) never does
    assert emu_ops.conv_sub_batches(first, 256, h, w, per_object, 512, 0) == [first - 1, 1]
    parts = emu_ops.conv_sub_batches(first, 256, h, w, per_object, 512, 2 * per_object)
    assert sum(parts) == first and max(parts) < first - 1
    assert all((p - 1) * 2 * per_object + 512 * hw < SPAN_LIMIT for p in parts)


def test_conv_refuses_only_a_single_image_beyond_the_span_limit():
    """2^21 pixels x 256 channels = 2^29 floats in ONE image: refused, with the library's message, whatever the batch"""
    with pytest.raises(Exception, match='one image of a source spans 2 GiB or more'):
        emu_ops.conv_sub_batches(1, 256, 1 << 11, 1 << 10, 256 << 21)
    with pytest.raises(Exception, match='one image of a source spans 2 GiB or more'):
        emu_ops.conv_sub_batches(3, 256, 1 << 11, 1 << 10, 256 << 21)
    assert emu_ops.conv_sub_batches(1, 255, 1 << 11, 1 << 10, 255 << 21) == [1]
    hdr = open(os.path.join(ROOT, 'include', 'deva_hip.h')).read()
    assert 'sub-batches' in hdr and '2^29 floats' in hdr
