"""Conditions on the INPUTS of the geometry tests, checked without a GPU: the generated convolution sweep of
tests/test_gpu_a_conv.py reaches every kernel family on both sides of its rule (so the generator cannot drift into
friendly shapes), the Winograd predicate of tests/emu_ops.py agrees with the cases the Winograd tests already pin, and the
arithmetic by which deva_conv2d cuts a batch whose source spans 2^29 floats into sub-batches (include/deva_hip.h)."""
import math
import os
import re
from collections import Counter
from types import SimpleNamespace

import pytest
import torch

import emu_ops
import test_gpu_a_conv as conv_tests

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'tracking-anything-with-deva_amd', 'csrc')


def _fp32_policy(case):
    """the fp32 kernel a sweep case runs on, restated from deva_conv2d (csrc/conv_igemm.hip) and launch_conv_q4 /
    launch_tile_q4 (csrc/conv_mfma.hip) for guard-banded inputs: (kernel, K-slice groups per workgroup, global split-K)"""
    cid, family, mode, c0, c1, cout, k, stride, pad, batch, H, W = case[:12]
    oh, ow = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    n, ctot = batch * oh * ow, c0 + c1
    K = k * k * ctot
    ksteps = math.ceil(K / 32)
    vec_ok = stride == 1 and (oh, ow) == (H, W) and (oh * ow) % 4 == 0 and ow >= 4
    if cout == 1:
        if vec_ok and k == 3 and pad == 1 and ow % 4 == 0 and n >= 16384 and ctot <= 1024:
            return 'cout1_rows', 1, False
        if K <= 7168 and n < 16384:
            return 'cout1_table', 1, False
    vec_kind = vec_ok and c0 % 32 == 0 and (k == 1 or (ctot % 32 == 0 and k == 3 and pad == 1))
    b128, b64 = math.ceil(cout / 128) * math.ceil(n / 128), math.ceil(cout / 64) * math.ceil(n / 64)
    if cout <= 32:
        tile, wk, blocks = 32, 1, math.ceil(n / 128)
    elif cout >= 128 and b128 >= 64 and not (b128 < 192 and b64 >= 256):
        tile, wk, blocks = 128, (2 if vec_kind and b128 <= 256 and ksteps >= 16 else 1), b128
    else:
        wk = 4 if (ksteps >= 32 and 64 <= b64 <= 208) else 2 if ((ksteps >= 16 and b64 <= 208) or (ksteps >= 32 and b64 <= 512)) else 1
        tile, blocks = 64, b64
    split = False
    if blocks < 192 and ksteps >= (32 if blocks >= 128 else 8):
        split = min(math.ceil(512 / (blocks * wk)), ksteps // (4 * wk), 16) >= 2
    return f'tile{tile}', wk, split


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
    """by the restated policy: the three MFMA tiles, 2 and 4 K-slice groups, global split-K on and off, the two
    single-channel kernels and the MFMA tile behind them; both sides of the 128-vs-64 switch on the SAME layer"""
    runs = {c[0]: _fp32_policy(c) for c in conv_tests.SWEEP if c[2] == 'fp32'}
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
    and test_conv_wino_small_layers_stay_on_the_direct_kernels that three shapes do not: the predicate must say the same"""
    def takes(c0, c1, cout, batch, H, W):
        pc = SimpleNamespace(kh=3, kw=3, cout=cout, weight_wino=True)
        x0 = torch.empty(batch, c0, H, W, device='meta')
        x1 = torch.empty(batch, c1, H, W, device='meta') if c1 else None
        return emu_ops.wino_takes(pc, x0, x1, 1, 1, batch)
    for name, c0, c1, cout, batch, H, W, *_ in conv_tests.WINO_CASES:
        assert takes(c0, c1, cout, batch, H, W), name
    for shape in ((1, 64, 30, 54), (4, 64, 31, 54), (64, 64, 30, 53)):
        assert not takes(shape[1], 0, 64, shape[0], shape[2], shape[3]), shape
    src = open(os.path.join(CSRC, 'conv_wino.hip')).read()
    assert re.search(r'const int min_blocks = 160;', src) and re.search(r'constexpr int WM = 64, WN = 64;', src)


# the decoder's 256-channel maps at 1/4 scale, contiguous over the objects of a pass: floats per object, and the first
# object count whose batch spans 2^29 floats
@pytest.mark.parametrize('H,W,per_object,first', [(480, 864, 6_635_520, 81), (1088, 1920, 33_423_360, 17),
                                                  (2160, 3840, 132_710_400, 5)])
def test_conv_sub_batches_at_the_span_limit(H, W, per_object, first):
    """deva_conv2d addresses a source with 32-bit byte offsets: below 2^29 floats per launch.  From `first` objects per
    pass the library cuts the batch into sub-batches of `first - 1` images; it refuses nothing a frame can produce."""
    hw = (H // 4) * (W // 4)
    assert 256 * hw == per_object
    assert math.ceil(emu_ops.CONV_SPAN_LIMIT / per_object) == first
    assert emu_ops.conv_sub_batches(first - 1, 256, hw, per_object) == [first - 1]
    for batch in (first, 2 * first - 1, 200):
        parts = emu_ops.conv_sub_batches(batch, 256, hw, per_object)
        assert sum(parts) == batch and parts[0] == first - 1 and len(parts) == math.ceil(batch / (first - 1))
        assert all((p - 1) * per_object + 256 * hw < emu_ops.CONV_SPAN_LIMIT for p in parts)
    # two sources (the fuser's concatenations): the tighter one decides; a broadcast source (stride 0) never does
    assert emu_ops.conv_sub_batches(first, 256, hw, per_object, 512, 0) == [first - 1, 1]
    parts = emu_ops.conv_sub_batches(first, 256, hw, per_object, 512, 2 * per_object)
    assert sum(parts) == first and max(parts) < first - 1
    assert all((p - 1) * 2 * per_object + 512 * hw < emu_ops.CONV_SPAN_LIMIT for p in parts)


def test_conv_refuses_only_a_single_image_beyond_the_span_limit():
    with pytest.raises(Exception, match='one image of a source'):
        emu_ops.conv_sub_batches(1, 256, 1 << 21, 256 << 21)
    with pytest.raises(Exception, match='one image of a source'):
        emu_ops.conv_sub_batches(3, 256, 1 << 21, 256 << 21)
    assert emu_ops.conv_sub_batches(1, 255, 1 << 21, 255 << 21) == [1]
    # the restated constants and the message are the library's
    src = open(os.path.join(CSRC, 'conv_igemm.hip')).read()
    assert 'const int64_t lim = (1ll << 29) - 1;' in src and emu_ops.CONV_SPAN_LIMIT == 1 << 29
    assert 'one image of a source spans 2 GiB or more' in src
    hdr = open(os.path.join(ROOT, 'include', 'deva_hip.h')).read()
    assert 'sub-batches' in hdr and '2^29 floats' in hdr

