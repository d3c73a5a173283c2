"""The output stage of the fp32 Winograd kernel on all eight waves, and its pinned K-step schedule (csrc/conv_wino.hip).

Output stage: each half of the workgroup (the waves of transform rows 0 - 1 and of rows 2 - 3) finishes eight of a lane's
sixteen output channels -- channels [0, 16) and [32, 48) of a 64-channel block belong to the first half, [16, 32) and
[48, 64) to the second -- and receives the other half's partial sums through LDS.  Schedule: the fragments of a position
pair are requested one MFMA group ahead into the other register set, on both sides of the workgroup barrier.

Helpers and contract of test_gpu_a_conv_wino_pipeline.py: fp32 F.conv2d on the CPU, 2e-5 of the output range, guard bands
poisoned with NaN, the result NOT bit-identical to the direct kernels'.  Every case is the smallest shape that still
reaches the kernel (ceil(cout / 64) * ceil(tiles / 64) >= 160 workgroups)."""
import zlib

import pytest
import torch

from deva.hip import ops
from gpu_util import rand, to_dev
from test_gpu_a_conv import _guarded
from test_gpu_a_conv_wino_pipeline import _blocks, _check, _packs

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()) % 100000)


# ---- the four RELU x RES instances of the kernel, with a bias and without: two K steps, exactly 160 workgroups
@pytest.mark.parametrize('bias', [True, False], ids=['bias', 'nobias'])
@pytest.mark.parametrize('res', [False, True], ids=['nores', 'res'])
@pytest.mark.parametrize('relu_in', [False, True], ids=['plain', 'relu'])
def test_outstage_instances(relu_in, res, bias):
    name = f'inst_{int(relu_in)}{int(res)}{int(bias)}'
    g = _gen(name)
    assert _blocks(64, 1, 160, 256) == 160
    pc, pcd = _packs(g, 64, 16, bias=bias)
    x = rand(g, 1, 16, 160, 256)
    residual = rand(g, 1, 64, 160, 256) if res else None
    _check(name, pcd, to_dev(pc), to_dev(pcd), x, None, relu_in, residual, ops.ACT_NONE)


@pytest.mark.parametrize('act', [ops.ACT_RELU, ops.ACT_SIGMOID, ops.ACT_SQUARE_PLUS_ONE], ids=['relu', 'sigmoid', 'sq1'])
def test_outstage_activations(act):
    """behind bias and residual, in both halves' channels"""
    name = f'act_{act}'
    g = _gen(name)
    pc, pcd = _packs(g, 64, 16)
    _check(name, pcd, to_dev(pc), to_dev(pcd), rand(g, 1, 16, 160, 256), None, False, rand(g, 1, 64, 160, 256), act)


# ---- ragged edges.  (name, c0, c1, cout, batch, H, W, relu_in, res, in_place)
CASES = [
    ('in_place', 16, 0, 64, 1, 160, 256, False, True, True),        # `out` is the residual: every half loads before it stores
    ('in_place_cout72', 16, 0, 72, 1, 80, 256, True, True, True),   # ... with a last cout block of 8 channels
    ('cout72', 16, 0, 72, 1, 80, 256, False, True, False),          # last block: 8 valid channels, all in the first half's rows
    ('cout40', 16, 0, 40, 1, 160, 256, False, True, False),         # one block: [0, 16) + [32, 40) first half, [16, 32) second
    ('cout88', 16, 0, 88, 1, 80, 256, True, False, False),          # last block: [0, 16) first half, [16, 24) second
    ('tiles_10287', 16, 0, 64, 1, 162, 254, False, True, False),    # 81 x 127 tiles: the last workgroup holds 47
    ('odd_height', 16, 0, 64, 1, 161, 256, True, True, False),      # a last tile row of one output row, in both halves' rows
    ('odd_height_cout40', 16, 0, 40, 1, 161, 256, False, False, False),
    ('width4', 16, 0, 64, 300, 34, 4, False, True, False),          # every tile touches the left or the right edge
    ('two_sources', 24, 16, 64, 2, 160, 128, True, True, False),    # the boundary inside the loop (steps 0 - 2 | 3 - 4)
]


@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
def test_outstage_ragged(case):
    name, c0, c1, cout, batch, H, W, relu_in, res, in_place = case
    g = _gen(name)
    assert _blocks(cout, batch, H, W) >= 160
    if name == 'tiles_10287':
        assert batch * ((H + 1) // 2) * (W // 2) == 10287 and 10287 % 64 == 47
    pc, pcd = _packs(g, cout, c0 + c1)
    x0 = rand(g, batch, c0, H, W)
    x1 = rand(g, batch, c1, H, W) if c1 else None
    residual = rand(g, batch, cout, H, W) if res else None
    _check(name, pcd, to_dev(pc), to_dev(pcd), x0, x1, relu_in, residual, ops.ACT_NONE, in_place=in_place)


# ---- the pinned schedule, deep: 64 K steps at the minimal shape, twice.  A fragment read that races the staging of the
# tile after next shows as a difference between the runs (or against the CPU)
def test_schedule_deep_64_steps_twice():
    g = _gen('deep512')
    assert _blocks(64, 1, 160, 256) == 160
    pc, pcd = _packs(g, 64, 512)
    x = rand(g, 1, 512, 160, 256)
    pc_dev, pcd_dev = to_dev(pc), to_dev(pcd)
    _check('deep512', pcd, pc_dev, pcd_dev, x, None, False, None, ops.ACT_NONE)
    dx = _guarded(x)
    a = ops.conv2d(pc_dev, dx, pad=1).clone()
    b = ops.conv2d(pc_dev, dx, pad=1)
    torch.cuda.synchronize()
    assert not torch.isnan(a).any() and torch.equal(a, b)


# ---- bit-exact invariants
@pytest.mark.parametrize('relu_in', [False, True], ids=['plain', 'relu'])
def test_residual_equals_residual_added_afterwards(relu_in):
    """(partial + partial) + bias + residual: the call with a residual is the call without it plus the residual in fp32"""
    g = _gen(f'res_after_{int(relu_in)}')
    pc, _ = _packs(g, 72, 24)
    pc = to_dev(pc)
    assert _blocks(72, 1, 80, 256) == 160
    x, r = _guarded(rand(g, 1, 24, 80, 256)), to_dev(rand(g, 1, 72, 80, 256))
    a = ops.conv2d(pc, x, pad=1, relu_in=relu_in, residual=r)
    b = ops.conv2d(pc, x, pad=1, relu_in=relu_in) + r
    torch.cuda.synchronize()
    assert not torch.isnan(a).any() and torch.equal(a, b)


def test_cout72_equals_its_first_64_filters_alone():
    """a partial last cout block changes nothing in the full one (both calls above the workgroup threshold)"""
    g = _gen('cout72_vs_64')
    w = rand(g, 72, 16, 3, 3, scale=(2.0 / (16 * 9))**0.5)
    bias = rand(g, 72, scale=0.1)
    pc72 = to_dev(ops.pack_conv(w, bias, None, wino=True))
    pc64 = to_dev(ops.pack_conv(w[:64].contiguous(), bias[:64].contiguous(), None, wino=True))
    assert pc72.weight_wino is not None and pc64.weight_wino is not None
    assert _blocks(64, 1, 160, 256) >= 160
    x, r = _guarded(rand(g, 1, 16, 160, 256)), to_dev(rand(g, 1, 72, 160, 256))
    a = ops.conv2d(pc72, x, pad=1, residual=r)
    b = ops.conv2d(pc64, x, pad=1, residual=r[:, :64].contiguous())
    torch.cuda.synchronize()
    assert not torch.isnan(a).any() and torch.equal(a[:, :64], b)
