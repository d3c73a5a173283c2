"""The K pipeline of the fp32 Winograd kernel (csrc/conv_wino.hip): weights by LDS-DMA, K loop unrolled by two over
compile-time LDS buffers, activations loaded two steps ahead and staged behind the workgroup barrier.

Every case is the smallest shape that still reaches the kernel: the launcher takes a layer only with
ceil(cout / 64) * ceil(batch * ceil(H / 2) * (W / 2) / 64) >= 160 workgroups; batch 1 at 160 x 256 with cout 64 is 10 240
tiles = exactly 160.  Contract as in test_gpu_a_conv.py: fp32 F.conv2d on the CPU, 2e-5 of the output range, guard bands
poisoned with NaN, and the result must NOT be bit-identical to the direct kernels' (the Winograd kernel ran).  The
bit-exact invariants at the end catch a staging or hand-over slip that stays inside 2e-5."""
import os
import zlib

import pytest
import torch

import emu_ops
from deva.hip import ops
from gpu_util import dev, max_err, rand, to_dev
from test_gpu_a_conv import _guarded

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

DRY = os.environ.get('DEVA_TEST_DRYRUN') == '1'  # (the emulated ops have one convolution)


def _blocks(cout, batch, H, W):
    tiles = batch * ((H + 1) // 2) * (W // 2)
    return ((cout + 63) // 64) * ((tiles + 63) // 64)


def _tap_major(pc, w):
    """the same layer with its direct-kernel weights in the tap-major layout ([tap][cin][cout], k-quad interleaved): what
    ops.pack_conv builds when cin is no multiple of 32.  With cin = 32 it picks 32-channel slabs, and ops.conv2d then wants
    BOTH sources to be multiples of 32 channels -- the (24, 8) pair needs the other layout to be callable at all"""
    cout, cin = w.shape[:2]
    packed = torch.zeros(9 * cin, pc.cout_pad)
    packed[:, :cout] = w.permute(2, 3, 1, 0).reshape(9 * cin, cout)
    packed = packed.view(9 * cin // 4, 4, pc.cout_pad).permute(0, 2, 1).contiguous().view(9 * cin, pc.cout_pad)
    return ops.PackedConv(packed, pc.bias, pc.cin, pc.cout, pc.cout_pad, 3, 3, ops.KLAYOUT_TAP_MAJOR | ops.KLAYOUT_Q4,
                          None, None, 0, pc.weight_wino)


def _packs(g, cout, cin, bias=True, tap_major=False):
    w = rand(g, cout, cin, 3, 3, scale=(2.0 / (cin * 9))**0.5)
    b = rand(g, cout, scale=0.1) if bias else None
    pc, pcd = ops.pack_conv(w, b, None, wino=True), ops.pack_conv(w, b, None)
    assert pc.weight_wino is not None
    if tap_major:
        pc, pcd = _tap_major(pc, w), _tap_major(pcd, w)
    return pc, pcd


def _check(name, pcd, pc_dev, pcd_dev, x0, x1, relu_in, residual, act, in_place=False):
    """one call through the Winograd kernel against the CPU convolution and against the direct kernels"""
    want = emu_ops.conv2d(pcd, x0, x1, pad=1, relu_in=relu_in, residual=residual, act=act)
    dx0, dx1 = _guarded(x0), _guarded(x1)
    direct = ops.conv2d(pcd_dev, dx0, dx1, pad=1, relu_in=relu_in, residual=to_dev(residual), act=act)
    if in_place:
        res = _guarded(residual)
        got = ops.conv2d(pc_dev, dx0, dx1, pad=1, relu_in=relu_in, residual=res, act=act, out=res)
        assert got.data_ptr() == res.data_ptr()
    else:
        got = ops.conv2d(pc_dev, dx0, dx1, pad=1, relu_in=relu_in, residual=to_dev(residual), act=act)
    torch.cuda.synchronize()
    assert got.shape == want.shape
    assert not torch.isnan(got).any(), f'{name}: guard-band values leaked into the result'
    if not DRY:
        assert not torch.equal(got, direct), f'{name}: the Winograd kernel did not run (bit-identical to the direct kernels)'
    scale = max(1.0, want.abs().max().item())
    err = max_err(got, want)
    print(f'{name}: max abs err {err:.3e} (|ref|max {scale:.3e})')
    assert err <= 2e-5 * scale, (name, err)


# ---- pipeline depth: ksteps 1 .. 5 (prologue only, one and two steps in flight, odd and even counts under the unroll by
# two) x the four RELU x RES instances of the kernel
@pytest.mark.parametrize('res', [False, True], ids=['nores', 'res'])
@pytest.mark.parametrize('relu_in', [False, True], ids=['plain', 'relu'])
@pytest.mark.parametrize('ctot', [8, 16, 24, 32, 40])
def test_wino_pipeline_depth(ctot, relu_in, res):
    name = f'depth_{ctot}_{int(relu_in)}{int(res)}'
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()) % 100000)
    assert _blocks(64, 1, 160, 256) == 160
    pc, pcd = _packs(g, 64, ctot)
    x = rand(g, 1, ctot, 160, 256)
    residual = rand(g, 1, 64, 160, 256) if res else None
    _check(name, pcd, to_dev(pc), to_dev(pcd), x, None, relu_in, residual, ops.ACT_RELU if ctot == 24 else ops.ACT_NONE)


def test_wino_pipeline_in_place_residual():
    """`out` aliasing the residual, three steps"""
    g = torch.Generator().manual_seed(31)
    pc, pcd = _packs(g, 64, 24)
    _check('in_place', pcd, to_dev(pc), to_dev(pcd), rand(g, 1, 24, 160, 256), None, True, rand(g, 1, 64, 160, 256),
           ops.ACT_NONE, in_place=True)


# ---- two sources: the boundary at each position of the two-deep pipeline; batch 2 at 160 x 128 (the batch offset)
@pytest.mark.parametrize('c0,c1,bcast1', [(8, 8, False), (8, 16, True), (16, 8, False), (24, 8, False)],
                         ids=['8+8', '8+16bcast', '16+8', '24+8'])
def test_wino_two_sources(c0, c1, bcast1):
    name = f'cat_{c0}_{c1}'
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()) % 100000)
    assert _blocks(64, 2, 160, 128) == 160
    pc, pcd = _packs(g, 64, c0 + c1, tap_major=(c0 + c1) % 32 == 0)
    x0 = rand(g, 2, c0, 160, 128)
    x1 = rand(g, 1 if bcast1 else 2, c1, 160, 128)
    _check(name, pcd, to_dev(pc), to_dev(pcd), x0, x1, c0 == 16, None, ops.ACT_NONE)


# ---- ragged edges.  (name, cin, cout, batch, H, W, relu_in, res)
RAGGED = [
    ('cout40', 16, 40, 1, 160, 256, False, True),    # one partial 64-channel block
    ('cout136', 16, 136, 1, 80, 256, True, False),   # a full block, a full block and a ragged one: 3 x 80 workgroups
    ('tiles_10287', 24, 64, 1, 162, 254, False, False),  # 81 x 127 tiles: the last workgroup holds 47
    ('odd_height', 16, 64, 1, 161, 256, False, True),    # a last tile row of one output row
    ('last_column_w4', 16, 64, 300, 34, 4, True, False),  # every tile touches the left or the right edge
]


@pytest.mark.parametrize('case', RAGGED, ids=[c[0] for c in RAGGED])
def test_wino_ragged_edges(case):
    name, cin, cout, batch, H, W, relu_in, res = case
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()) % 100000)
    assert _blocks(cout, batch, H, W) >= 160
    if name == 'tiles_10287':
        assert batch * ((H + 1) // 2) * (W // 2) == 10287 and 10287 % 64 == 47
    pc, pcd = _packs(g, cout, cin)
    x = rand(g, batch, cin, H, W)
    residual = rand(g, batch, cout, H, W) if res else None
    _check(name, pcd, to_dev(pc), to_dev(pcd), x, None, relu_in, residual, ops.ACT_SIGMOID if name == 'cout40' else ops.ACT_NONE)


# ---- bit-exact invariants
def test_wino_relu_on_load_equals_relu_first():
    g = torch.Generator().manual_seed(41)
    pc, _ = _packs(g, 64, 40)
    pc = to_dev(pc)
    x = rand(g, 1, 40, 160, 256)
    a = ops.conv2d(pc, _guarded(x), pad=1, relu_in=True)
    b = ops.conv2d(pc, _guarded(torch.relu(x)), pad=1, relu_in=False)
    torch.cuda.synchronize()
    assert not torch.isnan(a).any() and torch.equal(a, b)


@pytest.mark.parametrize('c0,c1', [(8, 16), (24, 8)])
def test_wino_two_sources_equal_one_concatenated(c0, c1):
    g = torch.Generator().manual_seed(43 + c0)
    pc, _ = _packs(g, 64, c0 + c1, tap_major=(c0 + c1) % 32 == 0)
    pc = to_dev(pc)
    x0, x1 = rand(g, 2, c0, 160, 128), rand(g, 2, c1, 160, 128)
    a = ops.conv2d(pc, _guarded(x0), _guarded(x1), pad=1)
    b = ops.conv2d(pc, _guarded(torch.cat([x0, x1], 1)), pad=1)
    torch.cuda.synchronize()
    assert not torch.isnan(a).any() and torch.equal(a, b)


def test_wino_same_call_repeats_bit_for_bit():
    """the same call twice, and again after an unrelated Winograd call of another shape on the same stream: stale LDS or a
    DMA still in flight across launches would show"""
    g = torch.Generator().manual_seed(47)
    pc, _ = _packs(g, 64, 40)
    pc2, _ = _packs(g, 128, 16)
    pc, pc2 = to_dev(pc), to_dev(pc2)
    x, r = _guarded(rand(g, 1, 40, 160, 256)), to_dev(rand(g, 1, 64, 160, 256))
    y = _guarded(rand(g, 2, 16, 96, 128))
    a = ops.conv2d(pc, x, pad=1, relu_in=True, residual=r).clone()
    b = ops.conv2d(pc, x, pad=1, relu_in=True, residual=r).clone()
    other = ops.conv2d(pc2, y, pad=1)
    c = ops.conv2d(pc, x, pad=1, relu_in=True, residual=r)
    torch.cuda.synchronize()
    assert not torch.isnan(a).any() and not torch.isnan(other).any()
    assert torch.equal(a, b) and torch.equal(a, c)


def test_wino_batch_items_do_not_depend_on_their_position():
    """item 2 of a batch of 3 equals item 1 of the batch of 2 that starts at item 1 (both above the threshold)"""
    g = torch.Generator().manual_seed(53)
    pc, _ = _packs(g, 64, 24)
    pc = to_dev(pc)
    x = rand(g, 3, 24, 160, 256)
    a = ops.conv2d(pc, _guarded(x), pad=1)
    b = ops.conv2d(pc, _guarded(x[1:].contiguous()), pad=1)
    torch.cuda.synchronize()
    assert not torch.isnan(a).any() and torch.equal(a[2], b[1]) and torch.equal(a[1], b[0])
