"""pooling / resampling / CBAM / GRU / aggregate kernels against their PyTorch definitions."""
import pytest
import torch

import emu_ops
from deva.hip import ops
from gpu_util import dev, max_err, rand, to_dev

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


def _check(name, got, want, tol=1e-5):
    torch.cuda.synchronize()
    assert got.shape == want.shape, (name, got.shape, want.shape)
    err = max_err(got, want)
    print(f'{name}: max abs err {err:.3e}')
    assert err <= tol * max(1.0, want.abs().max().item()), (name, err)


# (widths that are multiples of 8 take the four-outputs-per-thread kernel, the others the scalar one)
@pytest.mark.parametrize('shape', [(1, 64, 48, 64), (2, 8, 45, 65), (1, 3, 1, 1), (3, 5, 2, 7), (2, 3, 5, 8), (1, 2, 9, 16), (1, 4, 1, 24)])
@pytest.mark.parametrize('relu', [False, True])
def test_maxpool(shape, relu):
    x = rand(torch.Generator().manual_seed(1), *shape)
    _check('maxpool', ops.maxpool3x3s2(to_dev(x), relu), emu_ops.maxpool3x3s2(x, relu), 0)


@pytest.mark.parametrize('shape', [(2, 16, 6, 8), (1, 3, 1, 1), (3, 5, 7, 9), (2, 4, 5, 4), (1, 2, 3, 6), (3, 8, 68, 120), (1, 2, 1, 4)])
@pytest.mark.parametrize('with_skip', [False, True])
def test_upsample2x_add(shape, with_skip):
    g = torch.Generator().manual_seed(2)
    x = rand(g, *shape)
    skip = rand(g, 1, shape[1], 2 * shape[2], 2 * shape[3]) if with_skip else None
    _check('up2x', ops.upsample2x_add(to_dev(x), to_dev(skip)), emu_ops.upsample2x_add(x, skip))


@pytest.mark.parametrize('shape', [(2, 16, 60, 108), (11, 8, 136, 240), (1, 3, 6, 10), (2, 2, 4, 6)])
def test_upsample2x_add_ds2_is_both_kernels_in_one_pass(shape):
    """deva_upsample2x_add_ds2: the x2 up-sampling + skip AND area_downsample(x, 2) of the input from the same loads --
    bit-identical to the two separate launches"""
    g = torch.Generator().manual_seed(sum(shape))
    x = to_dev(rand(g, *shape))
    skip = to_dev(rand(g, 1, shape[1], 2 * shape[2], 2 * shape[3]))
    up, ds = ops.upsample2x_add_ds2(x, skip)
    torch.cuda.synchronize()
    assert torch.equal(up, ops.upsample2x_add(x, skip)) and torch.equal(ds, ops.area_downsample(x, 2))


@pytest.mark.parametrize('shape,f', [((2, 5, 32, 48), 16), ((3, 7, 8, 12), 2), ((2, 1, 8, 12), 4), ((1, 2, 3, 3), 1)])
def test_area_downsample(shape, f):
    x = rand(torch.Generator().manual_seed(3), *shape)
    _check('area', ops.area_downsample(to_dev(x), f), emu_ops.area_downsample(x, f))


@pytest.mark.parametrize('shape,f', [((3, 16, 272, 480), 4), ((2, 8, 120, 216), 4), ((2, 8, 136, 240), 2), ((3, 4, 60, 108), 2),
                                     ((1, 3, 12, 20), 4), ((2, 2, 8, 12), 2), ((5, 480, 864), 16), ((2, 3, 32, 48), 16)])
def test_area_downsample_vector_path_is_bit_identical_to_the_scalar_kernel(shape, f):
    """factors 2 / 4 on aligned rows run 16-byte loads (2 or 4 outputs per thread); same sums in the same order as the
    one-output-per-thread kernel, which an unaligned view of the same data still takes"""
    g = torch.Generator().manual_seed(sum(shape) + f)
    x = rand(g, *shape)
    n = x.numel()
    buf = torch.zeros(n + 8, device=dev())
    buf[4:4 + n] = x.reshape(-1).to(dev())   # 16-byte aligned view -> vector path
    buf2 = torch.zeros(n + 8, device=dev())
    buf2[1:1 + n] = x.reshape(-1).to(dev())  # 4-byte aligned view -> scalar path
    a = ops.area_downsample(buf[4:4 + n].view(*shape), f)
    b = ops.area_downsample(buf2[1:1 + n].view(*shape), f)
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    _check('area', a, emu_ops.area_downsample(x, f))


@pytest.mark.parametrize('k', [1, 3])
@pytest.mark.parametrize('shape', [(1, 256, 120, 216), (3, 64, 60, 108), (2, 5, 14, 22), (1, 3, 6, 10)])
def test_gather_s2_is_the_stride2_convolutions_im2col(shape, k):
    """deva_gather_s2: the taps of a k x k stride-2 convolution as channels (tap-major), exact copies; a 1x1 convolution with
    the weights in [cout][t*C + c] order over it is the stride-2 convolution (checked on the CPU in fp64)"""
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(k + sum(shape))
    x = rand(g, *shape)
    got = ops.gather_s2(to_dev(x), k)
    torch.cuda.synchronize()
    assert torch.equal(got.cpu(), emu_ops.gather_s2(x, k))
    w = rand(g, 8, shape[1], k, k)
    ref = F.conv2d(x.double(), w.double(), stride=2, padding=k // 2)
    via = F.conv2d(got.cpu().double(), w.permute(0, 2, 3, 1).reshape(8, -1, 1, 1).double())
    assert (via - ref).abs().max().item() <= 1e-9 * max(1.0, ref.abs().max().item())


@pytest.mark.parametrize('no', [1, 2, 5])
def test_aggregate_and_softmax(no):
    g = torch.Generator().manual_seed(4)
    logits = rand(g, no, 24, 33, scale=4.0)
    _check('aggregate_sigmoid', ops.aggregate(to_dev(logits), True), emu_ops.aggregate(logits, True), 2e-6)
    prob = torch.rand(no, 24, 33, generator=g)
    prob[0, :3] = 0.0
    prob[0, 3:6] = 1.0  # exercise the clamp
    agg = emu_ops.aggregate(prob)
    _check('aggregate_prob', ops.aggregate(to_dev(prob)), agg, 2e-6)
    onehot = (torch.rand(24, 33, generator=g) * (no + 1)).long()
    onehot = torch.stack([onehot == i + 1 for i in range(no)], 0)
    _check('aggregate_bool', ops.aggregate(to_dev(onehot)), emu_ops.aggregate(onehot), 2e-6)
    _check('softmax_channels', ops.softmax_channels(to_dev(agg)), emu_ops.softmax_channels(agg), 2e-6)


def test_aggregate_without_objects():
    """nothing tracked yet (empty detection round, inference_core.py:196): background-only logits"""
    empty = torch.zeros(0, 24, 33)
    _check('aggregate_empty', ops.aggregate(to_dev(empty)), emu_ops.aggregate(empty), 2e-6)


@pytest.mark.parametrize('c,h,w', [(3, 6, 8), (6, 24, 32), (1, 1, 1), (2, 5, 3)])
def test_upsample4x_softmax(c, h, w):
    x = rand(torch.Generator().manual_seed(5), c, h, w, scale=5.0)
    up, prob = ops.upsample4x_softmax(to_dev(x))
    wup, wprob = emu_ops.upsample4x_softmax(x)
    _check('up4x_logits', up, wup, 2e-6)
    _check('up4x_prob', prob, wprob, 2e-6)
    _, prob2 = ops.upsample4x_softmax(to_dev(x), need_logits=False)
    _check('up4x_prob_only', prob2, wprob, 2e-6)


@pytest.mark.parametrize('b,c,h,w', [(2, 512, 6, 8), (1, 512, 30, 54), (3, 64, 5, 7), (5, 512, 30, 54), (2, 40, 9, 12)])
def test_cbam(b, c, h, w):
    g = torch.Generator().manual_seed(6)
    x = rand(g, b, c, h, w)
    hid = c // 16
    w1, b1 = rand(g, hid, c, scale=c**-0.5), rand(g, hid, scale=0.1)
    w2, b2 = rand(g, c, hid, scale=hid**-0.5), rand(g, c, scale=0.1)
    sp = ops.pack_conv(rand(g, 1, 2, 7, 7, scale=0.2), rand(g, 1, scale=0.1))
    want = emu_ops.cbam(x, w1, b1, w2, b2, sp)
    got = ops.cbam(to_dev(x), to_dev(w1), to_dev(b1), to_dev(w2), to_dev(b2), to_dev(sp))
    _check('cbam', got, want, 1e-5)


@pytest.mark.parametrize('b,c,h,w', [(2, 512, 6, 8), (1, 16, 3, 5)])
def test_gru(b, c, h, w):
    g = torch.Generator().manual_seed(7)
    v, hh = rand(g, b, 3 * c, h, w, scale=2.0), rand(g, b, c, h, w)
    _check('gru', ops.gru_update(to_dev(v), to_dev(hh)), emu_ops.gru_update(v, hh), 2e-6)


@pytest.mark.parametrize('h,w,size,aa', [(720, 1280, (480, 853), True), (1080, 1920, (480, 853), True),
                                         (2160, 3840, (480, 853), True), (240, 320, (480, 640), True),
                                         (720, 1280, (480, 853), False), (97, 131, (50, 203), True),
                                         (480, 854, None, True)])
def test_input_head(h, w, size, aa):
    """uint8 HWC -> normalised, (antialias-)resized CHW vs torchvision's tensor pipeline restated with
    torch (ToTensor + Normalize + F.interpolate(bilinear, antialias))"""
    g = torch.Generator().manual_seed(h + w)
    img = torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8)
    # smooth it a little so that neighbouring pixels correlate like in a photograph
    img = ((img.float() + img.float().roll(1, 0) + img.float().roll(1, 1)) / 3).round().to(torch.uint8)
    want = emu_ops.input_head(img, size, antialias=aa)
    got = ops.input_head(to_dev(img), size, antialias=aa)
    assert tuple(got.shape) == tuple(want.shape)
    _check(f'input_head {h}x{w}->{size} aa={aa}', got, want, 3e-6)
    # fused pad_divide_by: same pixels inside an exactly zero border
    pad = (3, 4, 1, 2)
    padded = ops.input_head(to_dev(img), size, antialias=aa, pad=pad)
    want_p = emu_ops.input_head(img, size, antialias=aa, pad=pad)
    assert tuple(padded.shape) == tuple(want_p.shape)
    assert torch.equal(padded[:, 1:padded.shape[1] - 2, 3:padded.shape[2] - 4], got)
    border = padded.clone()
    border[:, 1:padded.shape[1] - 2, 3:padded.shape[2] - 4] = 0
    assert (border == 0).all()


@pytest.mark.parametrize('dtype', [torch.float32, torch.int64, torch.uint8])
@pytest.mark.parametrize('shape,pad', [((3, 480, 854), (5, 5, 0, 0)), ((1080, 1920), (0, 0, 4, 4)), ((2, 3, 37, 51), (6, 7, 5, 6))])
def test_pad2d_matches_f_pad(dtype, shape, pad):
    """deva_pad2d (one launch) against F.pad with zeros: bit-identical; the path of tensor_utils.pad_divide_by"""
    import torch.nn.functional as F
    from deva.utils.tensor_utils import pad_divide_by
    g = torch.Generator().manual_seed(sum(shape))
    x = (torch.randn(*shape, generator=g) * 50).to(dtype)
    got = ops.pad2d(to_dev(x), pad)
    torch.cuda.synchronize()
    assert got.dtype == dtype and torch.equal(got.cpu(), F.pad(x, pad))
    via, p = pad_divide_by(to_dev(x), 16)
    ref, p_ref = pad_divide_by(x, 16)
    assert p == p_ref and torch.equal(via.cpu(), ref)



# ---------------------------------------------------------------------------------------------------------------------
# Vector-versus-scalar identity (each 16-byte form is "bit-identical, asserted against the scalar
# forms").  The layers of four frames whose 1/16 maps are 30x45, 29x53, 54x30 and 45x80 (tests/test_gpu_m_geometry.py), at
# their object counts: the same data through a 16-byte-aligned view and through a view 4 bytes further on must give
# torch.equal results, and both must meet the emu_ops contract at this file's tolerances.  Every input sits inside a
# buffer filled with +inf on one run and -inf on the other: NaN does not survive fmaxf, so a NaN poison would not show a
# max-pool over-read; an infinity of either sign survives every kernel here as inf or NaN.
FRAMES = [(480, 720, 2), (464, 848, 1), (864, 480, 3), (720, 1280, 2)]
POISONS = [float('inf'), float('-inf')]
_PAD = 4096  # floats of poison on either side of a view (a multiple of 4: the aligned view stays aligned)


def _views(x, poison):
    """(16-byte aligned view, view 4 bytes further on) of the same values on the device, each inside a poisoned buffer"""
    out = []
    for shift in (0, 1):
        buf = torch.full((x.numel() + 2 * _PAD + 4,), poison, device=dev())
        view = buf[_PAD + shift:_PAD + shift + x.numel()].view(*x.shape)
        view.copy_(x)
        assert dev().type == 'cpu' or view.data_ptr() % 16 == 4 * shift
        out.append(view)
    return out


def _identical(name, results, want, tol):
    """results: the same op over differently aligned views of the same data"""
    torch.cuda.synchronize()
    for r in results[1:]:
        assert torch.equal(results[0], r), f'{name}: the vector and the scalar kernel differ'
    for r in results:
        assert bool(torch.isfinite(r).all()), f'{name}: poison from outside the tensor reached the result'
        _check(name, r, want, tol)


@pytest.mark.parametrize('poison', POISONS, ids=['+inf', '-inf'])
@pytest.mark.parametrize('H,W,no', FRAMES)
def test_maxpool_vector_path_is_bit_identical_to_the_scalar_kernel(H, W, no, poison):
    """the value encoder's pool on the stem output (1/2 scale: 240x360, 232x424, 432x240, 360x640 -- widths of 8k, so the
    aligned view runs four outputs per thread), ReLU after it for every other frame"""
    x = rand(torch.Generator().manual_seed(H + W), no, 64, H // 2, W // 2)
    relu = bool(no % 2)
    _identical(f'maxpool {tuple(x.shape)}', [ops.maxpool3x3s2(v, relu) for v in _views(x, poison)],
               emu_ops.maxpool3x3s2(x, relu), 0)


def _up_cases():
    cases = []
    for H, W, no in FRAMES:
        cases.append((no, 256, H // 16, W // 16))  # 1/16 -> 1/8: 30x45 and 29x53 have odd widths (scalar kernel either way)
        cases.append((no, 64, H // 8, W // 8))     # 1/8 -> 1/4: even sizes, also with the fused x0.5 output
    # the quad kernel runs one grid row per plane: up to 65 535 planes
    return cases + [(255, 257, 3, 4), (256, 256, 3, 4)]


@pytest.mark.parametrize('poison', POISONS, ids=['+inf', '-inf'])
@pytest.mark.parametrize('shape', _up_cases(), ids=lambda s: 'x'.join(map(str, s)))
def test_upsample2x_vector_path_is_bit_identical_to_the_scalar_kernel(shape, poison):
    """x2 up-sampling (+ skip, + the fused x0.5 output, + the per-item skip map): the switch looks at `out` and `skip`, not
    at the input -- an offset OUTPUT view (out=) or an offset skip sends the call to the scalar kernel"""
    b, c, h, w = shape
    g = torch.Generator().manual_seed(sum(shape))
    x, skip = rand(g, *shape), rand(g, 1, c, 2 * h, 2 * w)
    want = emu_ops.upsample2x_add(x, skip)
    xa, xo = _views(x, poison)
    sa, so = _views(skip, poison)
    oa, oo = _views(torch.zeros(b, c, 2 * h, 2 * w), poison)
    res = [ops.upsample2x_add(xa, sa), ops.upsample2x_add(xo, sa), ops.upsample2x_add(xa, sa, out=oa),
           ops.upsample2x_add(xa, sa, out=oo), ops.upsample2x_add(xa, so)]
    assert res[2].data_ptr() == oa.data_ptr() and res[3].data_ptr() == oo.data_ptr()
    _identical(f'up2x+skip {shape}', res, want, 1e-5)
    _identical(f'up2x {shape}', [ops.upsample2x_add(xa, None), ops.upsample2x_add(xa, None, out=oo)],
               emu_ops.upsample2x_add(x, None), 1e-5)
    if h % 2 == 0 and w % 2 == 0:
        (ua, da), (uo, do) = ops.upsample2x_add_ds2(xa, sa), ops.upsample2x_add_ds2(xo, sa, out=oo)
        _identical(f'up2x+ds2 {shape}', [ua, uo, res[0]], want, 1e-5)
        _identical(f'ds2 {shape}', [da, do], emu_ops.area_downsample(x, 2), 1e-5)
    if b <= 3:
        skips = rand(g, 2, c, 2 * h, 2 * w)
        index = ops.clip_index([1, 0, 1][:b], 2, dev())
        want_m = torch.cat([emu_ops.upsample2x_add(x[i:i + 1], skips[s:s + 1]) for i, s in enumerate([1, 0, 1][:b])], 0)
        ma, _ = _views(skips, poison)
        _identical(f'up2x+map {shape}', [ops.upsample2x_add_map(xa, ma, index), ops.upsample2x_add_map(xa, ma, index, out=oo)],
                   want_m, 1e-5)
    for buf in (oa, oo):  # what the kernels wrote stayed inside the output views
        flat, off = buf._base, buf.storage_offset()
        assert bool((flat[:off] == poison).all()) and bool((flat[off + buf.numel():] == poison).all())


@pytest.mark.parametrize('poison', POISONS, ids=['+inf', '-inf'])
@pytest.mark.parametrize('H,W,no', FRAMES)
def test_cbam_apply_vector_path_is_bit_identical_to_the_scalar_kernel(H, W, no, poison):
    """the fuser's CBAM at 1/16 (512 channels): pooling, MLP and the 7x7 gate do not look at the alignment; the final
    x + x * scale * sigmoid(gate) runs four pixels per thread on aligned maps of 4k pixels (54x30, 45x80) only"""
    b, c, h, w = no, 512, H // 16, W // 16
    g = torch.Generator().manual_seed(H + W + 6)
    x = rand(g, b, c, h, w)
    hid = c // 16
    w1, b1 = rand(g, hid, c, scale=c**-0.5), rand(g, hid, scale=0.1)
    w2, b2 = rand(g, c, hid, scale=hid**-0.5), rand(g, c, scale=0.1)
    sp = ops.pack_conv(rand(g, 1, 2, 7, 7, scale=0.2), rand(g, 1, scale=0.1))
    args = [to_dev(t) for t in (w1, b1, w2, b2, sp)]
    _identical(f'cbam {(b, c, h, w)}', [ops.cbam(v, *args) for v in _views(x, poison)], emu_ops.cbam(x, w1, b1, w2, b2, sp), 1e-5)


@pytest.mark.parametrize('poison', POISONS, ids=['+inf', '-inf'])
@pytest.mark.parametrize('H,W,no', FRAMES)
def test_gru_gate_vector_path_is_bit_identical_to_the_scalar_kernel(H, W, no, poison):
    """the sensory update at 1/16: values [no, 1536, h, w], state [no, 512, h, w]; either operand off 16 bytes -> scalar"""
    b, c, h, w = no, 512, H // 16, W // 16
    g = torch.Generator().manual_seed(H + W + 7)
    v, hh = rand(g, b, 3 * c, h, w, scale=2.0), rand(g, b, c, h, w)
    (va, vo), (ha, ho) = _views(v, poison), _views(hh, poison)
    _identical(f'gru {(b, c, h, w)}', [ops.gru_update(va, ha), ops.gru_update(vo, ha), ops.gru_update(va, ho)],
               emu_ops.gru_update(v, hh), 2e-6)
