"""Per-frame result kernels (csrc/frame_result.hip) and `FrameResultSaver` on the device.  The channel decision is held
against `ops.index_mask` bit for bit; everything downstream of it (statistics, gray / colour / overlay planes, run
boundaries) is judged from the kernel's own `index` bytes against the CPU contract (tests/emu_frame_result.py), so
that a near-tie label can neither excuse nor hide anything.  With DEVA_TEST_DRYRUN=1 the same code runs on the CPU
contracts."""
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

import emu_frame_result as E
import full_frame_shapes as FS
import gpu_util
from deva.hip import DevaHipError, check, lib, ops
from gpu_util import to_dev

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DRYRUN = os.environ.get('DEVA_TEST_DRYRUN') == '1'
ALL = ('index', 'labels', 'stats', 'color', 'gray', 'blend')


@pytest.fixture(autouse=True)
def _emulated_when_dry(monkeypatch):
    if DRYRUN:
        E.install(monkeypatch)
        monkeypatch.setattr(torch.Tensor, 'cuda', lambda self, *a, **k: self)


def _soft(g, c, h, w):
    p = torch.softmax(torch.randn(c, h, w, generator=g) * 2, dim=0)
    p[:, :3, :5] = 1.0 / c  # exact ties: the first maximum must win
    return p


def _lut(c):
    """ids above 65535 (all three colour bytes in use); every fifth channel has no object (id 0), as the background"""
    return torch.tensor([0] + [0 if i % 5 == 4 else 70000 + 65537 * i + 259 * i for i in range(1, c)], dtype=torch.int64)


def _colors(lut):
    ids = lut.numpy()
    return torch.from_numpy(np.stack([ids % 256, ids // 256 % 256, ids // 65536 % 256], axis=1).astype(np.uint8))


def _inputs(c, h, w, size):
    g = torch.Generator().manual_seed(c * 1000 + h)
    oh, ow = size or (h, w)
    prob, lut = _soft(g, c, h, w), _lut(c)
    image = torch.randint(0, 256, (oh, ow, 3), generator=g, dtype=torch.uint8)
    return prob, lut, _colors(lut), image


# the shape list of test_index_mask_resize_argmax_lut (tests/test_gpu_c_bank.py) plus one that spans many workgroups
SHAPES = [(3, 40, 56, None), (2, 33, 47, (97, 61)), (4, 96, 128, (48, 64)), (1, 8, 8, (20, 20)),
          (6, 120, 216, (270, 480))]


def _check_products(res, c, lut, colors, image, want=ALL):
    index = res.index.cpu()
    made = E.products_from_index(index, c, lut, colors, image, want)
    for name in want:
        got = getattr(res, name).cpu().numpy()
        assert got.dtype == made[name].dtype and got.shape == made[name].shape, name
        assert np.array_equal(got, made[name]), f'{name}: {int((got != made[name]).sum())} elements differ'


@pytest.mark.parametrize('c,h,w,size', SHAPES)
def test_labels_equal_index_mask_and_products_follow_the_index(c, h, w, size):
    prob, lut, colors, image = _inputs(c, h, w, size)
    dprob, dlut = to_dev(prob), to_dev(lut)
    res = ops.frame_result(dprob, size, dlut, color_lut=to_dev(colors), image=to_dev(image), want=ALL)
    assert res.labels.dtype == torch.int64 and torch.equal(res.labels, ops.index_mask(dprob, size, dlut))
    assert res.index.dtype == torch.int16 and torch.equal(res.index.long(), ops.index_mask(dprob, size))
    _check_products(res, c, lut, colors, image)
    if size is None:
        assert int(res.index[:3, :5].abs().sum()) == 0       # exact ties -> channel 0
    # without a table the ids are the channel indices; a subset of the products leaves the others out
    plain = ops.frame_result(dprob, size, want=('index', 'gray', 'stats'))
    assert plain.labels is None and plain.color is None and torch.equal(plain.index, res.index)
    assert torch.equal(plain.gray.cpu(), (res.index.cpu() & 0xff).to(torch.uint8))
    assert torch.equal(plain.stats, res.stats)


@pytest.mark.parametrize('size', [FS.FRAME_PACKED, FS.FRAME_ELEMENTWISE])
def test_grid_stride_takes_a_second_step(size):
    """more 4-pixel groups than the 4096 x 256 threads of the capped grid: the grid-stride loop takes a second step
    with the LDS statistics table carried across it.  (2052, 2048): the packed stores, 1 050 624 groups; (2052, 2050):
    the element-wise stores, 513 groups per row with a 2-pixel last one, 1 052 676 groups"""
    c, h, w = FS.FRAME_PROB
    prob, lut, colors, image = _inputs(c, h, w, size)
    dprob, dlut = to_dev(prob), to_dev(lut)
    res = ops.frame_result(dprob, size, dlut, color_lut=to_dev(colors), image=to_dev(image), want=ALL)
    assert res.labels.dtype == torch.int64 and torch.equal(res.labels, ops.index_mask(dprob, size, dlut))
    assert res.index.dtype == torch.int16 and torch.equal(res.index.long(), ops.index_mask(dprob, size))
    _check_products(res, c, lut, colors, image)
    assert int(res.stats[:, 0].sum()) == size[0] * size[1]
    assert res.stats[:, 3].max() == size[1] - 1 and res.stats[:, 4].max() == size[0] - 1


@pytest.mark.parametrize('size', [(37, 45), (40, 48)])
def test_id_table_shorter_than_the_channels(size):
    """6 channels, ids for the first 4 only: where channel 4 or 5 wins the id is 0 (labels and gray 0, the overlay
    shows the image), the colour plane still carries the channel's colour and the statistics still count it"""
    c = 6
    prob, lut, _, image = _inputs(c, 20, 28, size)
    lut = lut[:4]
    colors = torch.tensor([[0, 0, 0], [10, 20, 30], [40, 50, 60], [70, 80, 90], [101, 111, 121], [131, 141, 151]],
                          dtype=torch.uint8)
    res = ops.frame_result(to_dev(prob), size, to_dev(lut), color_lut=to_dev(colors), image=to_dev(image), want=ALL)
    assert torch.equal(res.labels, ops.index_mask(to_dev(prob), size, to_dev(lut)))
    _check_products(res, c, lut, colors, image)
    index = res.index.cpu().long()
    for ch in (4, 5):
        won = index == ch
        assert int(won.sum()) > 0
        assert int(res.labels.cpu()[won].abs().sum()) == 0 and int(res.gray.cpu()[won].sum()) == 0
        assert torch.equal(res.blend.cpu()[won], image[won])
        assert bool((res.color.cpu()[won] == colors[ch]).all())
        ys, xs = torch.nonzero(won, as_tuple=True)
        assert res.stats[ch].tolist() == [int(won.sum()), int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max())]


def test_more_channels_than_the_index_plane_holds():
    """40 000 channels without the int16 `index` plane: winners at 0, 32767, 32768 and 39999; labels are
    `index_mask`'s, the statistics the contract's (the absent rows against the empty pattern directly), and asking
    for `index` is refused"""
    c, h, w = 40000, 4, 5
    present = torch.tensor([0, 32767, 32768, 39999])
    owner = present[(torch.arange(h * w) * 7 % 20 % 4)].view(h, w)
    prob = torch.full((c, h, w), 0.1 / c)
    prob.scatter_(0, owner[None], 0.9)
    lut = torch.arange(c, dtype=torch.int64) * 3 + 1
    dprob, dlut = to_dev(prob), to_dev(lut)
    res = ops.frame_result(dprob, None, dlut, want=('labels', 'stats'))
    assert res.index is None and torch.equal(res.labels, ops.index_mask(dprob, None, dlut))
    assert torch.equal(res.labels.cpu(), owner * 3 + 1)
    made = E.products_from_index(owner, c, lut, want=('labels', 'stats'))
    stats = res.stats.cpu().numpy()
    assert stats.dtype == np.int32 and stats.shape == (c, 5)
    for ch in present.tolist():
        ys, xs = torch.nonzero(owner == ch, as_tuple=True)
        assert stats[ch].tolist() == [len(ys), int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max())] and len(ys) == 5
    absent = np.ones(c, dtype=bool)
    absent[present.numpy()] = False
    assert np.array_equal(stats[absent], np.tile(np.array([0, E.INT_MAX, E.INT_MAX, -1, -1], dtype=np.int32), (c - 4, 1)))
    assert np.array_equal(stats, made['stats'])
    with pytest.raises(DevaHipError):
        ops.frame_result(dprob, None, dlut, want=('index', 'stats'))


def _poisoned(nbytes, offset, guard=64):
    buf = torch.full((guard + offset + nbytes + guard + 16,), 0xA5, dtype=torch.uint8)
    return to_dev(buf), guard + offset


@pytest.mark.parametrize('c,h,w,size', [(3, 40, 56, None), (2, 33, 47, (97, 61)), (6, 120, 216, (270, 480))])
@pytest.mark.parametrize('shift', [1, 2, 3])
def test_shifted_outputs_give_the_same_bytes_and_keep_their_guard_bands(c, h, w, size, shift):
    """every output plane `shift` elements into a poisoned buffer (index, labels and stats keep their natural alignment,
    the byte planes and the image lose theirs): the element-wise path must write the bytes of the packed one, and
    nothing else"""
    if DRYRUN:
        pytest.skip('raw pointers: needs the library')
    prob, lut, colors, image = _inputs(c, h, w, size)
    oh, ow = size or (h, w)
    dprob, dlut, dcol = to_dev(prob), to_dev(lut), to_dev(colors)
    ref = ops.frame_result(dprob, size, dlut, color_lut=dcol, image=to_dev(image), want=ALL)
    elem = dict(index=2, labels=8, stats=4, color=1, gray=1, blend=1)
    count = dict(index=oh * ow, labels=oh * ow, stats=c * 5, color=oh * ow * 3, gray=oh * ow, blend=oh * ow * 3)
    bufs = {k: _poisoned(count[k] * elem[k], shift * elem[k]) for k in ALL}
    img_buf, img_at = _poisoned(oh * ow * 3, shift)
    img_buf[img_at:img_at + oh * ow * 3] = to_dev(image).view(-1)
    ptr = {k: b.data_ptr() + at for k, (b, at) in bufs.items()}
    check(lib().deva_frame_result(dprob.data_ptr(), c, h, w, oh, ow, dlut.data_ptr(), dlut.numel(), dcol.data_ptr(),
                                  img_buf.data_ptr() + img_at, ptr['index'], ptr['labels'], ptr['stats'], ptr['color'],
                                  ptr['gray'], ptr['blend'], ops._stream()), 'deva_frame_result')
    torch.cuda.synchronize()
    for k, (b, at) in bufs.items():
        host, nbytes = b.cpu(), count[k] * elem[k]
        assert bool((host[:at] == 0xA5).all()) and bool((host[at + nbytes:] == 0xA5).all()), f'{k}: guard band touched'
        want = getattr(ref, k).cpu().contiguous().view(-1).view(torch.uint8)
        assert torch.equal(host[at:at + nbytes], want), f'{k}: bytes differ from the aligned call'


def test_many_channels_and_the_global_table():
    """300 channels at 24 x 40, every channel present (an 8-bit index or a statistics table sized for few objects
    fails here), and 1100 channels at 24 x 48: beyond the 1024 channels of the LDS table the statistics go through
    global atomics and must be the same numbers.  The edge itself: 1024 channels at 32 x 32 (the LDS table at its
    limit, every channel owning one pixel) and 1025 at 25 x 41 (the first global table, on an odd width)"""
    for c, h, w in ((300, 24, 40), (1100, 24, 48), (1024, 32, 32), (1025, 25, 41)):
        owner = torch.arange(h * w).view(h, w) % c
        prob = torch.full((c, h, w), 0.1 / c)
        prob.scatter_(0, owner[None], 0.9)
        lut = torch.arange(c, dtype=torch.int64) * 3
        colors = _colors(lut)
        image = torch.full((h, w, 3), 200, dtype=torch.uint8)
        res = ops.frame_result(to_dev(prob), None, to_dev(lut), color_lut=to_dev(colors), image=to_dev(image), want=ALL)
        assert torch.equal(res.index.cpu().long(), owner)
        _check_products(res, c, lut, colors, image)
        assert int((res.stats[:min(c, h * w), 0] > 0).sum()) == min(c, h * w)
        n, bounds = ops.mask_rle(res.index, c)
        _check_rle(res.index.cpu(), c, n, bounds)


# ------------------------------------------------------------------------------------------ run boundaries
def _check_rle(index, channels, n, bounds, strings=True, fast=False):
    """`strings`: True decodes every channel's COCO string, a list only those channels (the decoder is a Python loop);
    `fast`: the vectorised reference, for tables of thousands of channels"""
    from deva.inference.frame_results import rle_strings
    if fast:
        want_n, want_b = E.rle_bounds_fast(index, channels)
    else:
        want_n, want_b = E.rle_bounds(index, channels)
        want_b = np.concatenate(want_b)
    n, bounds = n.cpu().numpy(), bounds.cpu().numpy()
    assert n.dtype == np.int32 and bounds.dtype == np.int32
    assert np.array_equal(n, want_n), (n[:8], want_n[:8])
    assert np.array_equal(bounds, want_b), f'{int((bounds != want_b).sum())} of {bounds.size} boundaries differ'
    if strings:
        h, w = index.shape
        texts = rle_strings(n, bounds, h * w)
        for c in (range(1, channels) if strings is True else strings):
            got = E.coco_decode({'size': [h, w], 'counts': texts[c]})
            assert np.array_equal(got, index.numpy() == c), c


def _planes(h, w):
    """hand-built index planes -> (name, int16 [h,w] tensor, channels)"""
    z = lambda: torch.zeros(h, w, dtype=torch.int16)
    yy, xx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing='ij')
    out = []
    p = z(); p[0, 0] = 1; p[h - 1, w - 1] = 2; p[h // 2, w // 2] = 4                          # channel 3 absent
    out.append(('first, last and a single pixel; an absent channel between present ones', p, 5))
    p = z(); p[:3, 0] = 2; p[h - 2:, w - 1] = 2
    out.append(('one object owning p = 0 and the last position', p, 3))
    out.append(('a full-frame object', torch.full((h, w), 1, dtype=torch.int16), 2))
    out.append(('vertical 1-pixel stripes of two objects', (1 + xx % 2).to(torch.int16), 3))
    out.append(('horizontal 1-pixel stripes of two objects', (1 + yy % 2).to(torch.int16), 3))
    # two objects alternating along the scan order p = x*h + y (the (x + y) % 2 checkerboard when h is odd; with an even h
    # the columns are offset so that the label also changes at every column wrap): 2*h*w - 1 boundaries
    out.append(('checkerboard of two objects, no background', (1 + (xx * h + yy) % 2).to(torch.int16), 3))
    p = z(); p[:, w // 8: w - w // 8] = 1; p[h // 3, :] = 2
    out.append(('a band much wider than one workgroup range, cut by a row of another object', p, 3))
    p = z(); p[:, 1:w - 1] = 3
    out.append(('one run crossing every workgroup boundary', p, 4))
    return out


@pytest.mark.parametrize('h,w', [(33, 47), (270, 480)])
def test_run_boundaries_of_hand_built_planes(h, w):
    for name, plane, channels in _planes(h, w):
        n, bounds = ops.mask_rle(to_dev(plane), channels)
        _check_rle(plane, channels, n, bounds)
        if 'checkerboard' in name:
            assert int(n.sum()) == 2 * h * w - 1, name   # the capacity worst case to within one
        if 'full-frame' in name:
            assert n.tolist() == [0, 1] and bounds.tolist() == [0]
    # the default channel count is max + 1
    n, _ = ops.mask_rle(to_dev(_planes(h, w)[0][1]))
    assert n.numel() == 5


@pytest.mark.parametrize('k', range(8))
@pytest.mark.parametrize('h,w', [FS.RLE_TWO_ENTRIES[:2], FS.RLE_PARTIAL_CHUNK[:2]])
def test_run_boundaries_with_several_table_entries_per_thread(h, w, k):
    """the hand-built planes at 300 x 480 (282 ranges: two table entries per scan thread, 115 idle threads) and at
    526 x 750 (771 ranges: four entries, thread 192 with a partial chunk of three, 63 idle threads); one case per
    plane.  The run crossing every boundary leaves ranges without a boundary between ranges that have one; the
    checkerboard has one at every position, so any wrong prefix offset moves a checked boundary"""
    planes = _planes(h, w)
    assert len(planes) == 8
    name, plane, channels = planes[k]
    n, bounds = ops.mask_rle(to_dev(plane), channels)
    _check_rle(plane, channels, n, bounds)
    if 'checkerboard' in name:
        assert int(n.sum()) == 2 * h * w - 1, name
    if 'crossing' in name:
        assert n.tolist() == [0, 0, 0, 2] and bounds.tolist() == [h, (w - 1) * h]


def _scan_order(h, w):
    yy, xx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing='ij')
    return xx * h + yy


def test_run_boundaries_of_a_full_table_on_a_grown_range():
    """544 x 1000 with 4096 channels: 945 ranges of 576 positions instead of 512, four table entries per scan thread,
    4096 scan workgroups.  The label changes every 131 positions of the scan order (131 is prime to 64 and to 576: run
    ends fall on every lane and cross range ends); the 4153 runs wrap past 4096, so every channel is present and
    1..56 twice (the second run of 56 reaches the end of the plane: three boundaries, not four)"""
    h, w = FS.RLE_GROWN_RANGE[:2]
    channels = FS.RLE_GROWN_CHANNELS
    plane = ((_scan_order(h, w) // 131) % channels).to(torch.int16)
    n, bounds = ops.mask_rle(to_dev(plane), channels)
    _check_rle(plane, channels, n, bounds, strings=[1, 30, 56, 57, 4095], fast=True)
    assert n[0] == 0 and n[1:56].tolist() == [4] * 55 and n[56] == 3 and n[57:].tolist() == [2] * (channels - 57)
    p = torch.zeros(h, w, dtype=torch.int16)
    p[:, 1:w - 1] = channels - 1
    n, bounds = ops.mask_rle(to_dev(p), channels)
    _check_rle(p, channels, n, bounds, strings=[1, channels - 1], fast=True)
    assert int(n.sum()) == 2 and bounds.tolist() == [h, (w - 1) * h]


def test_values_outside_the_table_are_no_object():
    """-1, -32768, `channels` and 32767 in the plane, next to objects, to the background and to each other: the result
    is that of the plane with those values replaced by 0"""
    h, w, channels = 19, 23, 5
    g = torch.Generator().manual_seed(7)
    clean = torch.randint(0, channels, (h, w), generator=g).to(torch.int16)
    clean[:, 5:9] = 0
    hit = torch.rand(h, w, generator=g) < 0.3
    hit[:4, :] = True      # (a block of nothing but out-of-table values of all four kinds)
    outside = torch.tensor([-1, -32768, channels, 32767], dtype=torch.int16)[torch.randint(0, 4, (h, w), generator=g)]
    bad = torch.where(hit, outside, clean)
    clean = torch.where(hit, torch.zeros_like(clean), clean)
    assert all(bool((bad == v).any()) for v in outside.unique().tolist())
    n, bounds = ops.mask_rle(to_dev(bad), channels)
    n0, bounds0 = ops.mask_rle(to_dev(clean), channels)
    assert torch.equal(n, n0) and torch.equal(bounds, bounds0) and int(n.sum()) > 100
    _check_rle(clean, channels, n, bounds)
    _check_rle(bad, channels, n, bounds, strings=False)


@pytest.mark.parametrize('h,w', [(1, 700), (700, 1), (1, 1)])
def test_run_boundaries_of_planes_one_pixel_high_or_wide(h, w):
    g = torch.Generator().manual_seed(h + 2 * w)
    plane = torch.randint(0, 4, (h, w), generator=g).to(torch.int16)
    plane.view(-1)[0], plane.view(-1)[-1] = 2, 2     # (the first and the last position belong to an object)
    n, bounds = ops.mask_rle(to_dev(plane), 4)
    _check_rle(plane, 4, n, bounds)
    if h * w == 1:
        assert n.tolist() == [0, 0, 1, 0] and bounds.tolist() == [0]
        n, bounds = ops.mask_rle(to_dev(torch.zeros(1, 1, dtype=torch.int16)), 4)
        assert n.tolist() == [0, 0, 0, 0] and bounds.numel() == 0


def test_a_table_of_the_background_alone_and_a_full_table():
    """`channels == 1`: nothing can be an object, n == [0] and no boundaries, without an error; `channels == 4096`, the
    most the LDS cursors hold, is accepted (test_rle_refusals holds the refusal of 4097)"""
    plane = (torch.arange(24 * 48).view(24, 48) % 7).to(torch.int16)
    n, bounds = ops.mask_rle(to_dev(plane), 1)
    assert n.dtype == torch.int32 and n.tolist() == [0]
    assert bounds.dtype == torch.int32 and bounds.numel() == 0
    plane = (torch.arange(24 * 48).view(24, 48) * 5 % 1153).to(torch.int16)    # 1152 distinct labels 0..1152
    plane[3, 7:11] = 4095
    n, bounds = ops.mask_rle(to_dev(plane), 4096)
    _check_rle(plane, 4096, n, bounds, strings=[1, 5, 1152, 4094, 4095])
    assert n.numel() == 4096 and n[4095] == 8 and n[4094] == 0


def test_rle_refusals():
    if DRYRUN:
        pytest.skip('the library refuses')
    plane = to_dev(torch.zeros(8, 8, dtype=torch.int16))
    with pytest.raises(DevaHipError):
        ops.mask_rle(plane, 4097)                                   # more channels than the LDS cursors hold
    with pytest.raises(DevaHipError):
        ops.mask_rle(plane.long(), 2)
    # `write` refuses a capacity below what `n` announces, before any launch
    nbytes = lib().deva_mask_rle_scratch(8, 8, 3)
    scratch = torch.empty(nbytes // 4 + 1, dtype=torch.int32, device=plane.device)
    n_host = torch.tensor([0, 4, 2], dtype=torch.int32)
    out = torch.empty(6, dtype=torch.int32, device=plane.device)
    assert lib().deva_mask_rle_write(8, 8, 3, scratch.data_ptr(), nbytes, n_host.data_ptr(), out.data_ptr(), 5, None) != 0
    assert b'do not fit' in lib().deva_hip_last_error()


# ------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize('dataset', ['demo', 'burst'])
def test_clip_through_the_saver(dataset, peaky_state_dict, tmp_path):
    """the smoke-size clip (96 x 128, the recipe of the ensemble test, 2 objects, 3 frames): `DEVAInferenceCore.step` ->
    `FrameResultSaver` into tmp_path; the files and the JSON must be what the CPU contract makes of the same
    probabilities' `index` planes, and nothing may be left queued after `end()`"""
    import ensemble_case as EC
    from deva.inference.frame_results import FrameResultSaver, long_id_colors
    from deva.inference.inference_core import DEVAInferenceCore
    from deva.model.network import DEVA
    dev = gpu_util.dev()
    net = DEVA(EC.clip_config())
    net.load_weights(peaky_state_dict)
    core = DEVAInferenceCore(net.to(dev).eval(), EC.clip_config())
    om = core.object_manager
    long_id = dataset == 'demo'
    om.use_long_id = long_id
    wanted = [70000, 66051] if long_id else [1, 2]
    saver = FrameResultSaver(str(tmp_path), 'clip', dataset=dataset, object_manager=om)
    frames = EC.clip_frames()[:3]
    from workload import synth
    mask = torch.tensor([0] + wanted)[synth.box_mask(EC.H, EC.W, 2)]
    kept = []
    for t, frame in enumerate(frames):
        image = emu_ops_input(frame).to(dev)
        prob = core.step(image, mask.to(dev) if t == 0 else None, wanted if t == 0 else None)
        kept.append((prob, ops.frame_result(prob.contiguous(), want=('index',)).index.cpu(), frame.numpy()))
        saver.save_mask(prob, f'{t:05d}.jpg', image_np=frame.numpy())
    saver.end()
    assert saver.queue.empty() and not saver.thread.is_alive() and saver.error is None
    assert om.all_obj_ids == wanted
    table = torch.tensor([0] + wanted)
    entries = saver.video_json['segmentations' if dataset == 'burst' else 'annotations']
    assert [e['file_name'] for e in entries] == [f'{t:05d}.jpg' for t in range(3)]
    for t, (prob, index, frame) in enumerate(kept):
        made = E.products_from_index(index, prob.shape[0], table, long_id_colors(table.numpy()), frame)
        live = [(tmp, oid) for tmp, oid in enumerate(wanted, start=1) if made['stats'][tmp, 0] > 0]
        if dataset == 'demo':
            assert np.array_equal(np.array(Image.open(tmp_path / 'Annotations' / 'clip' / f'{t:05d}.png')), made['color'])
            assert Image.open(tmp_path / 'Visualizations' / 'clip' / f'{t:05d}.jpg').size == (EC.W, EC.H)
            assert entries[t]['segments_info'] == [dict(category_id=None, id=oid, score=None, area=int(made['stats'][tmp, 0]))
                                                   for tmp, oid in live]
        else:
            assert np.array_equal(np.array(Image.open(tmp_path / 'clip' / f'{t:05d}.png')), made['gray'])
            assert [s['id'] for s in entries[t]['segmentations']] == [oid for _, oid in live]
            for seg, (tmp, _) in zip(entries[t]['segmentations'], live):
                assert seg['rle'] == E.coco_encode(index.numpy() == tmp)
    assert len(live) == 2    # both objects are still there on the last frame: the comparison is not empty
    # the overlay before the JPEG codec, from the saver's own path
    res = om.frame_result(kept[-1][0], image=kept[-1][2], color='id')
    assert np.array_equal(res.blend.cpu().numpy(), made['blend'])
    json.dumps(saver.video_json)


def emu_ops_input(frame_u8):
    """the reader's transform of a decoded frame (ToTensor + Normalize), on the host"""
    import ensemble_case as EC
    mean, std = torch.tensor(EC.MEAN).view(3, 1, 1), torch.tensor(EC.STD).view(3, 1, 1)
    return (frame_u8.permute(2, 0, 1).float() / 255 - mean) / std
