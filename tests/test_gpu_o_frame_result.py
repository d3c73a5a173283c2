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
    global atomics and must be the same numbers"""
    for c, h, w in ((300, 24, 40), (1100, 24, 48)):
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
def _check_rle(index, channels, n, bounds, strings=True):
    from deva.inference.frame_results import rle_strings
    want_n, want_b = E.rle_bounds(index, channels)
    n, bounds = n.cpu().numpy(), bounds.cpu().numpy()
    assert n.dtype == np.int32 and bounds.dtype == np.int32
    assert np.array_equal(n, want_n), (n[:8], want_n[:8])
    assert np.array_equal(bounds, np.concatenate(want_b))
    if strings:
        h, w = index.shape
        texts = rle_strings(n, bounds, h * w)
        for c in range(1, channels):
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
