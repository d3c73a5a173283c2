"""The prompt-point choice (csrc/prompts.hip, `ops.prompt_points`, `detections.forward_prompt_points`) on the device
against its CPU contract (tests/emu_prompts.py), and `AutomaticProcessor` on the HIP library against the straight-line
restatement of tests/test_prompts_cpu.py run on the same library.  Every fp32 operation of the contract is a single
rounded one on both sides, so every comparison is exact: labels as int32 bits, kept points, count.  With
DEVA_TEST_DRYRUN=1 the same code runs on the CPU contract."""
import os

import numpy as np
import pytest
import torch

import emu_detections as ED
import emu_prompts as EM
import emu_proposals as EP
import gpu_util
import prompt_case as PC
import test_prompts_cpu as CPU
from deva.hip import check, lib, ops
from gpu_util import to_dev

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DRYRUN = os.environ.get('DEVA_TEST_DRYRUN') == '1'
NAN_BITS = 0x7FC00ABC   # the poison: a NaN no kernel produces


@pytest.fixture(autouse=True)
def _emulated_when_dry(monkeypatch):
    if DRYRUN:
        EP.install(monkeypatch)
        ED.install(monkeypatch)
        EM.install(monkeypatch)
        monkeypatch.setattr(torch.Tensor, 'cuda', lambda self, *a, **k: self)


def bits(t):
    return t.cpu().contiguous().view(torch.int32)


def speckle(h, w, seed, p=0.012):
    """sparse foreground: labels scatter around the threshold, so both sides of the comparison occur everywhere"""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(h, w, generator=g) < p).to(torch.int64) * ((1 << 31) + 5)


def masks_of(h, w, seed):
    return {'discs': PC.forward_mask(h, w, seed), 'speckle': speckle(h, w, seed)}


def compare(mask, grid, threshold=0.01):
    """`ops.prompt_points` on the device against the contract, bit for bit; the rows beyond the count keep their poison
    -> (labels, count)"""
    n = grid.shape[0]
    want_points, want_labels, want_count = EM.prompt_points(mask.cpu(), grid, threshold)
    packed = to_dev(torch.full((2 * n + 1,), NAN_BITS, dtype=torch.int32).view(torch.float32))
    points, labels, count = ops.prompt_points(to_dev(mask), to_dev(grid), threshold, packed=None if DRYRUN else packed)
    kept = int(count.cpu()[0])
    assert kept == int(want_count) and count.dtype == torch.int32 and tuple(count.shape) == (1,)
    assert tuple(labels.shape) == (n,) and torch.equal(bits(labels), bits(want_labels))
    assert tuple(points.shape) == (n, 2) and torch.equal(bits(points[:kept]), bits(want_points[:kept]))
    if not DRYRUN:
        assert bool((bits(points[kept:]) == NAN_BITS).all())
    return want_labels, kept


# ------------------------------------------------------------------------------------------ shapes
@pytest.mark.parametrize('h,w,n', [(16, 16, 2), (17, 33, 3), (31, 47, 3), (96, 128, 8), (481, 853, 33), (1080, 1920, 64),
                                   (1080, 1920, 128)])
def test_shapes_are_bit_identical(h, w, n):
    """16 x 16: a 1 x 1 map, every tap of every point is the one cell or outside; 17 x 33 and 31 x 47: a clipped last
    window, rows and columns beyond 16 (H / 16) that still lie inside a support, 9 points; 481 x 853: odd sizes, 1089
    points; 1080 x 1920 with 4096 and with 16384 points, the limit"""
    grid = PC.grid(n)
    both = 0
    for kind, mask in masks_of(h, w, h + n).items():
        labels, kept = compare(mask, grid)
        both += 0 < kept < n * n
        assert float(labels.max()) > 0.0, kind
    assert both >= 1 or h < 96                     # at the sizes of a frame some points are kept and some are not


def test_uint8_and_int64_masks_agree():
    grid = PC.grid(8)
    for kind, mask in masks_of(96, 128, 7).items():
        a = ops.prompt_points(to_dev(mask), to_dev(grid))
        b = ops.prompt_points(to_dev((mask > 0).to(torch.uint8)), to_dev(grid))
        c = ops.prompt_points(to_dev(mask > 0), to_dev(grid))
        kept = int(a[2].cpu()[0])
        for other in (b, c):
            assert int(other[2].cpu()[0]) == kept and torch.equal(bits(a[1]), bits(other[1]))
            assert torch.equal(bits(a[0][:kept]), bits(other[0][:kept]))
        compare((mask > 0).to(torch.uint8), grid)
        compare(mask, grid)


def test_nothing_tracked_keeps_every_point_and_everything_tracked_keeps_none():
    for n in (8, 33):
        grid = PC.grid(n)
        labels, kept = compare(torch.zeros(96, 128, dtype=torch.int64), grid)
        assert kept == n * n and bool((labels == 0).all())                      # in order: compare() checked the bits
        labels, kept = compare(torch.full((96, 128), 200, dtype=torch.uint8), grid)
        assert kept == 0 and float(labels.min()) > 0.2                          # out_points is left as poisoned
        labels, kept = compare(torch.full((96, 128), 1 << 40, dtype=torch.int64), grid)
        assert kept == 0


def test_foreground_is_decided_on_64_bits():
    ids = torch.zeros(96, 128, dtype=torch.int64)
    ids[:, :40] = (1 << 31) + 5                 # low word 0x80000005: negative as an int32
    ids[:48, 40:80] = 1 << 32                   # low word 0
    ids[48:, 40:80] = -3
    ids[:, 80:] = -(1 << 40)
    grid = PC.grid(8)
    labels, kept = compare(ids, grid)
    want = EM.prompt_points((ids > 0).to(torch.uint8), grid)
    assert torch.equal(bits(labels), bits(want[1])) and kept == int(want[2]) and 0 < kept < 64
    field = labels.view(8, 8)
    assert float(field[:, 0].min()) > 0.5 and float(field[1, 3]) > 0.5 and float(field[6, 3]) < 0.5 and float(field[:, 7].max()) == 0.0


def test_thresholds_are_strict_and_fp32():
    mask, grid = PC.forward_mask(96, 128, 6), PC.grid(8)
    labels = EM.prompt_points(mask, grid)[1]
    some = sorted(set(float(v) for v in labels if 0 < float(v) < 1))
    assert len(some) >= 3
    for value in (some[0], some[len(some) // 2]):
        _, at = compare(mask, grid, value)                                      # equal is not below
        _, above = compare(mask, grid, float(np.nextafter(np.float32(value), np.float32(2))))
        assert above == at + int((labels == value).sum())
    assert compare(mask, grid, float('inf'))[1] == 64 and compare(mask, grid, -1.0)[1] == 0


# ------------------------------------------------------------------------------------------ raw pointers
def _poisoned(words, guard=64):
    buf = torch.full((guard + words + guard,), NAN_BITS, dtype=torch.int32)
    buf[guard + words:] = 0x5E471E1                                             # the sentinel behind
    return to_dev(buf), guard


def test_outputs_stay_inside_their_buffers_and_a_misaligned_mask_start():
    """481 x 853 int64 with the mask one row into its allocation (853 * 8 bytes: 8 past a 16-byte boundary, so the
    16-byte loads meet a misaligned start on every other row), uint8 at every byte offset; out_points, out_labels and
    out_count in poisoned buffers with a sentinel behind; twice: the same bytes"""
    if DRYRUN:
        pytest.skip('raw pointers: needs the library')
    L = lib()
    h, w, n = 481, 853, 33
    grid = PC.grid(n)
    p = n * n
    nbytes = L.deva_prompt_scratch(h, w, p)
    for kind, mask in masks_of(h, w, 5).items():
        want_points, want_labels, want_count = EM.prompt_points(mask, grid)
        kept = int(want_count)
        for elem, offset in ((8, w * 8), (8, 0), (1, 0), (1, 1), (1, 7), (1, 13)):
            src = mask if elem == 8 else (mask > 0).to(torch.uint8)
            raw = torch.zeros(offset + h * w * elem + 64, dtype=torch.uint8)
            raw[offset:offset + h * w * elem] = src.contiguous().view(torch.uint8).view(-1)
            raw = to_dev(raw)
            assert (raw.data_ptr() + offset) % 16 == offset % 16
            runs = []
            for _ in range(2):
                (pts, gp), (lab, gl), (cnt, gc) = _poisoned(2 * p), _poisoned(p), _poisoned(1)
                scratch = to_dev(torch.full((nbytes // 4 + 64,), NAN_BITS, dtype=torch.int32))
                dev_grid = to_dev(grid)
                check(L.deva_prompt_points(raw.data_ptr() + offset, elem, h, w, dev_grid.data_ptr(), p, 0.01, scratch.data_ptr(),
                                           nbytes, pts.data_ptr() + 4 * gp, lab.data_ptr() + 4 * gl, cnt.data_ptr() + 4 * gc,
                                           None), 'deva_prompt_points')
                torch.cuda.synchronize()
                pts, lab, cnt, scratch = pts.cpu(), lab.cpu(), cnt.cpu(), scratch.cpu()
                for buf, guard, words in ((pts, gp, 2 * p), (lab, gl, p), (cnt, gc, 1)):
                    assert bool((buf[:guard] == NAN_BITS).all()) and bool((buf[guard + words:] == 0x5E471E1).all())
                assert bool((scratch[nbytes // 4:] == NAN_BITS).all())
                assert int(cnt[gc]) == kept and torch.equal(lab[gl:gl + p], bits(want_labels))
                assert torch.equal(pts[gp:gp + 2 * kept], bits(want_points[:kept]).view(-1))
                assert bool((pts[gp + 2 * kept:gp + 2 * p] == NAN_BITS).all())  # rows beyond the count: untouched
                runs.append((pts, lab, cnt))
            assert all(torch.equal(a, b) for a, b in zip(*runs))


# ------------------------------------------------------------------------------------------ the reference's points
def test_the_reference_golden_on_the_device(golden_dir):
    """what the REFERENCE's auto_segment kept (tests/golden/prompt_points.npz), through `forward_prompt_points`: the same
    set in the same order, under the margin condition asserted on torch's CPU evaluation; no case is left out"""
    from deva.inference import detections as D
    golden = np.load(os.path.join(golden_dir, 'prompt_points.npz'))
    assert sorted({k.split('/')[0] for k in golden.files}) == sorted(PC.GOLDEN_CASES)
    for name, (h, w, n, seed, t) in PC.GOLDEN_CASES.items():
        mask = PC.golden_mask(name)
        margin = float((CPU.torch_labels(mask, PC.grid(n), n) - np.float32(0.01)).abs().min())
        print(name, f'min |label - 0.01| = {margin:.3e}')
        assert margin >= 1e-4, (name, margin)
        got = D.forward_prompt_points(to_dev(mask), n)
        want = golden[name + '/points']
        assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == want.shape
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), name
        again = D.forward_prompt_points(to_dev(mask), point_grid=to_dev(PC.grid(n)))       # an explicit grid; the pinned buffer again
        assert np.array_equal(again.view(np.int32), want.view(np.int32)), name
    assert len(golden['covered_96x128_n8/points']) == 0


def test_a_padded_forward_mask_view():
    """`estimate_forward_mask` returns the unpadded view of a padded mask: not contiguous"""
    from deva.inference import detections as D
    padded = torch.zeros(496, 864, dtype=torch.int64)
    mask = PC.forward_mask(481, 853, 5)
    padded[7:488, 5:858] = mask
    view = to_dev(padded)[7:488, 5:858]
    assert not view.is_contiguous()
    want = EM.prompt_points(mask, PC.grid(32))
    got = D.forward_prompt_points(view, 32)
    assert np.array_equal(got.view(np.int32), want[0][:int(want[2])].numpy().view(np.int32)) and 0 < len(got) < 1024


# ------------------------------------------------------------------------------------------ the frame loop
@pytest.mark.parametrize('setting', ['online', 'semionline'])
def test_processor_is_the_restated_loop_on_the_library(setting, recipe_state_dict, monkeypatch):
    """the clip of the CPU test through AutomaticProcessor and through the straight-line restatement, both on the HIP
    library: bit-identical probabilities, the same points asked (this checks the loop, not the kernels)"""
    from deva.inference.inference_core import DEVAInferenceCore
    from deva.model.network import DEVA
    net = DEVA(gpu_util.net_config(**PC.loop_config(setting)))
    net.load_weights(recipe_state_dict[0])
    net = net.to(gpu_util.dev()).eval()
    frames, rects = PC.clip()
    names = [f'{t:05d}.jpg' for t in range(len(frames))]
    make_core = lambda s: DEVAInferenceCore(net, gpu_util.net_config(**PC.loop_config(s)))   # noqa: E731
    got, flushed, processor = CPU.check_clip(setting, make_core, frames, rects, names, monkeypatch)
    assert flushed == [] and all(p.device.type == gpu_util.dev().type for _, p in got)
