"""The box prompts (csrc/box_prompts.hip, `ops.box_nms_xyxy`, `ops.box_mask_select`, `detections.text_detections`) on the
device against their CPU contract (tests/emu_text.py), and `TextPromptedProcessor` on the HIP library against the
straight-line restatement of tests/text_case.py run on the same library.  Every fp32 operation of the contract is a
single rounded one on both sides and the rest are comparisons, so every comparison is exact: keep lists in order,
choices, planes.  With DEVA_TEST_DRYRUN=1 the same code runs on the CPU contract."""
import os

import numpy as np
import pytest
import torch

import emu_detections as ED
import emu_proposals as EP
import emu_text as ET
import gpu_util
import test_text_cpu as CPU
import text_case as TC
from deva.hip import check, lib, ops
from gpu_util import to_dev

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DRYRUN = os.environ.get('DEVA_TEST_DRYRUN') == '1'
F = np.float32


@pytest.fixture(autouse=True)
def _emulated_when_dry(monkeypatch):
    if DRYRUN:
        EP.install(monkeypatch)
        ED.install(monkeypatch)
        ET.install(monkeypatch)
        monkeypatch.setattr(torch.Tensor, 'cuda', lambda self, *a, **k: self)


def candidates(b, m, h, w, seed):
    """fp32 logits [b,m,h,w] around 0 (a quarter exactly at the threshold 0.25 or at 0, some NaN and +-inf) and scores
    [b,m] from a small grid, so that ties are common, with a NaN and a -0.0 / 0.0 pair here and there"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((b, m, h, w)).astype(F)
    pick = rng.integers(0, 16, x.shape)
    x[pick == 0], x[pick == 1], x[pick == 2] = 0.25, 0.0, -0.0
    x[pick == 3] = np.nextafter(F(0.25), F(1))
    holes = rng.integers(0, 97, x.shape)
    x[holes == 0], x[holes == 1], x[holes == 2] = np.nan, np.inf, -np.inf
    s = rng.choice(np.array([0.5, 0.75, 0.9, 0.9, -0.0, 0.0], dtype=F), (b, m))
    if b >= 3:
        s[rng.integers(0, b, max(b // 8, 1)), rng.integers(0, m, max(b // 8, 1))] = np.nan
    return x, s


# ------------------------------------------------------------------------------------------ box_mask_select
@pytest.fixture(scope='module')
def select_cases():
    """every (h, w, m) once at the largest batch: inputs and the contract's answer (shared, never modified); a smaller
    batch is a prefix"""
    out = {}
    for h, w in ((8, 12), (29, 53), (30, 45), (64, 64)):
        for m in (1, 3, 4):
            x, s = candidates(65, m, h, w, 1000 * h + m)
            out[(h, w, m)] = (x, s, *ET.mask_select(x, s, 0.25))
    return out


@pytest.mark.parametrize('b', [0, 1, 3, 64, 65])
@pytest.mark.parametrize('m', [1, 3, 4])
@pytest.mark.parametrize('h,w', [(8, 12), (29, 53), (30, 45), (64, 64)])
def test_select_is_bit_identical(h, w, m, b, select_cases):
    """29 x 53: every plane after the first starts 4 bytes off a 16-byte boundary and the width is no multiple of 4;
    called twice: the same bytes"""
    x, s, want_planes, want_chosen = select_cases[(h, w, m)]
    logits, scores = to_dev(torch.from_numpy(x[:b])), to_dev(torch.from_numpy(s[:b]))
    runs = [ops.box_mask_select(logits, scores, 0.25) for _ in range(2)]
    for planes, chosen in runs:
        assert planes.dtype == torch.uint8 and tuple(planes.shape) == (b, h, w)
        assert chosen.dtype == torch.int32 and chosen.cpu().tolist() == want_chosen[:b].tolist()
        assert np.array_equal(planes.cpu().numpy(), want_planes[:b])
    if b == 65 and m > 1:
        assert len(set(want_chosen.tolist())) == m and 0 < want_planes.mean() < 1


def test_more_boxes_than_one_grid_dimension():
    """66 000 boxes of 2 x 3 with two candidates: cut into launches of 65535 boxes"""
    b = 66000
    x, s = candidates(b, 2, 2, 3, 77)
    want_planes, want_chosen = ET.mask_select(x, s, 0.0)
    planes, chosen = ops.box_mask_select(to_dev(torch.from_numpy(x)), to_dev(torch.from_numpy(s)), 0.0)
    assert chosen.cpu().tolist() == want_chosen.tolist() and np.array_equal(planes.cpu().numpy(), want_planes)
    assert want_chosen[65535:].sum() > 0 and want_planes[65535:].sum() > 0


def test_only_the_chosen_plane_is_read():
    """the planes that are not chosen are NaN, +-inf or other boxes' planes: the result does not change; a chosen plane
    with NaN / +-inf holes obeys rule S2"""
    h, w, b, m = 30, 45, 24, 3
    x, s = candidates(b, m, h, w, 5)
    want_planes, want_chosen = ET.mask_select(x, s, 0.25)
    assert np.isnan(x[np.arange(b), want_chosen]).any() and np.isinf(x[np.arange(b), want_chosen]).any()
    others = np.ones((b, m), dtype=bool)
    others[np.arange(b), want_chosen] = False
    for fill in (np.nan, np.inf, -np.inf, 'rolled'):
        y = x.copy()
        y[others] = np.roll(x, 1, axis=0)[others] if isinstance(fill, str) else fill
        planes, chosen = ops.box_mask_select(to_dev(torch.from_numpy(y)), to_dev(torch.from_numpy(s)), 0.25)
        assert chosen.cpu().tolist() == want_chosen.tolist() and np.array_equal(planes.cpu().numpy(), want_planes)


def _poisoned(nbytes, offset, guard=256):
    buf = torch.full((guard + offset + nbytes + guard,), 0xA5, dtype=torch.uint8)
    return to_dev(buf), guard + offset


@pytest.mark.parametrize('h,w,shift', [(29, 53, 0), (29, 53, 5), (30, 45, 7), (64, 64, 13), (8, 12, 5)])
def test_guard_bands(h, w, shift):
    """`out` and `chosen` inside 0xA5-poisoned buffers, `out` at every alignment: the guards come back untouched"""
    if DRYRUN:
        pytest.skip('raw pointers: needs the library')
    b, m = 5, 3
    x, s = candidates(b, m, h, w, 31 + shift)
    want_planes, want_chosen = ET.mask_select(x, s, 0.25)
    logits, scores = to_dev(torch.from_numpy(x)), to_dev(torch.from_numpy(s))
    out, at = _poisoned(b * h * w, shift)
    chosen, cat = _poisoned(4 * b, 0)
    assert (out.data_ptr() + at) % 16 == shift and (chosen.data_ptr() + cat) % 4 == 0
    check(lib().deva_box_mask_select(logits.data_ptr(), scores.data_ptr(), b, m, h, w, 0.25, out.data_ptr() + at,
                                     chosen.data_ptr() + cat, None), 'deva_box_mask_select')
    torch.cuda.synchronize()
    host, chost = out.cpu(), chosen.cpu()
    assert bool((host[:at] == 0xA5).all()) and bool((host[at + b * h * w:] == 0xA5).all())
    assert bool((chost[:cat] == 0xA5).all()) and bool((chost[cat + 4 * b:] == 0xA5).all())
    assert np.array_equal(host[at:at + b * h * w].view(b, h, w).numpy(), want_planes)
    assert chost[cat:cat + 4 * b].view(torch.int32).tolist() == want_chosen.tolist()
    # through the wrapper: a slice of an arena at an odd byte offset, and no choice list wanted
    arena, at = _poisoned(b * h * w, shift)
    planes, _ = ops.box_mask_select(logits, scores, 0.25, out=arena[at:at + b * h * w].view(b, h, w))
    torch.cuda.synchronize()
    host = arena.cpu()
    assert bool((host[:at] == 0xA5).all()) and bool((host[at + b * h * w:] == 0xA5).all())
    assert np.array_equal(planes.cpu().numpy(), want_planes)
    check(lib().deva_box_mask_select(logits.data_ptr(), scores.data_ptr(), b, m, h, w, 0.25, arena.data_ptr() + at, None, None),
          'deva_box_mask_select')


def test_offsets_beyond_32_bits():
    """180 boxes of three 1080 x 1920 planes (4.5 GB, filled on the device with NaN): the scores send the last boxes'
    choice to plane 2, whose bytes start beyond 2^32.  Only boxes 0, 90, 178 and 179 hold data and are compared"""
    if DRYRUN:
        pytest.skip('4.5 GB of logits: the device only')
    h, w, m, b = 1080, 1920, 3, 180
    live = {0: 1, 90: 0, 178: 2, 179: 2}
    assert ((179 * m + 2) * h * w) * 4 > 1 << 32 and ((178 * m + 2) * h * w) * 4 > 1 << 32
    logits = torch.full((b, m, h, w), float('nan'), device=gpu_util.dev())
    scores = torch.full((b, m), 0.5)
    planes_in, _ = candidates(len(live), 1, h, w, 9)
    for (k, pick), plane in zip(live.items(), planes_in):
        logits[k, pick].copy_(torch.from_numpy(plane[0]))
        scores[k, pick] = 0.9
    planes, chosen = ops.box_mask_select(logits, to_dev(scores), 0.25)
    chosen = chosen.cpu().tolist()
    want, _ = ET.mask_select(planes_in, np.zeros((len(live), 1), dtype=F), 0.25)
    for row, (k, pick) in enumerate(live.items()):
        assert chosen[k] == pick and np.array_equal(planes[k].cpu().numpy(), want[row]), k
    assert all(c == 0 for k, c in enumerate(chosen) if k not in live)      # equal scores: the first
    assert int(planes[1].sum()) == 0                                        # a NaN plane: nothing set


# ------------------------------------------------------------------------------------------ box_nms_xyxy
def nms_case(n, integer=False):
    """fractional boxes with duplicates, zero-area and inverted boxes, blocks of equal scores, NaN and -0.0 scores"""
    rng = np.random.default_rng(n)
    side = 24 if n < 1000 else 160
    x0, y0 = rng.uniform(0, side, n), rng.uniform(0, side, n)
    boxes = np.stack([x0, y0, x0 + rng.uniform(0, 12, n), y0 + rng.uniform(0, 12, n)], 1)
    boxes = np.round(boxes) if integer else np.round(boxes * 8) / 8 + rng.choice([0.0, 0.1, 1 / 3], (n, 1))
    boxes = boxes.astype(F)
    boxes[rng.integers(0, n, n // 3)] = boxes[rng.integers(0, n, n // 3)]                    # duplicates
    zero = rng.integers(0, n, n // 10)
    boxes[zero, 2] = boxes[zero, 0]                                                          # zero-area
    inverted = rng.integers(0, n, n // 10)
    boxes[inverted] = boxes[inverted][:, [2, 1, 0, 3]]                                       # x1 < x0
    scores = rng.choice(np.array([0.5, 0.75, 0.9, 0.9, 1.0], dtype=F), n)                    # blocks of equal scores
    if n >= 63:
        scores[rng.integers(0, n, 3)] = np.nan
        scores[rng.integers(0, n, 3)] = -0.0
    return boxes, scores


@pytest.mark.parametrize('n', [1, 63, 64, 65, 130, 1000, 4096])
def test_box_nms_xyxy(n):
    boxes, scores = nms_case(n)
    assert n < 63 or ((boxes[:, 2] < boxes[:, 0]).any() and (boxes != np.round(boxes)).any())
    for thresh in (0.8, 0.5, 0.0):
        want = ET.nms_xyxy(boxes, scores, thresh)
        got = [ops.box_nms_xyxy(to_dev(torch.from_numpy(boxes)), to_dev(torch.from_numpy(scores)), thresh) for _ in range(2)]
        assert got[0].dtype == torch.int32 and got[0].cpu().tolist() == want and got[1].cpu().tolist() == want
        assert 0 < len(want) and (n < 63 or len(want) < n)
    # integer-valued input: what the integer entry point keeps
    boxes, scores = nms_case(n, integer=True)
    for thresh in (0.8, 0.0):
        as_float = ops.box_nms_xyxy(to_dev(torch.from_numpy(boxes)), to_dev(torch.from_numpy(scores)), thresh)
        as_int = ops.box_nms(to_dev(torch.from_numpy(boxes.astype(np.int32))), to_dev(torch.from_numpy(scores)), thresh)
        assert as_float.cpu().tolist() == as_int.cpu().tolist() == EP.nms(boxes.astype(np.int32), scores, thresh)


def test_box_nms_xyxy_of_nothing_and_packed():
    assert ops.box_nms_xyxy(to_dev(torch.zeros(0, 4)), to_dev(torch.zeros(0)), 0.8).cpu().tolist() == []
    boxes, scores = nms_case(130)
    want = ET.nms_xyxy(boxes, scores, 0.5)
    packed = to_dev(torch.full((131,), -7, dtype=torch.int32))
    assert ops.box_nms_xyxy(to_dev(torch.from_numpy(boxes)), to_dev(torch.from_numpy(scores)), 0.5, packed=packed) is packed
    host = packed.cpu().tolist()
    assert host[130] == len(want) and host[:len(want)] == want


# ------------------------------------------------------------------------------------------ text_detections
def test_the_reference_golden_on_the_device(golden_dir):
    CPU.check_against_golden(np.load(os.path.join(golden_dir, 'text_segmentation.npz')), gpu_util.dev())


class RandomSegmenter:
    """three candidate planes per box at the frame's size: a rectangle of the box grown by 0, 3 and 6 pixels, scores from
    the box's bits; the planes are made on the host once and uploaded"""
    mask_threshold = 0.0

    def __init__(self, h, w):
        self.h, self.w, self.calls = h, w, 0

    def answer(self, boxes):
        logits = np.full((len(boxes), 3, self.h, self.w), -4.0, dtype=F)
        scores = np.zeros((len(boxes), 3), dtype=F)
        for k, (x0, y0, x1, y1) in enumerate(boxes):
            for m in range(3):
                logits[k, m, max(int(y0) - 3 * m, 0):int(y1) + 3 * m, max(int(x0) - 3 * m, 0):int(x1) + 3 * m] = 4.0
            scores[k] = np.roll(np.array([0.9, 0.5, 0.9], dtype=F), int(x0) % 3)
        return logits, scores

    def predict_boxes(self, boxes_px):
        self.calls += 1
        assert 0 < boxes_px.shape[0] <= 16
        logits, scores = self.answer(boxes_px.cpu().numpy())
        return torch.from_numpy(logits).to(boxes_px.device), torch.from_numpy(scores).to(boxes_px.device)


def test_a_1080p_frame():
    """40 raw boxes through NMS, select in batches of 16 and the assembly to 480 x 853, against the CPU statement"""
    from deva.inference import detections as D
    h, w, size = 1080, 1920, (480, 853)
    rng = np.random.default_rng(40)
    x0, y0 = rng.uniform(0, w - 400, 28), rng.uniform(0, h - 300, 28)
    boxes = np.stack([x0, y0, x0 + rng.uniform(40, 400, 28), y0 + rng.uniform(30, 300, 28)], 1).astype(F)
    boxes = np.concatenate([boxes, boxes[:12] + rng.uniform(-3, 3, (12, 4)).astype(F)])      # near-duplicates
    conf = rng.choice(np.array([0.4, 0.55, 0.55, 0.7, 0.85], dtype=F), 40)
    classes = np.array([None if k % 11 == 5 else k % 3 for k in range(40)], dtype=object)
    keep = ET.nms_xyxy(boxes, conf, 0.8)
    assert 17 <= len(keep) < 40
    segmenter = RandomSegmenter(h, w)
    mask, info = D.text_detections(boxes, conf, classes, segmenter, (h, w), size, nms_threshold=0.8, device=gpu_util.dev())
    assert segmenter.calls == -(-len(keep) // 16)
    planes, _ = ET.mask_select(*segmenter.answer(boxes[keep]))
    want_mask, want_rec = ED.detection_assemble(torch.from_numpy(planes), size, 'text')
    assert mask.dtype == torch.int64 and torch.equal(mask.cpu(), want_mask)
    order = sorted((int(r[0]), k) for k, r in enumerate(want_rec.tolist()) if r[0] > 0)
    assert [o.id for o in info] == [i for i, _ in order] and len(order) >= 10
    assert [o.category_ids[0] for o in info] == [classes[keep[k]] for _, k in order]
    assert [float(o.scores[0]) for o in info] == [float(conf[keep[k]]) for _, k in order]


# ------------------------------------------------------------------------------------------ the frame loop
@pytest.mark.parametrize('setting', ['online', 'semionline'])
def test_processor_is_the_restated_loop_on_the_library(setting, recipe_state_dict, monkeypatch):
    """the clip of the CPU test through TextPromptedProcessor and through the straight-line restatement, both on the HIP
    library: bit-identical probabilities, the same index masks and segments (this checks the loop, not the kernels)"""
    from deva.inference.inference_core import DEVAInferenceCore
    from deva.model.network import DEVA
    net = DEVA(gpu_util.net_config(**TC.loop_config(setting)))
    net.load_weights(recipe_state_dict[0])
    net = net.to(gpu_util.dev()).eval()
    make_core = lambda s: DEVAInferenceCore(net, gpu_util.net_config(**TC.loop_config(s)))   # noqa: E731
    got, flushed, processor, keywords = TC.check_clip(setting, make_core, monkeypatch)
    assert keywords == [{}, {}, {}] and flushed == [] and all(p.device.type == gpu_util.dev().type for _, p in got)
