"""The box prompts and the text-prompted frame loop without a GPU: the two entry points on the ABI and their argument
errors, the CPU contract (tests/emu_text.py) by hand and against the integer NMS, `text_detections` against what the
REFERENCE's segment_with_text produced (tests/golden/text_segmentation.npz), and `TextPromptedProcessor` on the emulated
ops against a straight-line restatement of the reference's loop (deva/ext/with_text_processor.py:30-122,
demo_utils.py:22-46)."""
import os
import re

import numpy as np
import pytest
import torch

import abi_util
import emu_detections as ED
import emu_ops
import emu_proposals as EP
import emu_text as ET
import text_case as TC

torch.set_grad_enabled(False)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('deva_box_nms_xyxy', 'deva_box_mask_select')
F = np.float32


@pytest.fixture()
def emu(monkeypatch):
    emu_ops.install(monkeypatch)
    ED.install(monkeypatch)
    EP.install(monkeypatch)
    ET.install(monkeypatch)
    monkeypatch.setattr(torch.Tensor, 'cuda', lambda self, *a, **k: self)   # (frame_to_network_input uploads the frame)


# ------------------------------------------------------------------------------------------ ABI
def test_entry_points_are_exported_declared_and_bound():
    from deva import hip
    from deva.hip import ops
    header = abi_util.inference_entry_points(NAMES, returns='int')
    assert 'box_nms_xyxy' in ops.__all__ and 'box_mask_select' in ops.__all__
    assert len(hip.SIGNATURES) == 80
    for ref in ('grounding_dino.py:101-115', 'grounding_dino.py:112'):
        assert ref in header, ref


A, S = 1 << 30, 1 << 20   # made-up addresses: validation fails before anything is dereferenced or launched


def _nms(L, boxes=A, scores=A, n=8, thr=0.5, scratch=S, nbytes=1 << 24, keep=A, n_keep=A):
    return L.deva_box_nms_xyxy(boxes, scores, n, thr, scratch, nbytes, keep, n_keep, None)


def _select(L, logits=A, scores=A, batch=2, per_box=3, h=8, w=12, thr=0.0, out=A + 1, chosen=A):
    return L.deva_box_mask_select(logits, scores, batch, per_box, h, w, thr, out, chosen, None)


def test_argument_errors_before_any_launch():
    from deva import hip
    L = hip.lib()
    err = L.deva_hip_last_error
    assert _nms(L, n=-1) == 2 and b'negative number of boxes' in err()
    assert _nms(L, n=4097) == 2 and b'at most 4096 boxes' in err()
    assert _nms(L, thr=float('nan')) == 2 and b'not a number' in err()
    assert _nms(L, n_keep=None) == 2 and b'keep count' in err()
    assert _nms(L, n_keep=A + 2) == 2 and b'keep count' in err()
    assert _nms(L, boxes=None) == 2 and b'boxes' in err()
    assert _nms(L, boxes=A + 2) == 2 and b'misaligned boxes' in err()
    assert _nms(L, scores=None) == 2 and b'scores' in err()
    assert _nms(L, keep=None) == 2 and b'keep list' in err()
    assert _nms(L, scratch=None) == 2 and b'scratch' in err()
    assert _nms(L, scratch=S + 8) == 2 and b'scratch' in err()
    need = L.deva_proposal_scratch(8)
    assert _nms(L, nbytes=need - 1) == 2 and b'scratch' in err() and str(need).encode() in err()
    assert all(b'deva_box_nms_xyxy' in (_nms(L, **kw), err())[1] for kw in (dict(n=-1), dict(boxes=None), dict(scratch=None)))

    assert _select(L, batch=-1) == 2 and b'negative batch' in err()
    for per_box in (0, 17, -3):
        assert _select(L, per_box=per_box) == 2 and b'1 to 16 planes per box' in err()
    assert _select(L, h=0) == 2 and b'bad plane size' in err()
    assert _select(L, w=-4) == 2 and b'bad plane size' in err()
    assert _select(L, h=40000, w=40000) == 2 and b'bad plane size' in err()
    assert _select(L, thr=float('nan')) == 2 and b'not a number' in err()
    assert _select(L, logits=None) == 2 and b'logits' in err()
    assert _select(L, logits=A + 2) == 2 and b'misaligned logits' in err()
    assert _select(L, scores=None) == 2 and b'scores' in err()
    assert _select(L, scores=A + 1) == 2 and b'misaligned scores' in err()
    assert _select(L, out=None) == 2 and b'null output' in err()
    assert _select(L, chosen=A + 2) == 2 and b'choice list' in err()
    assert _select(L, batch=1 << 30, per_box=2) == 2 and b'2^30 planes' in err()
    assert all(b'deva_box_mask_select' in (_select(L, **kw), err())[1] for kw in (dict(batch=-1), dict(h=0), dict(out=None)))
    # nothing to do: no launch, nothing dereferenced (a null stream handle and made-up addresses)
    assert _select(L, batch=0, logits=None, scores=None, out=None, chosen=None) == 0


def test_wrapper_errors_before_any_launch():
    """the wrappers check shapes and sizes first, then refuse host tensors: no CPU path"""
    from deva.hip import DevaHipError, ops
    boxes, scores = torch.zeros(5, 4), torch.zeros(5)
    with pytest.raises(DevaHipError, match=r'M,4'):
        ops.box_nms_xyxy(boxes.view(-1), scores, 0.5)
    with pytest.raises(DevaHipError, match=r'scores must be fp32 \[5\]'):
        ops.box_nms_xyxy(boxes, scores[:4], 0.5)
    with pytest.raises(DevaHipError, match='at most 4096 boxes'):
        ops.box_nms_xyxy(torch.zeros(4097, 4), torch.zeros(4097), 0.5)
    with pytest.raises(DevaHipError, match='not a number'):
        ops.box_nms_xyxy(boxes, scores, float('nan'))
    with pytest.raises(DevaHipError, match='HIP device'):
        ops.box_nms_xyxy(boxes, scores, 0.5)
    logits, s = torch.zeros(2, 3, 8, 12), torch.zeros(2, 3)
    with pytest.raises(DevaHipError, match=r'B,M,H,W'):
        ops.box_mask_select(logits[0], s)
    with pytest.raises(DevaHipError, match='1 to 16 planes per box'):
        ops.box_mask_select(torch.zeros(2, 17, 8, 12), torch.zeros(2, 17))
    with pytest.raises(DevaHipError, match=r'scores must be fp32 \[2,3\]'):
        ops.box_mask_select(logits, s[:1])
    with pytest.raises(DevaHipError, match='not a number'):
        ops.box_mask_select(logits, s, float('nan'))
    with pytest.raises(DevaHipError, match=r'`out` must be uint8 \[2,8,12\]'):
        ops.box_mask_select(logits, s, out=torch.zeros(2, 8, 12))
    with pytest.raises(DevaHipError, match='HIP device'):
        ops.box_mask_select(logits, s)


# ------------------------------------------------------------------------------------------ the rules by hand
def test_choice_rules_by_hand():
    nan = float('nan')
    assert ET.choice([0.1, 0.9, 0.2]) == 1
    assert ET.choice([0.9, 0.9, 0.2]) == 0 and ET.choice([0.2, 0.9, 0.9]) == 1          # the first maximum
    assert ET.choice([0.5, nan, 0.9, nan]) == 1 and ET.choice([nan, 2.0]) == 0          # the first NaN
    assert ET.choice([-0.0, 0.0]) == 0 and ET.choice([0.0, -0.0]) == 0                  # -0.0 == 0.0
    assert ET.choice([-np.inf, -np.inf]) == 0 and ET.choice([-np.inf, np.inf, np.inf]) == 1
    assert ET.choice([-3.0]) == 0
    for s in ([0.1, 0.9, 0.2], [0.5, nan, 0.9, nan], [-0.0, 0.0], [0.0, -0.0], [0.2, 0.9, 0.9], [-np.inf, np.inf, np.inf]):
        assert ET.choice(s) == int(np.argmax(np.array(s, dtype=F)))                     # numpy's own argmax


def test_select_rules_by_hand():
    nan, inf = float('nan'), float('inf')
    logits = np.zeros((2, 3, 2, 4), dtype=F)
    logits[0, 1] = [[0.5, 0.25, nan, inf], [-inf, 0.2500001, -0.0, 0.0]]
    logits[0, 0], logits[0, 2] = nan, inf                                               # not chosen: never looked at
    logits[1, 2] = [[1, -1, 1, -1], [nan, nan, 2, 0]]
    scores = np.array([[0.1, 0.9, 0.2], [0.3, 0.3, 0.31]], dtype=F)
    planes, chosen = ET.mask_select(logits, scores, 0.25)
    assert chosen.tolist() == [1, 2] and planes.dtype == np.uint8
    assert planes[0].tolist() == [[1, 0, 0, 1], [0, 1, 0, 0]]                           # strict: 0.25 > 0.25 is false; NaN -> 0
    assert planes[1].tolist() == [[1, 0, 1, 0], [0, 0, 1, 0]]
    # the threshold is rounded to fp32 once: 0.1 (double) against fp32(0.1) is not above
    planes, _ = ET.mask_select(np.full((1, 1, 1, 2), F(0.1)), np.zeros((1, 1), dtype=F), 0.1)
    assert planes.tolist() == [[[0, 0]]]
    planes, chosen = ET.mask_select(np.zeros((0, 3, 2, 4), dtype=F), np.zeros((0, 3), dtype=F))
    assert planes.shape == (0, 2, 4) and chosen.shape == (0,)


def test_nms_xyxy_on_integer_boxes_is_the_integer_nms():
    for m in (1, 7, 64, 130, 400):
        rng = np.random.default_rng(m)
        x0, y0 = rng.integers(0, 24, m), rng.integers(0, 24, m)
        boxes = np.stack([x0, y0, x0 + rng.integers(0, 12, m), y0 + rng.integers(0, 12, m)], 1).astype(np.int32)
        boxes[rng.integers(0, m, m // 3)] = boxes[rng.integers(0, m, m // 3)]
        boxes[rng.integers(0, m, m // 10), 2:] = 0
        scores = rng.choice(np.array([0.5, 0.75, 0.9, 0.9, 1.0], dtype=F), m)
        if m >= 64:
            scores[rng.integers(0, m, 3)] = np.nan
            scores[rng.integers(0, m, 3)] = -0.0
        for thresh in (0.8, 0.5, 0.0):
            assert ET.nms_xyxy(boxes.astype(F), scores, thresh) == EP.nms(boxes, scores, thresh)


def test_nms_rules_by_hand():
    box = lambda *v: list(v)
    # an inverted box has a negative area (N1): with a box it "overlaps" by max(0, .) = 0 -> ovr = 0 / (a + b) -> kept
    boxes = np.array([box(0, 0, 10, 10), box(8, 8, 2, 2), box(0.5, 0.5, 10.5, 10.5)], dtype=F)
    assert ET.nms_xyxy(boxes, np.array([0.9, 0.8, 0.7], dtype=F), 0.5) == [0, 1]       # 2 overlaps 0 by 0.82
    # zero-area boxes: two identical points give 0 / 0 = NaN, which suppresses nothing (N3)
    boxes = np.array([box(3, 3, 3, 3), box(3, 3, 3, 3), box(0, 0, 6, 6)], dtype=F)
    assert ET.nms_xyxy(boxes, np.array([0.9, 0.8, 0.7], dtype=F), 0.0) == [0, 1, 2]
    # an inverted box inside a box: area_i + area_j - inter can be 0 or negative; inter = 0 -> 0 / negative = -0 -> kept
    boxes = np.array([box(0, 0, 4, 4), box(4, 0, 0, 4)], dtype=F)                       # areas 16 and -16: 0 / 0
    assert ET.nms_xyxy(boxes, np.array([0.5, 0.5], dtype=F), 0.0) == [0, 1]
    # strict: an overlap equal to the threshold does not suppress; fractional coordinates are taken as given
    boxes = np.array([box(0, 0, 2, 1), box(1, 0, 3, 1)], dtype=F)                       # inter 1, union 3: fp32(1/3)
    third = float(F(1) / F(3))
    assert ET.nms_xyxy(boxes, np.array([0.9, 0.8], dtype=F), third) == [0, 1]
    assert ET.nms_xyxy(boxes, np.array([0.9, 0.8], dtype=F), float(np.nextafter(F(third), F(0)))) == [0]
    boxes = np.array([box(0.25, 0.5, 10.25, 10.5), box(0.75, 0.5, 10.75, 10.5)], dtype=F)
    assert ET.nms_xyxy(boxes, np.array([0.5, 0.5], dtype=F), 0.9) == [0]                # 9.5 / 10.5 = 0.905; the lower index
    assert ET.nms_xyxy(boxes, np.array([0.5, 0.5], dtype=F), 0.91) == [0, 1]
    # order (N4): NaN first, then descending, -0.0 == 0.0 by index
    far = np.array([box(20 * k, 0, 20 * k + 5, 5) for k in range(5)], dtype=F)
    assert ET.nms_xyxy(far, np.array([0.0, np.nan, -0.0, 0.7, np.nan], dtype=F), 0.5) == [1, 4, 3, 0, 2]
    assert ET.nms_xyxy(np.zeros((0, 4), dtype=F), np.zeros(0, dtype=F), 0.5) == []


# ------------------------------------------------------------------------------------------ text_detections
class ReplaySegmenter:
    """answers a box with the logits the golden file recorded for it (matched by its bits)"""
    mask_threshold = 0.0

    def __init__(self, golden, device='cpu'):
        self.rows = {}
        for k, g in enumerate(golden['boxes']):
            self.rows.setdefault(g.tobytes(), k)                    # (a duplicate box has the answer of its first copy)
        self.logits, self.scores = torch.from_numpy(golden['logits']), torch.from_numpy(golden['scores'])
        self.calls, self.device = [], device

    def predict_boxes(self, boxes_px):
        rows = [self.rows[b.tobytes()] for b in boxes_px.cpu().numpy()]
        self.calls.append(rows)
        return self.logits[rows].contiguous().to(boxes_px.device), self.scores[rows].contiguous().to(boxes_px.device)


def golden_inputs(golden):
    classes = np.array([None if c < 0 else int(c) for c in golden['class_ids']], dtype=object)
    return golden['boxes'], golden['confidences'], classes


def check_against_golden(golden, device):
    """shared with tests/test_gpu_s_text.py: `text_detections` reproduces what the reference's segment_with_text produced"""
    from deva.inference import detections as D
    boxes, conf, classes = golden_inputs(golden)
    assert np.array_equal(boxes, TC.golden_inputs()[0]) and len(boxes) == 12                # the recipe has not drifted
    for min_side in TC.GOLDEN_MIN_SIDES:
        key = f'min_side_{min_side}'
        h, w = TC.GOLDEN_HW
        size = D.detection_size(h, w, min_side)
        segmenter = ReplaySegmenter(golden)
        mask, info = D.text_detections(boxes, conf, classes, segmenter, (h, w), size, nms_threshold=TC.NMS_THRESHOLD,
                                       boxes_per_batch=4, device=device)
        want = golden[key + '/mask']
        assert mask.dtype == torch.int64 and tuple(mask.shape) == want.shape == size
        assert np.array_equal(mask.cpu().numpy(), want.astype(np.int64)), key
        assert [o.id for o in info] == golden[key + '/ids'].tolist()
        assert [-1 if o.category_ids[0] is None else o.category_ids[0] for o in info] == golden[key + '/categories'].tolist()
        assert [float(o.scores[0]) for o in info] == golden[key + '/scores'].tolist()
        assert segmenter.calls == [[1, 9, 4, 10], [11, 7]]                                  # keep order, batches of 4
    # the case holds what it promises: a None class passes through, one segment is painted over completely (its id is
    # in the list and not in the mask), one best mask is empty (6 boxes kept, 5 segments)
    assert None in [o.category_ids[0] for o in info] and golden['min_side_0/categories'].tolist().count(-1) == 1
    ids = golden['min_side_0/ids'].tolist()
    assert len(ids) == 5 and sorted(set(np.unique(golden['min_side_0/mask']).tolist()) - {0}) == [1, 3, 4, 5]


def test_text_detections_reproduces_the_reference(emu, golden_dir):
    golden = np.load(os.path.join(golden_dir, 'text_segmentation.npz'))
    check_against_golden(golden, 'cpu')
    # the choices of the case: the best index differs between boxes, one is a tie, one best mask is empty; no two
    # areas are equal (the reference's own order among equal areas depends on the machine: tests/text_case.py)
    planes, chosen = ET.mask_select(golden['logits'], golden['scores'])
    assert chosen.tolist() == [1, 1, 1, 0, 0, 0, 1, 1, 1, 1, 0, 0]
    assert golden['scores'][9].tolist() == [F(0.7), F(0.9), F(0.9)]
    areas = [int(planes[k].sum()) for k in (1, 9, 4, 10, 11, 7)]
    assert len(set(areas)) == 6 and areas[-1] == 0


def test_equal_areas_are_painted_in_the_fixed_order(emu):
    """two kept masks of equal areas: the higher index is painted first (include/deva_hip.h, policy 2) -- `left`, which
    NMS keeps after `right`, takes the lower id"""
    from deva.inference import detections as D
    boxes, conf, classes = TC.golden_inputs(equal_halves=True)
    h, w = TC.GOLDEN_HW
    segmenter = TC.FakeBoxSegmenter()
    segmenter.set_image(np.zeros((h, w, 3), dtype=np.uint8))
    mask, info = D.text_detections(boxes, conf, classes, segmenter, (h, w), (h, w), nms_threshold=TC.NMS_THRESHOLD, device='cpu')
    kept = np.concatenate(segmenter.asked())
    assert [b.tolist() for b in kept[3:5]] == [boxes[10].tolist(), boxes[11].tolist()]      # right, then left
    planes, _ = ET.mask_select(*(np.stack(v) for v in zip(*(TC.box_answer(b, h, w) for b in kept))))
    assert int(planes[3].sum()) == int(planes[4].sum()) > 0
    assert [o.category_ids[0] for o in info] == [1, 0, 0, 1, None]                          # main 1, main 0, left, right, part
    left_only = (planes[4] == 1) & (planes[3] == 0) & (planes[1] == 0)
    assert np.array_equal(mask.numpy() == 3, left_only) and int(left_only.sum()) > 0        # right and part paint over it
    assert 2 not in mask.unique().tolist()                                                  # main 0: painted over completely


def test_tensors_and_numpy_are_the_same_call(emu, golden_dir):
    from deva.inference import detections as D
    golden = np.load(os.path.join(golden_dir, 'text_segmentation.npz'))
    boxes, conf, classes = golden_inputs(golden)
    h, w = TC.GOLDEN_HW
    a = D.text_detections(boxes, conf, classes, ReplaySegmenter(golden), (h, w), (h, w), nms_threshold=0.8, device='cpu')
    b = D.text_detections(torch.from_numpy(boxes), torch.from_numpy(conf), list(classes), ReplaySegmenter(golden), (h, w), (h, w),
                          nms_threshold=0.8, device='cpu')
    arena = torch.full((8, h, w), 7, dtype=torch.uint8)
    c = D.text_detections(boxes, conf, classes, ReplaySegmenter(golden), (h, w), (h, w), nms_threshold=0.8, capacity=8, arena=arena)
    for mask, info in (b, c):
        assert torch.equal(mask, a[0]) and [(o.id, o.category_ids, o.scores) for o in info] == [(o.id, o.category_ids, o.scores) for o in a[1]]
    assert bool((arena[6:] == 7).all()) and int(arena[:6].max()) == 1                       # the planes went into the arena


def test_capacity_error_arrives_before_the_segmenter_is_asked(emu, golden_dir):
    from deva.hip import DevaHipError
    from deva.inference import detections as D
    golden = np.load(os.path.join(golden_dir, 'text_segmentation.npz'))
    boxes, conf, classes = golden_inputs(golden)
    h, w = TC.GOLDEN_HW
    segmenter = ReplaySegmenter(golden)
    with pytest.raises(DevaHipError, match=r'\b6 boxes are left after NMS, the arena holds 5\b'):
        D.text_detections(boxes, conf, classes, segmenter, (h, w), (h, w), nms_threshold=0.8, capacity=5, device='cpu')
    assert segmenter.calls == []
    D.text_detections(boxes, conf, classes, segmenter, (h, w), (h, w), nms_threshold=0.8, capacity=6, device='cpu')
    assert sum(len(c) for c in segmenter.calls) == 6


def test_no_boxes_and_none_kept(emu):
    from deva.inference import detections as D

    class Untouchable:
        def __getattr__(self, name):
            raise AssertionError(f'the segmenter was asked for {name}')

    mask, info = D.text_detections(np.zeros((0, 4), dtype=F), np.zeros(0, dtype=F), np.zeros(0, dtype=object), Untouchable(),
                                   (48, 64), (30, 40), nms_threshold=0.8, device='cpu')
    assert info == [] and mask.dtype == torch.int64 and tuple(mask.shape) == (30, 40) and int(mask.abs().sum()) == 0
    with pytest.raises(ValueError, match='2 boxes, 1 confidences'):
        D.text_detections(np.zeros((2, 4), dtype=F), np.zeros(1, dtype=F), [0, 1], Untouchable(), (48, 64), (48, 64),
                          nms_threshold=0.8, device='cpu')


# ------------------------------------------------------------------------------------------ the frame loop
def emulated_core_factory(recipe_state_dict):
    from deva.inference.inference_core import DEVAInferenceCore
    from deva.model.network import DEVA
    net = DEVA(TC.loop_config('online'))
    net.load_weights(recipe_state_dict[0])
    return lambda setting: DEVAInferenceCore(net, TC.loop_config(setting))


@pytest.mark.parametrize('setting', ['online', 'semionline'])
def test_processor_is_the_restated_reference_loop(setting, emu, recipe_state_dict, monkeypatch):
    make_core = emulated_core_factory(recipe_state_dict)
    got, flushed, processor, keywords = TC.check_clip(setting, make_core, monkeypatch)
    assert keywords == [{}, {}, {}]                                               # never `incremental`
    if setting == 'semionline':
        # 13 frames, windows voted at 2, 7 and 12: nothing is left; a clip that ends inside a window is flushed
        assert flushed == [] and processor.next_voting_frame == 17
        frames, rects = TC.clip()
        names = [f'{t:05d}.jpg' for t in range(len(frames))]
        _, flushed, processor = TC.run_processor(make_core(setting), TC.FakeDetector(frames, rects, TC.HALVES),
                                                 TC.FakeBoxSegmenter(), frames[:7], names[:7])
        assert [n for n, _ in flushed] == names[5:7] and processor.next_voting_frame == 7
    else:
        assert flushed == []


def test_no_forward_mask_is_estimated(emu, recipe_state_dict, monkeypatch):
    from deva.inference import detections as D
    monkeypatch.setattr(D, 'estimate_forward_mask', lambda *a, **k: (_ for _ in ()).throw(AssertionError('forward mask')))
    frames, rects = TC.clip()
    core = emulated_core_factory(recipe_state_dict)('online')
    detector, segmenter = TC.FakeDetector(frames, rects, TC.HALVES), TC.FakeBoxSegmenter()
    from deva.inference.with_text import TextPromptedProcessor
    processor = TextPromptedProcessor(core, detector, segmenter, boxes_per_batch=2)
    for ti in range(6):
        out = processor.process_frame(frames[ti], ti, f'{ti}.jpg')
        assert len(out) == 1 and out[0][0] == f'{ti}.jpg'
    kinds = [c[0] for c in segmenter.calls]
    assert kinds[:2] == ['set_image', 'predict_boxes'] and kinds.count('set_image') == 2 and kinds.count('reset_image') == 2
    assert all(len(b) <= 2 for b in segmenter.asked()) and sum(len(b) for b in segmenter.asked()) == 4 + 4
    assert processor.prompts == ['person', 'dog', 'a hat']


def test_a_missing_key_is_named(emu, recipe_state_dict):
    from deva.inference.with_text import CONFIG_KEYS, TextPromptedProcessor
    assert set(CONFIG_KEYS) == {'size', 'temporal_setting', 'num_voting_frames', 'detection_every', 'prompt', 'DINO_THRESHOLD',
                                'DINO_NMS_THRESHOLD'}
    core = emulated_core_factory(recipe_state_dict)('online')
    full = dict(core.config)
    for key in CONFIG_KEYS:
        core.config = {k: v for k, v in full.items() if k != key}
        with pytest.raises(KeyError, match=key):
            TextPromptedProcessor(core, object(), object())
    core.config = dict(full, temporal_setting='offline')
    with pytest.raises(ValueError, match='temporal_setting'):
        TextPromptedProcessor(core, object(), object())
    import deva.inference.with_text as M
    src = open(M.__file__).read()
    banned = r'^\s*(?:import|from)\s+(?:cv2|segment_anything|torchvision|groundingdino|supervision|deva\.ext|deva\.inference\.(?:frame_utils|result_utils|demo_utils))\b'
    assert not re.search(banned, src, flags=re.M)
