"""The proposal filter without a GPU: the entry points on the ABI and their argument errors, `ProposalFilter` on the
emulated ops (tests/emu_proposals.py) through to `assemble_automatic` and `incorporate_detection`, and hand-made cases
of every rule of the contract (include/deva_hip.h, deva_proposal_batch)."""
import os

import numpy as np
import pytest
import torch

import abi_util
import emu_detections as ED
import emu_ops
import emu_proposals as EP
import proposal_case as PC
from workload import synth

torch.set_grad_enabled(False)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('deva_proposal_scratch', 'deva_proposal_begin', 'deva_proposal_batch', 'deva_proposal_finish',
         'deva_proposal_gather', 'deva_box_nms')


@pytest.fixture()
def emu(monkeypatch):
    emu_ops.install(monkeypatch)
    ED.install(monkeypatch)
    EP.install(monkeypatch)


# ------------------------------------------------------------------------------------------ ABI
def test_entry_points_are_exported_declared_and_bound():
    from deva.hip import ops
    header = abi_util.inference_entry_points(NAMES)
    for name in ('proposal_state', 'proposal_begin', 'proposal_batch', 'proposal_finish', 'box_nms'):
        assert name in ops.__all__
    for ref in ('automatic_mask_generator.py:332-352', 'automatic_mask_generator.py:272-278', 'automatic_sam.py:26-40'):
        assert ref in header, ref


A, S = 1 << 30, 1 << 20   # made-up addresses: validation fails before anything is dereferenced or launched


def _batch(L, logits=A, iou=A, b=3, h=8, w=8, p=0.88, s=0.95, o=1.0, m=0.0, arena=A, cap=16, scratch=S, nbytes=1 << 24):
    return L.deva_proposal_batch(logits, iou, b, h, w, p, s, o, m, arena, cap, scratch, nbytes, None)


def test_argument_errors_before_any_launch():
    from deva import hip
    L = hip.lib()
    err = L.deva_hip_last_error
    nan = float('nan')
    assert _batch(L, logits=None) == 2 and b'logits' in err()
    assert _batch(L, logits=A + 2) == 2 and b'misaligned logits' in err()
    assert _batch(L, iou=None) == 2 and b'predicted IoUs' in err()
    assert _batch(L, b=-1) == 2 and b'negative batch' in err()
    assert _batch(L, h=0) == 2 and b'plane size' in err()
    assert _batch(L, h=1 << 16, w=1 << 15) == 2 and b'plane size' in err()
    for name in 'psom':
        assert _batch(L, **{name: nan}) == 2 and b'not a number' in err()
    assert _batch(L, arena=None) == 2 and b'null arena' in err()
    assert _batch(L, cap=0) == 2 and b'capacity' in err()
    assert _batch(L, cap=4097) == 2 and b'4096' in err()
    assert _batch(L, scratch=None) == 2 and b'scratch' in err()
    assert _batch(L, scratch=S + 8) == 2 and b'scratch' in err()          # not 16-byte aligned
    need = L.deva_proposal_scratch(16)
    assert _batch(L, nbytes=need - 1) == 2 and b'scratch' in err()
    assert L.deva_proposal_begin(16, S, need - 1, None) == 2 and b'deva_proposal_begin' in err()
    assert L.deva_proposal_begin(0, S, need, None) == 2 and b'capacity' in err()
    assert L.deva_proposal_finish(16, 0.7, S, need, None, None) == 2 and b'result' in err()
    assert L.deva_proposal_finish(16, nan, S, need, A, None) == 2 and b'NMS threshold' in err()
    assert L.deva_proposal_finish(16, 0.7, S, need - 1, A, None) == 2 and b'scratch' in err()
    assert L.deva_proposal_gather(A, 16, 8, 8, S, need, 17, A, None) == 2 and b'kept' in err()
    assert L.deva_proposal_gather(A, 16, 8, 8, S, need, -1, A, None) == 2 and b'kept' in err()
    assert L.deva_proposal_gather(A, 16, 8, 8, S, need, 3, None, None) == 2 and b'null output' in err()
    assert L.deva_proposal_gather(None, 16, 8, 8, S, need, 3, A, None) == 2 and b'null arena' in err()
    assert L.deva_proposal_gather(A, 16, 0, 8, S, need, 3, A, None) == 2 and b'plane size' in err()
    assert L.deva_box_nms(A, A, 4097, 0.7, S, 1 << 24, A, A, None) == 2 and b'4096' in err()
    assert L.deva_box_nms(A, A, -1, 0.7, S, 1 << 24, A, A, None) == 2 and b'negative' in err()
    assert L.deva_box_nms(None, A, 5, 0.7, S, 1 << 24, A, A, None) == 2 and b'boxes' in err()
    assert L.deva_box_nms(A, None, 5, 0.7, S, 1 << 24, A, A, None) == 2 and b'scores' in err()
    assert L.deva_box_nms(A, A, 5, nan, S, 1 << 24, A, A, None) == 2 and b'NMS threshold' in err()
    assert L.deva_box_nms(A, A, 5, 0.7, S, 1 << 24, None, A, None) == 2 and b'keep list' in err()
    assert L.deva_box_nms(A, A, 5, 0.7, S, 1 << 24, A, None, None) == 2 and b'keep count' in err()
    assert L.deva_box_nms(A, A, 5, 0.7, S, L.deva_proposal_scratch(5) - 1, A, A, None) == 2 and b'scratch' in err()
    assert L.deva_proposal_scratch(0) == -1 and L.deva_proposal_scratch(4097) == -1 and L.deva_proposal_scratch(-3) == -1
    # small tables and the suppression matrix (4096 x 64 words): no copy of a plane
    assert 4096 * 64 * 8 < L.deva_proposal_scratch(4096) < 4096 * 64 * 8 + (1 << 18)
    assert 0 < L.deva_proposal_scratch(1) < 1 << 16


def test_wrapper_errors_before_any_launch():
    """the wrappers check shapes and sizes first, then refuse host tensors: no CPU path"""
    from deva.hip import DevaHipError, ops
    from deva.inference.proposals import ProposalFilter
    with pytest.raises(DevaHipError, match='capacity'):
        ProposalFilter(8, 8, capacity=0)
    with pytest.raises(DevaHipError, match='capacity'):
        ProposalFilter(8, 8, capacity=4097)
    with pytest.raises(DevaHipError, match='frame size'):
        ProposalFilter(0, 8, capacity=4)
    with pytest.raises(TypeError):
        ProposalFilter(8, 8)                                  # no hidden default
    with pytest.raises(DevaHipError, match='HIP device'):
        ProposalFilter(8, 8, capacity=4).add(torch.zeros(2, 8, 8), torch.zeros(2))
    with pytest.raises(DevaHipError, match='no batch'):
        ProposalFilter(8, 8, capacity=4).finish()
    with pytest.raises(DevaHipError, match=r'M,4'):
        ops.box_nms(torch.zeros(3, 5, dtype=torch.int32), torch.zeros(3), 0.7)
    with pytest.raises(DevaHipError, match='scores'):
        ops.box_nms(torch.zeros(3, 4, dtype=torch.int32), torch.zeros(2), 0.7)
    with pytest.raises(DevaHipError, match='4096'):
        ops.box_nms(torch.zeros(4097, 4, dtype=torch.int32), torch.zeros(4097), 0.7)
    with pytest.raises(DevaHipError, match='HIP device'):
        ops.box_nms(torch.zeros(3, 4, dtype=torch.int32), torch.zeros(3), 0.7)


# ------------------------------------------------------------------------------------------ the rules, by hand
def _filter(planes, iou, capacity=16, **over):
    from deva.inference.proposals import ProposalFilter
    h, w = planes.shape[1:]
    flt = ProposalFilter(h, w, capacity=capacity, **over)
    flt.add(planes, torch.tensor(iou, dtype=torch.float32))
    return flt.finish()


def _steps(counts, h=6, w=10):
    """planes with n_hi pixels at 2, up to n_lo at exactly 1 (= t_hi), the rest at exactly -1 (= t_lo)"""
    return torch.stack([PC.step_plane(h, w, n_hi, n_lo, (1, 1)) for n_hi, n_lo in counts])


def test_nineteen_of_twenty_pass_095_and_the_comparisons_are_strict(emu):
    found = _filter(_steps([(19, 20), (18, 20), (20, 20)]), [0.9, 0.9, 0.9], box_nms_thresh=2.0)
    assert found.index.tolist() == [0, 1] and found.masks.shape[0] == 2    # 18 / 20 = 0.9 is dropped; index = arrival among the stored
    assert found.stability.view(torch.int32).tolist() == torch.tensor([0.95, 1.0]).view(torch.int32).tolist()
    # the pixel at exactly t_hi = 1 does not count in hi; the background at exactly t_lo = -1 does not count in lo;
    # a logit of exactly the mask threshold is not set
    assert int(found.masks[0].sum()) == 20 and found.boxes[0].tolist() == [1, 1, 5, 4]
    zero = _steps([(19, 20)])
    zero[0, 0, 0] = 0.0                                                     # above t_lo: 19 / 21 now, and not in the mask
    assert _filter(zero, [0.9]).masks.shape[0] == 0
    kept = _filter(zero, [0.9], stability_score_thresh=0.9)
    assert kept.masks[0, 0, 0] == 0 and int(kept.masks.sum()) == 20
    assert found.masks.dtype == torch.uint8 and found.iou_preds.dtype == torch.float32 and found.boxes.dtype == torch.int32


def test_lo_zero_drops_and_a_disabled_drop_keeps_it(emu):
    planes = torch.full((2, 6, 10), -1.0)
    planes[1, 2, 3] = 5.0
    only = _filter(planes, [0.9, 0.9])                                      # 0 / 0 is NaN: dropped
    assert only.index.tolist() == [0] and only.boxes.tolist() == [[3, 2, 3, 2]]
    found = _filter(planes, [0.9, 0.95], stability_score_thresh=0.0)       # <= 0: no stability drop at all
    assert found.index.tolist() == [1, 0] and torch.isnan(found.stability[1]) and found.stability[0] == 1.0
    assert found.boxes.tolist() == [[3, 2, 3, 2], [0, 0, 0, 0]]


def test_threshold_at_or_below_zero_disables_the_iou_drop(emu):
    planes = _steps([(20, 20)] * 4)
    iou = [0.5, float('nan'), -1.0, 0.95]
    assert _filter(planes, iou, box_nms_thresh=2.0).iou_preds.tolist() == [torch.tensor(0.95).item()]
    for thresh in (0.0, -0.5):
        found = _filter(planes, iou, pred_iou_thresh=thresh, box_nms_thresh=2.0)
        assert found.index.tolist() == [1, 3, 0, 2]                        # NaN first, as torch sorts descending
    assert _filter(planes, iou, pred_iou_thresh=1e-60, box_nms_thresh=2.0).iou_preds.tolist() == [torch.tensor(0.95).item(), 0.5]   # > 0.0: on, at fp32(0)


def test_an_empty_mask_has_box_zero_and_is_never_suppressed(emu):
    planes = torch.full((3, 6, 10), -0.5)                                   # above t_lo everywhere: lo = 60, hi = 0
    planes[2, 0, 0:2] = 3.0
    planes[2, 1, 0:2] = 3.0
    found = _filter(planes, [0.9, 0.9, 0.95], stability_score_thresh=0.0, box_nms_thresh=0.0)
    # two empty masks with the same box 0,0,0,0: ovr = 0 / 0 = NaN, which suppresses nothing, even at a threshold of 0
    assert found.index.tolist() == [2, 0, 1] and found.boxes.tolist() == [[0, 0, 1, 1], [0, 0, 0, 0], [0, 0, 0, 0]]


def test_a_one_pixel_wide_mask_has_area_zero(emu):
    planes = torch.full((3, 8, 10), -1.0)
    planes[0, 1:7, 4] = 3.0                                                 # a column: (x1 - x0) = 0
    planes[1, 1:7, 4] = 3.0                                                 # the same column again
    planes[2, 1:7, 4:6] = 3.0                                               # two columns: area 1 * 5, the column inside it
    found = _filter(planes, [0.95, 0.9, 0.9], box_nms_thresh=0.5)
    assert found.index.tolist() == [0, 1, 2]                               # 0 / 0 and 0 / 5: nothing is suppressed
    assert EP.nms([[4, 1, 4, 6], [4, 1, 5, 6], [4, 1, 5, 6]], [0.9, 0.8, 0.7], 0.5) == [0, 1]  # 5 / 5 > 0.5


def test_tie_order_among_equal_predictions(emu):
    a, b = [2, 2, 8, 8], [3, 3, 9, 9]                                       # inter 25, union 47: 0.53
    assert EP.nms([a, b, a, b], [0.9, 0.9, 0.9, 0.9], 0.5) == [0]          # the lower index wins
    assert EP.nms([b, a], [0.9, 0.9], 0.5) == [0]
    assert EP.nms([a, b, a], [0.8, 0.9, 0.9], 0.6) == [1, 2]               # descending first; a suppresses its copy
    assert EP.nms([a, b], [0.0, -0.0], 0.9) == [0, 1]                      # 0.0 == -0.0: a tie
    assert EP.nms(np.zeros((0, 4)), [], 0.5) == []
    planes = torch.full((3, 12, 12), -1.0)
    planes[0, 3:10, 3:10] = planes[1, 2:9, 2:9] = planes[2, 3:10, 3:10] = 3.0
    found = _filter(planes, [0.9, 0.9, 0.9], box_nms_thresh=0.5)
    assert found.index.tolist() == [0] and found.boxes.tolist() == [[3, 3, 9, 9]]
    # the threshold comparison is (double)ovr > thresh: fp32(25 / 47) against the double 25 / 47
    ovr = np.float32(25) / np.float32(47)
    assert EP.nms([a, b], [0.9, 0.8], float(ovr)) == [0, 1] and EP.nms([a, b], [0.9, 0.8], np.nextafter(float(ovr), 0)) == [0]


def test_overflow_raises_with_the_count_and_reset_recovers(emu):
    from deva.hip import DevaHipError
    from deva.inference.proposals import ProposalFilter
    flt = ProposalFilter(6, 10, capacity=4)
    planes = _steps([(20, 20)] * 9 + [(1, 20)])
    iou = torch.full((10,), 0.9)
    flt.add(planes[:6], iou[:6])
    flt.add(planes[6:], iou[6:])
    with pytest.raises(DevaHipError, match=r'\b9 masks passed'):
        flt.finish()
    flt.add(planes[:3], iou[:3])
    assert flt.finish().masks.shape[0] == 1                                 # three copies of one box
    flt.add(planes, iou)
    flt.reset()
    flt.add(planes[8:], iou[8:])
    assert flt.finish().index.tolist() == [0]


def test_recipe_cases_decide_what_they_are_built_for():
    for h, w in PC.GEOMETRIES:
        PC.check_case(h, w, 0.95)
    PC.check_case(29, 53, 0.8)
    for b in PC.BATCHES:                  # one batch of every frame leaves nothing, one is empty
        sizes = [x.shape[0] for x, _ in PC.frame(29, 53, b)]
        assert sorted(sizes) == sorted([b, 4, 0])


# ------------------------------------------------------------------------------------------ through the core
def test_filter_to_assembly_to_the_core(emu, recipe_state_dict):
    """a short clip on the emulated core whose detections arrive as raw logit batches: ProposalFilter ->
    assemble_automatic -> incorporate_detection"""
    from deva.inference import detections as D
    from deva.inference.inference_core import DEVAInferenceCore
    from deva.inference.proposals import ProposalFilter
    from deva.model.network import DEVA
    cfg = synth.base_config(mem_every=2, max_missed_detection_count=1, max_num_objects=-1)
    net = DEVA(cfg)
    net.load_weights(recipe_state_dict[0])
    h, w = 96, 128
    core = DEVAInferenceCore(net, cfg)
    flt = ProposalFilter(h, w, capacity=64, stability_score_thresh=0.8)
    frames = [f for f, _ in zip(iter(synth.FrameStream(h, w, seed=2).next, None), range(3))]
    seen = []
    for t, frame in enumerate(frames):
        if t % 2 == 0:
            for logits, iou in (PC.batch(h, w, 12, 40 + t, 0.8), PC.barren(h, w, t), PC.batch(h, w, 5, 50 + t, 0.8)):
                flt.add(logits, iou)
            found = flt.finish()
            assert found.masks.shape[0] >= 3 and found.masks.dtype == torch.uint8
            assert found.iou_preds.tolist() == sorted(found.iou_preds.tolist(), reverse=True)
            mask, info = D.assemble_automatic(found.masks, found.iou_preds, suppress_small_objects=True)
            assert len(info) >= 2 and set(mask.unique().tolist()) - {0} == {o.id for o in info}
            assert set(float(o.scores[0]) for o in info) <= set(found.iou_preds.tolist())
            prob = core.incorporate_detection(frame, mask, info)
            seen.append(len(info))
        else:
            prob = core.step(frame)
        assert prob.shape[0] >= 2 and tuple(prob.shape[1:]) == (h, w)
    assert len(seen) == 2
