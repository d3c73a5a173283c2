"""Detector output -> (index mask, segments) without a GPU: the entry points on the ABI and their argument errors, and
`deva.inference.detections` on the emulated op (tests/emu_detections.py) against what the reference's own auto_segment
and segment_with_text returned for the same masks (tests/golden/detection_assembly.npz, made by
tests/golden/make_detection_golden.py on the case of tests/detection_case.py)."""
import os

import numpy as np
import pytest
import torch

import abi_util
import detection_case as DC
import emu_detections as ED
import emu_ops
from workload import synth

torch.set_grad_enabled(False)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('deva_detection_scratch', 'deva_detection_assemble')


@pytest.fixture()
def emu(monkeypatch):
    emu_ops.install(monkeypatch)
    ED.install(monkeypatch)


@pytest.fixture(scope='module')
def golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, 'detection_assembly.npz')))


# ------------------------------------------------------------------------------------------ ABI
def test_entry_points_are_exported_declared_and_bound():
    from deva.hip import ops
    header = abi_util.inference_entry_points(NAMES)
    assert 'detection_assemble' in ops.__all__
    for ref in ('automatic_sam.py:106-127', 'automatic_sam.py:128-143', 'grounding_dino.py:124-140'):
        assert ref in header, ref


def _call(L, masks=4096, n=3, h=8, w=8, oh=8, ow=8, policy=0, threshold=0.8, scratch=8192, nbytes=1 << 20, out=1 << 20,
          records=1 << 21):
    """made-up addresses: validation fails before anything is dereferenced or launched"""
    return L.deva_detection_assemble(masks, n, h, w, oh, ow, policy, threshold, 0, None, scratch, nbytes, out, records, None)


def test_argument_errors_before_any_launch():
    from deva import hip
    L = hip.lib()
    assert _call(L, masks=None) != 0 and b'null masks' in L.deva_hip_last_error()
    assert _call(L, n=4097) != 0 and b'4096' in L.deva_hip_last_error()
    assert _call(L, n=-1) != 0 and b'negative' in L.deva_hip_last_error()
    assert _call(L, oh=0) != 0 and b'output size' in L.deva_hip_last_error()
    assert _call(L, ow=0) != 0 and b'output size' in L.deva_hip_last_error()
    assert _call(L, h=0) != 0 and b'mask size' in L.deva_hip_last_error()
    assert _call(L, policy=3) != 0 and b'unknown policy' in L.deva_hip_last_error()
    assert _call(L, policy=-1) != 0 and b'unknown policy' in L.deva_hip_last_error()
    assert _call(L, out=None) != 0 and b'null output' in L.deva_hip_last_error()
    assert _call(L, records=None) != 0 and b'record' in L.deva_hip_last_error()
    assert _call(L, threshold=float('nan')) != 0 and b'threshold' in L.deva_hip_last_error()
    need = L.deva_detection_scratch(64, 1080, 1920, 1080, 1920)
    assert need >= 1080 * 1920 * 2 + 64 * 127 * 12
    assert need < 1080 * 1920 * 2 + (1 << 20)                     # the plane and small tables: no copy of the masks
    assert _call(L, n=64, h=1080, w=1920, oh=1080, ow=1920, nbytes=need - 1) != 0 and b'scratch' in L.deva_hip_last_error()
    assert _call(L, scratch=None) != 0 and b'scratch' in L.deva_hip_last_error()
    assert _call(L, scratch=8200) != 0 and b'scratch' in L.deva_hip_last_error()     # not 16-byte aligned
    assert L.deva_detection_scratch(4097, 8, 8, 8, 8) == -1 and L.deva_detection_scratch(3, 8, 8, 0, 8) == -1
    assert L.deva_detection_scratch(3, 1 << 16, 1 << 15, 8, 8) == -1
    assert L.deva_detection_scratch(0, 8, 8, 8, 8) == 0 and L.deva_detection_scratch(4096, 8, 12, 8, 12) > 0


def test_wrapper_errors_before_any_launch():
    """`ops.detection_assemble` checks shape, dtype and size first, then refuses host tensors: no CPU path"""
    from deva.hip import DevaHipError, ops
    masks = torch.zeros(3, 8, 8, dtype=torch.bool)
    with pytest.raises(DevaHipError, match='policy'):
        ops.detection_assemble(masks, policy='largest')
    with pytest.raises(DevaHipError, match='N,H,W'):
        ops.detection_assemble(masks[0])
    with pytest.raises(DevaHipError, match='bool, uint8 or fp32'):
        ops.detection_assemble(masks.long())
    with pytest.raises(DevaHipError, match='bad size'):
        ops.detection_assemble(masks, (0, 8))
    with pytest.raises(DevaHipError, match='4096'):
        ops.detection_assemble(torch.zeros(4097, 1, 1, dtype=torch.bool))
    with pytest.raises(DevaHipError, match='scores'):
        ops.detection_assemble(masks, scores=torch.zeros(2))
    with pytest.raises(DevaHipError, match='HIP device'):
        ops.detection_assemble(masks)
    with pytest.raises(DevaHipError, match='HIP device'):
        ops.detection_assemble(masks.float(), (16, 16), 'text')


# ------------------------------------------------------------------------------------------ against the reference
def _assemble(policy, threshold, masks, size_out, n, **kw):
    from deva.inference import detections as D
    if policy == 'text':
        return D.assemble_with_text(masks, DC.confidences(n), DC.class_ids(n), size_out)
    return D.assemble_automatic(masks, DC.scores(n), size_out, suppress_small_objects=policy == 'suppress',
                                overlap_threshold=0.8 if threshold is None else threshold, **kw)


@pytest.mark.parametrize('case', list(DC.golden_cases()), ids=lambda c: DC.golden_key(*c))
def test_assembly_matches_the_reference(case, emu, golden):
    policy, threshold, size_in, size_out, n = case
    key = DC.golden_key(*case)
    mask, info = _assemble(policy, threshold, DC.case_masks(size_in, n), size_out, n)
    assert mask.dtype == torch.int64 and tuple(mask.shape) == tuple(size_out)
    assert np.array_equal(mask.numpy(), golden[key + '/mask'].astype(np.int64))
    assert [o.id for o in info] == golden[key + '/ids'].tolist()
    assert [-1 if o.category_ids[0] is None else int(o.category_ids[0]) for o in info] == golden[key + '/categories'].tolist()
    assert [float(o.scores[0]) for o in info] == golden[key + '/scores'].tolist()      # fp32 values: exact
    assert all(len(o.scores) == 1 and o.poke_count == 0 for o in info)


def test_the_case_decides_what_it_is_built_for(golden):
    """the goldens themselves: every feature of the case is visible in the reference's answers at 24 x 36"""
    names = list(DC.NAMES)
    k08, k07 = (DC.golden_key('suppress', t, (24, 36), (24, 36), 18) for t in (0.8, 0.7))
    kept = [n for n in names if n not in ('R6', 'R7', 'Z', 'B2', 'T', 'D')]     # eaten, empty, 0.6 < 0.8, 0.7 < 0.8, duplicate
    assert len(golden[k08 + '/ids']) == len(kept) == 12 and 'B1' in kept          # 0.9 >= 0.8
    assert len(golden[k07 + '/ids']) == 13                                         # T: 7 / 10 is not < 0.7 in fp32
    scores = DC.scores(18).tolist()
    assert golden[k07 + '/scores'].tolist() == [scores[names.index(n)] for n in names if n in kept + ['T']]
    # prefer small: Z (index 9, value 10) is absent from the mask, which holds the uncompacted 1..17 around it
    kp = DC.golden_key('prefer', None, (24, 36), (24, 36), 18)
    assert np.unique(golden[kp + '/mask']).tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 11, 12, 13, 14, 15, 16, 17]
    assert golden[kp + '/ids'].tolist() == list(range(1, 17))
    # text: a listed id that no pixel holds (the duplicate D, painted first, is covered by R1)
    kt = DC.golden_key('text', None, (24, 36), (24, 36), 18)
    assert set(golden[kt + '/ids'].tolist()) - set(np.unique(golden[kt + '/mask']).tolist()) == {6}


@pytest.mark.parametrize('size_in,size_out', DC.SIZES)
def test_consistent_ids(size_in, size_out, emu, golden):
    """prefer small, consistent_ids=True: the mask's ids are exactly the ids of segments_info, and the segments are the
    reference's (same pixels, renumbered)"""
    key = DC.golden_key('prefer', None, size_in, size_out, 18)
    mask, info = _assemble('prefer', None, DC.case_masks(size_in, 18), size_out, 18, consistent_ids=True)
    ids = [o.id for o in info]
    assert ids == golden[key + '/ids'].tolist() == list(range(1, len(ids) + 1))
    assert sorted(set(np.unique(mask.numpy()).tolist()) - {0}) == ids
    ref = golden[key + '/mask'].astype(np.int64)
    present = sorted(set(np.unique(ref).tolist()) - {0})
    assert len(present) == len(ids) and present != ids          # the quirk: uncompacted in the reference's mask
    table = np.zeros(max(present) + 1, dtype=np.int64)
    table[present] = ids
    assert np.array_equal(mask.numpy(), table[ref])


def test_inputs_as_bool_uint8_and_fp32(emu, golden):
    key = DC.golden_key('suppress', 0.8, (24, 36), (48, 72), 18)
    masks = DC.case_masks((24, 36), 18)
    for m in (masks, masks.to(torch.uint8), masks.float()):
        mask, info = _assemble('suppress', 0.8, m, (48, 72), 18)
        assert np.array_equal(mask.numpy(), golden[key + '/mask']) and [o.id for o in info] == golden[key + '/ids'].tolist()


def test_detection_size():
    from deva.inference.detections import detection_size
    assert detection_size(1080, 1920, 480) == (480, 853)       # int(1920 * 480 / 1080) = int(853.33)
    assert detection_size(1920, 1080, 480) == (853, 480)
    assert detection_size(96, 128, 0) == (96, 128) and detection_size(96, 128, -1) == (96, 128)
    assert detection_size(100, 150, 48) == (48, 72)


# ------------------------------------------------------------------------------------------ forward mask
def _network(recipe_state_dict):
    from deva.model.network import DEVA
    sd, _ = recipe_state_dict
    net = DEVA(synth.base_config())
    net.load_weights(sd)
    return net


def test_estimate_forward_mask_leaves_no_trace(emu, recipe_state_dict):
    """on the emulated core, at a size that needs padding: the forward mask is the argmax of `_segment`'s probabilities,
    unpadded; the steps that follow are bit-identical to a run without the call, and so are the usage counters"""
    from deva.inference.detections import estimate_forward_mask
    from deva.inference.inference_core import DEVAInferenceCore
    from deva.utils.tensor_utils import pad_divide_by, unpad
    net = _network(recipe_state_dict)
    h, w = 90, 120
    frames = [f for f, _ in zip(iter(synth.FrameStream(h, w, seed=3).next, None), range(4))]
    runs = []
    for estimate in (False, True):
        core = DEVAInferenceCore(net, synth.base_config(mem_every=2))
        outs = [core.step(frames[0], synth.box_mask(h, w, 2), [1, 2]), core.step(frames[1])]
        if estimate:
            seen = []
            inner = core._segment
            core._segment = lambda *a, **k: seen.append(inner(*a, **k)) or seen[-1]
            forward = estimate_forward_mask(core, frames[2])
            core._segment = inner
            assert len(seen) == 1 and core.curr_ti == 1
            _, pad = pad_divide_by(frames[2], 16)
            assert forward.dtype == torch.int64 and tuple(forward.shape) == (h, w)
            assert torch.equal(forward, unpad(torch.argmax(seen[0], dim=0), pad))
            assert set(forward.unique().tolist()) <= {0, 1, 2} and (forward > 0).any()
        outs += [core.step(frames[2]), core.step(frames[3])]
        work = core.memory.work_mem      # (the arenas' live rows: the capacity beyond them is uninitialised)
        usage = [t[:work.size(b)].clone() for b in work.buckets for t in work.usage_arenas(b)]
        runs.append((outs, usage))
    for a, b in zip(runs[0][0], runs[1][0]):
        assert torch.equal(a, b)
    assert len(runs[0][1]) == len(runs[1][1]) > 0
    for a, b in zip(runs[0][1], runs[1][1]):
        assert torch.equal(a, b)
