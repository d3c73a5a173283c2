"""`ops.detection_assemble` (csrc/detections.hip) on the device against its CPU contract (tests/emu_detections.py) and,
where the golden file has the case, against what the reference's own auto_segment / segment_with_text returned
(tests/golden/detection_assembly.npz).  With DEVA_TEST_DRYRUN=1 the same code runs on the CPU contract.

Dyadic cases (equal sizes, x2, x2/3: every resized value is a multiple of 1/16 and every area is exact in fp32 in any
order) must agree bit for bit, records included.  For sizes that are not dyadic the kernel's fixed-order fp32 sums and
torch's differ in the last bits of an area, so a decision may differ where two scores nearly tie: those pixels are found
from an fp64 restatement of the INPUTS alone (never from the kernel's output), must be fewer than 1e-3 of the frame, and
everything else must be equal."""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import detection_case as DC
import emu_detections as ED
import gpu_util
from deva.hip import check, lib, ops
from gpu_util import to_dev
from workload import synth

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DRYRUN = os.environ.get('DEVA_TEST_DRYRUN') == '1'
OPS_POLICY = {'suppress': 'suppress_small', 'prefer': 'prefer_small', 'text': 'text'}


@pytest.fixture(autouse=True)
def _emulated_when_dry(monkeypatch):
    if DRYRUN:
        ED.install(monkeypatch)
        monkeypatch.setattr(torch.Tensor, 'cuda', lambda self, *a, **k: self)


@pytest.fixture(scope='module')
def golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, 'detection_assembly.npz')))


@functools.lru_cache(maxsize=None)
def _contract(size_in, size_out, n, policy, threshold, consistent=False, seed=0):
    """the CPU contract's (mask, records) of a case, computed once and shared (read-only)"""
    masks = DC.masks(*size_in, extra=max(0, n - 18), seed=seed)[:n]
    return ED.detection_assemble(masks, size_out, OPS_POLICY[policy], scores=DC.scores(n), consistent_ids=consistent,
                                 overlap_threshold=0.8 if threshold is None else threshold)


def _device(masks, size_out, n, policy, threshold, consistent=False):
    mask, rec = ops.detection_assemble(to_dev(masks), size_out, OPS_POLICY[policy], scores=to_dev(DC.scores(n)),
                                       consistent_ids=consistent, overlap_threshold=0.8 if threshold is None else threshold)
    return mask.cpu(), rec.cpu()


# ------------------------------------------------------------------------------------------ bit-identical group
DYADIC = [((24, 36), (24, 36), 18), ((23, 37), (23, 37), 18), ((270, 480), (270, 480), 40), ((24, 36), (48, 72), 18),
          ((30, 45), (20, 30), 18), ((24, 36), (24, 36), 0), ((24, 36), (24, 36), 1)]


@pytest.mark.parametrize('policy,threshold', DC.POLICIES)
@pytest.mark.parametrize('size_in,size_out,n', DYADIC)
def test_dyadic_cases_are_bit_identical(size_in, size_out, n, policy, threshold, golden):
    masks = DC.case_masks(size_in, n)
    want_mask, want_rec = _contract(size_in, size_out, n, policy, threshold)
    mask, rec = _device(masks, size_out, n, policy, threshold)
    assert mask.dtype == torch.int64 and rec.dtype == torch.int32 and tuple(rec.shape) == (n, 8)
    assert torch.equal(mask, want_mask)
    assert torch.equal(rec, want_rec), (rec - want_rec).abs().amax(0).tolist()
    key = DC.golden_key(policy, threshold, size_in, size_out, n)
    if key + '/mask' in golden:     # (every case but the text policy at the two larger equal sizes: see detection_case.py)
        from deva.inference import detections as D
        dev_masks = to_dev(masks)
        if policy == 'text':
            got, info = D.assemble_with_text(dev_masks, DC.confidences(n), DC.class_ids(n), size_out)
        else:
            got, info = D.assemble_automatic(dev_masks, to_dev(DC.scores(n)), size_out, suppress_small_objects=policy == 'suppress',
                                             overlap_threshold=0.8 if threshold is None else threshold)
        assert np.array_equal(got.cpu().numpy(), golden[key + '/mask'].astype(np.int64))
        assert [o.id for o in info] == golden[key + '/ids'].tolist()
        assert [float(o.scores[0]) for o in info] == golden[key + '/scores'].tolist()
        assert [-1 if o.category_ids[0] is None else int(o.category_ids[0]) for o in info] == golden[key + '/categories'].tolist()
    else:
        assert policy == 'text' and (size_in, n) in DC.MORE


@pytest.mark.parametrize('policy,threshold', DC.POLICIES[1:])
@pytest.mark.parametrize('size_in,size_out', [((24, 36), (24, 36)), ((23, 37), (23, 37)), ((24, 36), (48, 72))])
def test_inputs_as_bool_uint8_and_fp32(size_in, size_out, policy, threshold):
    masks = DC.case_masks(size_in, 18)
    want = _contract(size_in, size_out, 18, policy, threshold)
    for m in (masks.to(torch.uint8), masks.float()):
        mask, rec = _device(m, size_out, 18, policy, threshold)
        assert torch.equal(mask, want[0]) and torch.equal(rec, want[1])


def test_consistent_ids():
    want = _contract((24, 36), (48, 72), 18, 'prefer', None, True)
    mask, rec = _device(DC.case_masks((24, 36), 18), (48, 72), 18, 'prefer', None, True)
    assert torch.equal(mask, want[0]) and torch.equal(rec, want[1])
    assert sorted(set(mask.unique().tolist()) - {0}) == sorted(i for i in rec[:, 0].tolist() if i)


@pytest.mark.parametrize('policy', ['suppress_small', 'prefer_small', 'text'])
def test_more_masks_than_a_workgroup_has_threads(policy):
    """1025 masks at 8 x 12 (one table for every count: the LDS counters hold 4096 masks, there is no second path; this
    is the size at which the table kernel's threads take more than one mask each and the prep kernel wraps around):
    random small rectangles, every fifth mask empty, every seventh a copy of the one before"""
    rng = np.random.default_rng(7)
    n, h, w = 1025, 8, 12
    masks = torch.zeros(n, h, w, dtype=torch.bool)
    for k in range(n):
        if k % 5 == 4:
            continue
        if k % 7 == 6:
            masks[k] = masks[k - 1]
            continue
        y0, x0 = int(rng.integers(0, h)), int(rng.integers(0, w))
        masks[k, y0:y0 + int(rng.integers(1, 4)), x0:x0 + int(rng.integers(1, 5))] = True
    for size in (None, (16, 24)):
        want = ED.detection_assemble(masks, size, policy, scores=DC.scores(n))
        mask, rec = ops.detection_assemble(to_dev(masks), size, policy, scores=to_dev(DC.scores(n)))
        assert torch.equal(mask.cpu(), want[0]) and torch.equal(rec.cpu(), want[1])


# ------------------------------------------------------------------------------------------ sizes that are not dyadic
def _excused(masks, size_out, policy):
    """bool [OH,OW]: the pixels whose decision may depend on the order of an fp32 sum, from an fp64 restatement of the
    inputs: (a) the best and the second-best score are distinct and closer than 1e-5 (s1 + s2) + 1e-6 (a1 + a2) -- a
    fixed-order fp32 sum of at most 2^24 terms in [0, 1] errs by at most about 24 * 2^-24 = 1.4e-6 relative on either
    side, the sampling roundings are a few ulp of 1 and the two products add an ulp each; (b) some |P_k - 0.5| < 1e-6.
    Exact ties (identical planes) are not excused: both sides must give the first index."""
    p = F.interpolate(masks.double().unsqueeze(0), tuple(size_out), mode='bilinear', align_corners=False)[0]
    near_half = ((p - 0.5).abs() < 1e-6).any(0)
    if policy == 'text':
        return near_half
    area = p.flatten(1).sum(1)
    a = area if policy == 'suppress' else area.max() * 2 - area
    a = torch.cat([torch.zeros(1, dtype=torch.float64), a])
    s = torch.cat([torch.full((1, *p.shape[1:]), 0.1, dtype=torch.float64), p * a[1:].view(-1, 1, 1)])
    top, at = s.topk(2, dim=0)
    gap = top[0] - top[1]
    bound = 1e-5 * (top[0] + top[1]) + 1e-6 * (a[at[0]] + a[at[1]])
    return near_half | ((gap > 0) & (gap <= bound))


@pytest.mark.parametrize('policy,threshold', [('suppress', 0.8), ('prefer', None), ('text', None)])
@pytest.mark.parametrize('size_in,size_out', [((30, 45), (48, 72)), ((29, 53), (41, 75))])
def test_sizes_that_are_not_dyadic(size_in, size_out, policy, threshold):
    n = 30
    masks = DC.masks(*size_in, extra=n - 18, seed=3)
    excused = _excused(masks, size_out, policy)
    count = int(excused.sum())
    print(f'{size_in} -> {size_out} {policy}: {count} of {excused.numel()} pixels excused')
    assert count <= 1e-3 * excused.numel()
    want_mask, want_rec = _contract(size_in, size_out, n, policy, threshold, False, 3)
    mask, rec = _device(masks, size_out, n, policy, threshold)
    differ = mask != want_mask
    print(f'  {int(differ.sum())} pixels differ, records differ by at most {int((rec - want_rec)[:, 1:4].abs().max())}')
    if count == 0:
        assert torch.equal(mask, want_mask) and torch.equal(rec, want_rec)
    else:   # a decision inside the set moves at most that many pixels between two masks
        assert torch.equal(rec[:, 4:], want_rec[:, 4:]) and int((rec - want_rec)[:, 1:4].abs().max()) <= count
        if torch.equal(rec[:, 0], want_rec[:, 0]):
            assert not bool((differ & ~excused).any())


# ------------------------------------------------------------------------------------------ determinism and bounds
def _poisoned(nbytes, offset, guard=256):
    buf = torch.full((guard + offset + nbytes + guard,), 0xA5, dtype=torch.uint8)
    return to_dev(buf), guard + offset


@pytest.mark.parametrize('policy', [0, 1, 2])
@pytest.mark.parametrize('size_in,size_out,shift', [((24, 36), (24, 36), 0), ((24, 36), (24, 36), 8), ((23, 37), (23, 37), 8),
                                                   ((29, 53), (41, 75), 0), ((270, 480), (270, 480), 0)])
def test_two_runs_are_bit_identical_and_stay_inside_their_buffers(size_in, size_out, shift, policy):
    """raw calls with the output mask, the records and the scratch inside poisoned buffers (the mask once 16-byte
    aligned for the packed stores and once only 8-byte aligned): the guard bands come back untouched, and a second
    call leaves the same bytes in the mask and the records"""
    if DRYRUN:
        pytest.skip('raw pointers: needs the library')
    n = 24
    masks = to_dev(DC.masks(*size_in, extra=n - 18, seed=5).to(torch.uint8))
    scores = to_dev(DC.scores(n))
    (h, w), (oh, ow) = size_in, size_out
    nbytes = lib().deva_detection_scratch(n, h, w, oh, ow)
    sizes = dict(out=oh * ow * 8, rec=n * 8 * 4, scratch=nbytes)
    runs = []
    for _ in range(2):
        bufs = {k: _poisoned(v, shift if k == 'out' else 0) for k, v in sizes.items()}
        ptr = {k: b.data_ptr() + at for k, (b, at) in bufs.items()}
        assert ptr['scratch'] % 16 == 0 and ptr['out'] % 16 == shift
        check(lib().deva_detection_assemble(masks.data_ptr(), n, h, w, oh, ow, policy, 0.8, 0, scores.data_ptr(), ptr['scratch'],
                                            nbytes, ptr['out'], ptr['rec'], None), 'deva_detection_assemble')
        torch.cuda.synchronize()
        for k, (b, at) in bufs.items():
            host = b.cpu()
            assert bool((host[:at] == 0xA5).all()) and bool((host[at + sizes[k]:] == 0xA5).all()), k
        runs.append({k: bufs[k][0].cpu()[bufs[k][1]:bufs[k][1] + sizes[k]] for k in ('out', 'rec')})
    assert torch.equal(runs[0]['out'], runs[1]['out']) and torch.equal(runs[0]['rec'], runs[1]['rec'])
    want = ED.detection_assemble(masks.cpu(), size_out, ops.DETECTION_POLICIES[policy], scores=scores.cpu())
    if size_in == size_out:
        assert torch.equal(runs[0]['out'].view(torch.int64).view(oh, ow), want[0])
        assert torch.equal(runs[0]['rec'].view(torch.int32).view(n, 8), want[1])


# ------------------------------------------------------------------------------------------ through the core
def _network(recipe_state_dict):
    from deva.model.network import DEVA
    cfg = gpu_util.net_config(mem_every=2, max_missed_detection_count=1, max_num_objects=-1)
    net = DEVA(cfg)
    net.load_weights(recipe_state_dict[0])
    return net.to(gpu_util.dev()).eval(), cfg


@pytest.mark.parametrize('policy', ['suppress', 'text'])
def test_clip_with_raw_mask_stacks(policy, recipe_state_dict, monkeypatch):
    """a 96 x 128 clip whose detections arrive as raw mask stacks on every second frame: once assembled on the device,
    once by the CPU contract (which tests/test_detections_cpu.py holds to the reference's answers) and copied over, into
    two identical cores.  The segments and every frame's probabilities must be bit-identical."""
    from deva.inference import detections as D
    from deva.inference.inference_core import DEVAInferenceCore
    net, cfg = _network(recipe_state_dict)
    dev = gpu_util.dev()
    h, w, n = 96, 128, 9
    frames = [f for f, _ in zip(iter(synth.FrameStream(h, w, seed=2).next, None), range(4))]
    stacks = {0: DC.masks(h, w)[:n], 2: DC.masks(h, w)[:n].roll(3, dims=2)}

    def assemble(masks):
        if policy == 'text':
            return D.assemble_with_text(masks, DC.confidences(n), DC.class_ids(n))
        return D.assemble_automatic(masks, DC.scores(n), suppress_small_objects=True, overlap_threshold=0.8)

    runs = []
    for on_device in (True, False):
        core = DEVAInferenceCore(net, cfg)
        outs, infos = [], []
        for t, frame in enumerate(frames):
            if t in stacks:
                if on_device:
                    mask, info = assemble(to_dev(stacks[t]))
                else:
                    with monkeypatch.context() as m:
                        ED.install(m)
                        mask, info = assemble(stacks[t])
                    mask = to_dev(mask)
                infos.append([(o.id, o.category_ids, o.scores) for o in info])
                outs.append(core.incorporate_detection(to_dev(frame), mask, info))
            else:
                outs.append(core.step(to_dev(frame)))
        runs.append(([o.cpu() for o in outs], infos))
    assert runs[0][1] == runs[1][1] and len(runs[0][1][0]) >= 6
    for a, b in zip(runs[0][0], runs[1][0]):
        assert a.shape[0] > 6 and torch.equal(a, b)


def test_forward_mask_leaves_no_trace(recipe_state_dict):
    """`estimate_forward_mask` on the HIP core, then `step`: bit-identical probabilities to the run without the call"""
    from deva.inference.detections import estimate_forward_mask
    from deva.inference.inference_core import DEVAInferenceCore
    net, cfg = _network(recipe_state_dict)
    h, w = 90, 120
    frames = [to_dev(f) for f, _ in zip(iter(synth.FrameStream(h, w, seed=3).next, None), range(4))]
    runs = []
    for estimate in (False, True):
        core = DEVAInferenceCore(net, cfg)
        outs = [core.step(frames[0], to_dev(synth.box_mask(h, w, 2)), [1, 2]), core.step(frames[1])]
        if estimate:
            forward = estimate_forward_mask(core, frames[2])
            assert forward.dtype == torch.int64 and tuple(forward.shape) == (h, w) and core.curr_ti == 1
            assert set(forward.unique().tolist()) <= {0, 1, 2} and bool((forward > 0).any())
        outs += [core.step(frames[2]), core.step(frames[3])]
        runs.append([o.cpu() for o in outs])
    for a, b in zip(*runs):
        assert torch.equal(a, b)
