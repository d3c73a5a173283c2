"""The proposal filter (csrc/proposals.hip, `deva.inference.proposals.ProposalFilter`, `ops.box_nms`) on the device
against its CPU contract (tests/emu_proposals.py) on the recipe of tests/proposal_case.py.  Counts are integers and the
two divisions are single correctly rounded fp32 divisions on both sides, so every comparison is exact: planes, tables
and keep order, no tolerance and no excluded case.  With DEVA_TEST_DRYRUN=1 the same code runs on the CPU contract."""
import os

import numpy as np
import pytest
import torch

import emu_detections as ED
import emu_proposals as EP
import gpu_util
import owner_mode
import proposal_case as PC
from deva.hip import DevaHipError, check, lib, ops
from deva.inference.proposals import ProposalFilter
from gpu_util import to_dev
from workload import synth

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DRYRUN = os.environ.get('DEVA_TEST_DRYRUN') == '1'


@pytest.fixture(autouse=True)
def _emulated_when_dry(monkeypatch):
    if DRYRUN:
        EP.install(monkeypatch)
        ED.install(monkeypatch)


def bits(t):
    return t.cpu().contiguous().view(torch.int32).tolist()


def same(found, want):
    """planes, tables and keep order, bit for bit"""
    assert found.masks.dtype == torch.uint8 and found.boxes.dtype == torch.int32
    assert found.index.tolist() == want.index.tolist()
    assert bits(found.iou_preds) == bits(want.iou_preds) and bits(found.stability) == bits(want.stability)
    assert found.boxes.tolist() == want.boxes.tolist()
    assert tuple(found.masks.shape) == tuple(want.masks.shape) and torch.equal(found.masks.cpu(), want.masks)


def emulated(h, w, batches, capacity=4096, **over):
    """the CPU contract's result for a list of (logits, iou_preds) batches on the host"""
    p = PC.params(**over)
    nms = p.pop('box_nms_thresh')
    state = EP.proposal_state(h, w, capacity, 'cpu')
    EP.proposal_begin(state)
    for logits, iou in batches:
        EP.proposal_batch(state, logits, iou, **p)
    return EP.proposal_finish(state, nms)


def filtered(flt, batches):
    for logits, iou in batches:
        flt.add(to_dev(logits), to_dev(iou))
    return flt.finish()


# ------------------------------------------------------------------------------------------ frames of the recipe
@pytest.mark.parametrize('b', PC.BATCHES)
@pytest.mark.parametrize('h,w,stability', [(29, 53, 0.95), (30, 45, 0.95), (64, 64, 0.95), (29, 53, 0.8)])
def test_frames_are_bit_identical(h, w, stability, b):
    """three batches per frame (B planes, a batch without a survivor, B = 0); 29 x 53: every plane after the first is
    4 bytes off a 16-byte boundary and the width is no multiple of 4; the same filter takes the frame twice"""
    PC.check_case(h, w, stability)
    want, account = PC.oracle(h, w, b, stability)
    flt = ProposalFilter(h, w, capacity=256, stability_score_thresh=stability)
    first = filtered(flt, PC.frame(h, w, b, stability))
    same(first, want)
    again = filtered(flt, PC.frame(h, w, b, stability))       # the arena and the scratch are reused
    same(again, want)
    assert want.masks.shape[0] == account['kept']


def test_a_batch_longer_than_one_decide_launch():
    """1030 planes of 8 x 12 in one `add`: cut into launches of 1024 masks behind the same device-side count"""
    rng = np.random.default_rng(5)
    h, w, b = 8, 12, 1030
    logits = torch.full((b, h, w), -1.0)
    for k in range(b):                                       # a random rectangle at 2, every fourth with a rim at 1/2
        y0, x0 = int(rng.integers(0, h - 1)), int(rng.integers(0, w - 1))
        y1, x1 = y0 + int(rng.integers(1, 5)), x0 + int(rng.integers(1, 6))
        if k % 4 == 3:
            logits[k, max(y0 - 1, 0):y1 + 1, max(x0 - 1, 0):x1 + 1] = 0.5
        logits[k, y0:y1, x0:x1] = 2.0
    iou = torch.from_numpy(rng.choice(np.array(PC.GRID, dtype=np.float32), b))
    iou[1024:] = 1.0                                         # the second launch stores some too
    want = emulated(h, w, [(logits, iou)], stability=0.5, box_nms_thresh=0.9)
    assert want.masks.shape[0] >= 50 and int(want.index.max()) > 500 and int((want.iou_preds == 1.0).sum()) >= 3
    same(filtered(ProposalFilter(h, w, capacity=1024, stability_score_thresh=0.5, box_nms_thresh=0.9), [(logits, iou)]), want)


# ------------------------------------------------------------------------------------------ bounds, poison, determinism
def _poisoned(nbytes, offset, guard=256):
    buf = torch.full((guard + offset + nbytes + guard,), 0xA5, dtype=torch.uint8)
    return to_dev(buf), guard + offset


def _raw_frame(h, w, capacity, batches, shift, **over):
    """begin / batch / finish / gather by hand with the arena, the scratch, the result table and the output inside
    poisoned buffers (the arena and the output `shift` bytes off a 16-byte boundary) -> (result table, output planes)
    on the host; the guard bands must come back untouched"""
    p = PC.params(**over)
    L = lib()
    nbytes = L.deva_proposal_scratch(capacity)
    sizes = dict(arena=capacity * h * w, scratch=nbytes, result=(4 + capacity * 8) * 4)
    bufs = {k: _poisoned(v, shift if k == 'arena' else 0) for k, v in sizes.items()}
    ptr = {k: b.data_ptr() + at for k, (b, at) in bufs.items()}
    assert ptr['scratch'] % 16 == 0 and ptr['arena'] % 16 == shift
    check(L.deva_proposal_begin(capacity, ptr['scratch'], nbytes, None), 'deva_proposal_begin')
    keep_alive = []
    for logits, iou in batches:
        logits, iou = to_dev(logits.contiguous()), to_dev(iou)
        keep_alive.append((logits, iou))
        check(L.deva_proposal_batch(logits.data_ptr(), iou.data_ptr(), logits.shape[0], h, w, p['pred_iou_thresh'],
                                    p['stability_score_thresh'], p['stability_score_offset'], p['mask_threshold'],
                                    ptr['arena'], capacity, ptr['scratch'], nbytes, None), 'deva_proposal_batch')
    check(L.deva_proposal_finish(capacity, p['box_nms_thresh'], ptr['scratch'], nbytes, ptr['result'], None),
          'deva_proposal_finish')
    torch.cuda.synchronize()
    table = bufs['result'][0].cpu()[bufs['result'][1]:][:sizes['result']].view(torch.int32)
    stored, passed, kept = table[:3].tolist()
    out_bytes = kept * h * w
    out, at = _poisoned(out_bytes, shift)
    if passed <= capacity:
        check(L.deva_proposal_gather(ptr['arena'], capacity, h, w, ptr['scratch'], nbytes, kept, out.data_ptr() + at, None),
              'deva_proposal_gather')
    torch.cuda.synchronize()
    for k, (b, a) in list(bufs.items()) + [('out', (out, at))]:
        host, size = b.cpu(), sizes.get(k, out_bytes)
        assert bool((host[:a] == 0xA5).all()) and bool((host[a + size:] == 0xA5).all()), k
    return table, out.cpu()[at:at + out_bytes].view(kept, h, w)


def _against(table, planes, want):
    kept = want.masks.shape[0]
    assert table[2] == kept and table[3] == 0 and table[0] == min(int(table[1]), len(table) // 8)
    rows = table[4:4 + kept * 8].view(kept, 8)
    assert rows[:, 0].tolist() == want.index.tolist() and rows[:, 3:7].tolist() == want.boxes.tolist()
    assert rows[:, 1].tolist() == bits(want.iou_preds) and rows[:, 2].tolist() == bits(want.stability)
    assert rows[:, 7].abs().sum() == 0 and torch.equal(planes, want.masks)


@pytest.mark.parametrize('h,w,shift', [(29, 53, 0), (29, 53, 7), (30, 45, 4), (64, 64, 0), (64, 64, 13)])
def test_poisoned_planes_guard_bands_and_a_repeated_call(h, w, shift):
    """a batch with planes full of +-inf and NaN among the recipe's; arena, scratch, result and output in guarded
    buffers, the byte planes at every alignment; a second run leaves the same bytes"""
    if DRYRUN:
        pytest.skip('raw pointers: needs the library')
    logits, iou = (t.clone() for t in PC.batch(h, w, 40, 11))
    inf, nan = float('inf'), float('nan')
    logits[2] = inf                                           # hi = lo = all: stability 1, the whole plane set
    logits[3] = -inf                                          # lo = 0: dropped
    logits[4] = nan                                           # compares false everywhere: lo = 0, dropped
    logits[6].view(-1)[::3] = nan                             # a ramp with holes
    logits[7].view(-1)[::5] = inf
    logits[8].view(-1)[1::2] = -inf
    iou[2:9] = torch.tensor([1.0, 1.0, 1.0, 0.95, 0.95, 0.9, 0.9])
    batches = [(logits[:17], iou[:17]), (logits[17:], iou[17:])]
    want = emulated(h, w, batches, stability=0.8)
    assert int((want.masks.flatten(1).sum(1) == h * w).sum()) == 1 and want.masks.shape[0] >= 4
    runs = [_raw_frame(h, w, 24, batches, shift, stability=0.8) for _ in range(2)]
    _against(*runs[0], want)
    assert torch.equal(runs[0][0][:4 + 8 * int(runs[0][0][2])], runs[1][0][:4 + 8 * int(runs[1][0][2])])
    assert torch.equal(runs[0][1], runs[1][1])


def test_overflow_stays_inside_the_arena_and_the_filter_recovers():
    """capacity 4, 9 passing masks: nothing beyond the arena is written, `finish` raises with the count, and the same
    object filters the next frame correctly"""
    h, w = 29, 53
    steps = torch.stack([PC.step_plane(h, w, 20, 20, (1 + 5 * (k % 5), 1 + 6 * (k // 5))) for k in range(9)])
    steps = torch.cat([steps[:5], PC.barren(h, w, 0)[0], steps[5:]])
    iou = torch.cat([torch.full((5,), 0.9), PC.barren(h, w, 0)[1], torch.full((4,), 0.95)])
    batches = [(steps[:7], iou[:7]), (steps[7:], iou[7:])]
    if not DRYRUN:
        table, _ = _raw_frame(h, w, 4, batches, 5)
        assert table[:3].tolist()[:2] == [4, 9]
    buf, at = _poisoned(4 * h * w, 3) if not DRYRUN else (torch.zeros(4 * h * w + 1000, dtype=torch.uint8), 0)
    flt = ProposalFilter(h, w, capacity=4, arena=buf[at:at + 4 * h * w])
    with pytest.raises(DevaHipError, match=r'\b9 masks passed'):
        filtered(flt, batches)
    if not DRYRUN:
        host = buf.cpu()
        assert bool((host[:at] == 0xA5).all()) and bool((host[at + 4 * h * w:] == 0xA5).all())
    flt.add(to_dev(steps[:1]), to_dev(iou[:1]))
    flt.reset()                                               # forgotten
    few = [(steps[:2], iou[:2]), (steps[9:11], iou[9:11])]
    same(filtered(flt, few), emulated(h, w, few, capacity=4))
    assert emulated(h, w, few, capacity=4).index.tolist() == [2, 3, 0, 1]


def test_only_live_masks_are_read():
    """the planes of masks that are not live are NaN, +-inf or other planes altogether: the result does not change"""
    h, w = 30, 45
    logits, iou = PC.batch(h, w, 64, 21, 0.8)
    dead = ~(iou > np.float32(0.88))
    assert int(dead.sum()) >= 10
    want = emulated(h, w, [(logits, iou)], stability=0.8)
    flt = ProposalFilter(h, w, capacity=64, stability_score_thresh=0.8)
    for fill in (float('nan'), float('inf'), 3.0):
        other = logits.clone()
        other[dead] = fill
        same(filtered(flt, [(other, iou)]), want)


# ------------------------------------------------------------------------------------------ NMS alone
@pytest.mark.parametrize('m', [1, 63, 64, 65, 130, 1000, 4096])
def test_box_nms_alone(m):
    """random integer boxes with many duplicates, zero-area boxes and blocks of equal scores against the numpy
    restatement of rule 5 (tests/emu_proposals.py:nms); twice: the same list"""
    rng = np.random.default_rng(m)
    side = 24 if m < 1000 else 160
    x0, y0 = rng.integers(0, side, m), rng.integers(0, side, m)
    boxes = np.stack([x0, y0, x0 + rng.integers(0, 12, m), y0 + rng.integers(0, 12, m)], 1).astype(np.int32)
    copies = rng.integers(0, m, m // 3)
    boxes[rng.integers(0, m, m // 3)] = boxes[copies]                       # duplicates
    boxes[rng.integers(0, m, m // 10), 2:] = 0                               # degenerate: x1 < x0 or a point at 0,0
    scores = rng.choice(np.array([0.5, 0.75, 0.9, 0.9, 1.0], dtype=np.float32), m)   # blocks of equal scores
    if m >= 63:
        scores[rng.integers(0, m, 3)] = np.nan
        scores[rng.integers(0, m, 3)] = -0.0
    for thresh in (0.7, 0.0):
        want = EP.nms(boxes, scores, thresh)
        got = [ops.box_nms(to_dev(torch.from_numpy(boxes)), to_dev(torch.from_numpy(scores)), thresh) for _ in range(2)]
        assert got[0].dtype == torch.int32 and got[0].tolist() == want and got[1].tolist() == want
        assert 0 < len(want) and (m < 63 or len(want) < m)
    assert ops.box_nms(to_dev(torch.zeros(0, 4, dtype=torch.int32)), to_dev(torch.zeros(0)), 0.7).tolist() == []


# ------------------------------------------------------------------------------------------ large frames
def test_a_1080p_frame_through_the_assembly():
    """1080 x 1920, two batches of 24, then assemble_automatic: against the emulation end to end"""
    from deva.inference import detections as D
    h, w = 1080, 1920
    batches = [PC.batch(h, w, 24, 31, 0.8), PC.batch(h, w, 24, 32, 0.8)]
    want = emulated(h, w, batches, capacity=64, stability=0.8)
    assert want.masks.shape[0] >= 4
    found = filtered(ProposalFilter(h, w, capacity=64, stability_score_thresh=0.8), batches)
    same(found, want)
    mask, info = D.assemble_automatic(found.masks, found.iou_preds, suppress_small_objects=True)
    want_mask, want_rec = ED.detection_assemble(want.masks, None, 'suppress_small', scores=want.iou_preds)
    assert torch.equal(mask.cpu(), want_mask)
    ids = sorted(i for i in want_rec[:, 0].tolist() if i)
    assert [o.id for o in info] == ids and len(ids) >= 3
    assert [float(o.scores[0]) for o in info] == [float(want.iou_preds[k]) for k in range(len(want_rec)) if want_rec[k, 0]]


def test_offsets_beyond_32_bits():
    """one batch of 70 planes at 2160 x 3840 (2.3 GB, filled on the device): plane 69 starts beyond 2^31 bytes.  Only
    planes 0, 33 and 69 are live; the oracle runs on those three alone"""
    if DRYRUN:
        pytest.skip('2.3 GB of logits: the device only')
    h, w, b = 2160, 3840, 70
    live = (0, 33, 69)
    centres, radii = [(700.5, 1000.0), (1500.0, 2900.5), (1100.0, 1900.0)], [400.0, 300.0, 650.0]
    three = PC.ramps(h, w, centres, radii, [16.0, 16.0, 8.0])
    three_iou = torch.tensor([0.9, 0.95, 0.9])
    want = emulated(h, w, [(three, three_iou)], capacity=4)
    assert want.index.tolist() == [1, 0, 2]
    logits = torch.full((b, h, w), float('nan'), device=gpu_util.dev())
    iou = torch.full((b,), 0.5)
    for k, plane, score in zip(live, three, three_iou):
        logits[k].copy_(plane)
        iou[k] = score
    flt = ProposalFilter(h, w, capacity=4)
    flt.add(logits, to_dev(iou))
    same(flt.finish(), want)


# ------------------------------------------------------------------------------------------ through the core
def _network(recipe_state_dict):
    from deva.model.network import DEVA
    cfg = gpu_util.net_config(mem_every=2, max_missed_detection_count=1, max_num_objects=-1)
    net = DEVA(cfg)
    net.load_weights(recipe_state_dict[0])
    return net.to(gpu_util.dev()).eval(), cfg


def test_clip_with_raw_logit_batches(recipe_state_dict, monkeypatch):
    """a 96 x 128 clip on the HIP core whose detections arrive as raw logit batches on every second frame: once
    ProposalFilter -> assemble_automatic -> incorporate_detection on the device, once with the filter emulated (and its
    result copied over) into an identical core.  Segments, object tables and every frame's probabilities are equal."""
    from deva.inference import detections as D
    from deva.inference.inference_core import DEVAInferenceCore
    net, cfg = _network(recipe_state_dict)
    h, w = 96, 128
    frames = [f for f, _ in zip(iter(synth.FrameStream(h, w, seed=2).next, None), range(4))]
    runs = []
    for on_device in (True, False):
        np.random.seed(7)                                     # (a colliding id is replaced by a random one)
        core = DEVAInferenceCore(net, cfg)
        flt = ProposalFilter(h, w, capacity=64, stability_score_thresh=0.8)
        outs, infos, tables = [], [], []
        for t, frame in enumerate(frames):
            if t % 2 == 0:
                batches = [PC.batch(h, w, 12, 40 + t, 0.8), PC.barren(h, w, t), PC.batch(h, w, 5, 50 + t, 0.8)]
                if on_device:
                    found = filtered(flt, batches)
                else:
                    found = emulated(h, w, batches, capacity=64, stability=0.8)
                mask, info = D.assemble_automatic(to_dev(found.masks), to_dev(found.iou_preds), suppress_small_objects=True)
                infos.append([(o.id, o.scores) for o in info])
                outs.append(core.incorporate_detection(to_dev(frame), mask, info))
            else:
                outs.append(core.step(to_dev(frame)))
            tables.append(owner_mode.table(core.object_manager))
        runs.append(([o.cpu() for o in outs], infos, tables))
    assert runs[0][1] == runs[1][1] and len(runs[0][1][0]) >= 2
    assert runs[0][2] == runs[1][2] and core.object_manager.num_obj >= 2
    for a, b in zip(runs[0][0], runs[1][0]):
        assert a.shape[0] >= 3 and torch.equal(a, b)
