"""The filter and the best-mask choice from low-resolution logits (csrc/lowres/lowres.hip, `deva.hip.lowres`,
`ProposalFilter.add_lowres`) on the device against the numpy statement of rules L1-L6 (tests/lowres_case.py) and the CPU
contract of the proposal filter (tests/emu_proposals.py).  Every comparison with the statement is exact: fp32 values by
their bit patterns (every NaN counts as one pattern: which NaN an invalid operation gives is the processor's choice, not
the rules'), bytes, `chosen`, tables and keep order.  With DEVA_TEST_DRYRUN=1 the same code runs on the CPU contracts.

A small model_size keeps the shapes tiny: low 16 x 16, M = 64, input 36 x 64 takes the tile path at 33 x 70 and 65 x 129
(ragged bands in both directions: 33 = 2 * 16 + 1 rows, widths that are no multiple of 16) and the point path at 5 x 9 and
1 x 9 (ratio above 7)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import emu_lowres as EL
import emu_proposals as EP
import lowres_case as LC
import proposal_case as PC
from deva.hip import DevaHipError, check, lib, lowres
from deva.inference.proposals import ProposalFilter
from gpu_util import dev, to_dev

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DRYRUN = os.environ.get('DEVA_TEST_DRYRUN') == '1'

LOW, M, INPUT = (16, 16), 64, (36, 64)
SIZES = [(33, 70), (65, 129), (5, 9), (1, 9), (1, 1)]
TILE_SIZES, POINT_SIZES = SIZES[:2], SIZES[2:4]
REAL = [((256, 256), 1024, (576, 1024), (1080, 1920)), ((256, 256), 1024, (576, 1024), (480, 854))]


@pytest.fixture(autouse=True)
def _emulated_when_dry(monkeypatch):
    if DRYRUN:
        EP.install(monkeypatch)
        EL.install(monkeypatch)


def bits(x):
    """the bit patterns of fp32 values, every NaN as one pattern"""
    x = np.ascontiguousarray(x.cpu().numpy() if isinstance(x, torch.Tensor) else x, dtype=np.float32)
    return np.where(np.isnan(x), np.int32(0x7FC00000), x.view(np.int32))


def same(found, want):
    """planes, tables and keep order, bit for bit"""
    assert found.index.tolist() == want.index.tolist()
    assert np.array_equal(bits(found.iou_preds), bits(want.iou_preds)) and np.array_equal(bits(found.stability), bits(want.stability))
    assert found.boxes.tolist() == want.boxes.tolist()
    assert tuple(found.masks.shape) == tuple(want.masks.shape) and torch.equal(found.masks.cpu(), want.masks)


def statement_frame(size, batches, capacity=256, m=M, input_size=INPUT, **over):
    """the CPU contract of the full-resolution filter on the statement's planes; batches of (kind, planes, iou) with kind
    'low' (low-resolution logits) or 'full' (frame-sized ones)"""
    p = PC.params(**over)
    nms = p.pop('box_nms_thresh')
    state = EP.proposal_state(size[0], size[1], capacity, 'cpu')
    EP.proposal_begin(state)
    for kind, x, iou in batches:
        planes = torch.from_numpy(LC.upsample(x, m, input_size, size)).view(-1, *size) if kind == 'low' else torch.from_numpy(x)
        EP.proposal_batch(state, planes, torch.from_numpy(iou), **p)
    return state, nms


def filtered(flt, batches, m=M, input_size=INPUT):
    for kind, x, iou in batches:
        if kind == 'low':
            flt.add_lowres(to_dev(torch.from_numpy(x)), to_dev(torch.from_numpy(iou)), input_size, model_size=m)
        else:
            flt.add(to_dev(torch.from_numpy(x)), to_dev(torch.from_numpy(iou)))
    return flt.finish()


def frame(seed, n=24):
    """a frame of three batches: n planes with NaN and +-inf planes among them, a batch without a live plane, an empty one"""
    iou = LC.iou_preds(seed, n)
    iou[:4] = 0.99                                                     # the special planes are live
    return [('low', LC.logits(seed, n, LOW), iou),
            ('low', LC.logits(seed + 1, 5, LOW), np.full(5, 0.5, dtype=np.float32)),
            ('low', np.zeros((0,) + LOW, dtype=np.float32), np.zeros(0, dtype=np.float32))]


# ------------------------------------------------------------------------------------------ L3 materialised
@pytest.mark.parametrize('size', SIZES)
def test_upsample_is_the_statement_bit_for_bit(size):
    low = LC.logits(3, 7, LOW)
    want = LC.upsample(low, M, INPUT, size)
    assert np.isnan(want[1]).all() and np.isfinite(want[0]).all()
    assert size[0] < 33 or (np.isnan(want[2]).any() and np.isinf(want[2]).any() and np.isinf(want[3]).any())   # 0 * inf among them
    got = lowres.upsample_logits(to_dev(torch.from_numpy(low)), INPUT, size, model_size=M)
    assert got.dtype == torch.float32 and tuple(got.shape) == (7,) + size
    assert np.array_equal(bits(got), bits(want))
    n = 7 * size[0] * size[1]
    for off in (1, 3):                                                 # planes 4 and 12 bytes off a 16-byte boundary
        out = to_dev(torch.full((n + 4,), -7.0))
        view = out[off:off + n].view(7, *size)
        assert lowres.upsample_logits(to_dev(torch.from_numpy(low)), INPUT, size, model_size=M, out=view) is view
        assert np.array_equal(bits(view), bits(want))
        assert bool((out[:off] == -7.0).all()) and bool((out[off + n:] == -7.0).all())
    empty = lowres.upsample_logits(to_dev(torch.zeros((0,) + LOW)), INPUT, size, model_size=M)
    assert tuple(empty.shape) == (0,) + size


def test_the_plans_paths():
    assert all(lowres.plan(LOW, INPUT, s, model_size=M).path == lowres.PATH_TILE for s in TILE_SIZES)
    assert all(lowres.plan(LOW, INPUT, s, model_size=M).path == lowres.PATH_POINT for s in POINT_SIZES)
    assert all(lowres.plan(c[0], c[2], c[3], model_size=c[1]).path == lowres.PATH_TILE for c in REAL)


def _boundary():
    """the two output heights (width 70) between which the plan changes its path, read from the plan"""
    paths = {oh: lowres.plan(LOW, INPUT, (oh, 70), model_size=M).path for oh in range(1, 34)}
    flips = [oh for oh in range(1, 33) if paths[oh] != paths[oh + 1]]
    assert flips, paths
    return flips[-1], flips[-1] + 1


def test_each_side_of_the_path_boundary():
    below, above = _boundary()
    assert {lowres.plan(LOW, INPUT, (oh, 70), model_size=M).path for oh in (below, above)} == {lowres.PATH_TILE, lowres.PATH_POINT}
    low = LC.logits(5, 6, LOW)
    for oh in (below, above):
        size = (oh, 70)
        got = lowres.upsample_logits(to_dev(torch.from_numpy(low)), INPUT, size, model_size=M)
        assert np.array_equal(bits(got), bits(LC.upsample(low, M, INPUT, size)))
        batches = frame(7, 12)
        state, nms = statement_frame(size, batches, stability=0.7)
        same(filtered(ProposalFilter(*size, capacity=256, stability_score_thresh=0.7), batches), EP.proposal_finish(state, nms))


# ------------------------------------------------------------------------------------------ L6
@pytest.mark.parametrize('per_box', [1, 3, 16])
@pytest.mark.parametrize('size', [(33, 70), (5, 9)])
def test_select_bytes_and_choices(size, per_box):
    b = 9
    low = LC.logits(11, b * per_box, LOW).reshape(b, per_box, *LOW)
    scores = np.random.default_rng(4).uniform(0, 1, size=(b, per_box)).astype(np.float32)
    if per_box > 1:
        scores[1, 1] = np.nan                                          # the first NaN wins
        scores[2, :] = 0.5                                             # all tied: the first
        scores[3, -1] = scores[3].max()                                # a tie with an earlier maximum
        scores[4, 0], scores[4, 1] = -0.0, 0.0
        scores[4, 2:] = -1.0
    want, picks = LC.select(low, scores, M, INPUT, size)
    assert per_box == 1 or (picks[1] == 1 and picks[2] == 0 and picks[4] == 0 and len(set(picks.tolist())) > 1)
    low_d, scores_d = to_dev(torch.from_numpy(low)), to_dev(torch.from_numpy(scores))
    planes, chosen = lowres.select_masks(low_d, scores_d, INPUT, size, model_size=M)
    assert planes.dtype == torch.uint8 and chosen.dtype == torch.int32
    assert chosen.cpu().tolist() == picks.tolist() and np.array_equal(planes.cpu().numpy(), want)
    n = b * size[0] * size[1]
    for off in (1, 7, 15):                                             # `out` slices at byte offsets 1, 7 and 15
        buf = to_dev(torch.full((16 + n + 16,), 0xA5, dtype=torch.uint8))
        base = (-buf.data_ptr()) % 16 if not DRYRUN else 0
        view = buf[base + off:base + off + n].view(b, *size)
        lowres.select_masks(low_d, scores_d, INPUT, size, model_size=M, out=view)
        host = buf.cpu().numpy()
        assert np.array_equal(host[base + off:base + off + n].reshape(b, *size), want)
        assert (host[:base + off] == 0xA5).all() and (host[base + off + n:] == 0xA5).all()
    for t in (1.5, -2.0):
        got, _ = lowres.select_masks(low_d, scores_d, INPUT, size, model_size=M, threshold=t)
        assert np.array_equal(got.cpu().numpy(), LC.select(low, scores, M, INPUT, size, threshold=t)[0])


def test_select_without_scores_is_a_plain_threshold():
    low = LC.logits(13, 5, LOW).reshape(5, 1, *LOW)
    for size in ((65, 129), (1, 9)):
        planes, chosen = lowres.select_masks(to_dev(torch.from_numpy(low)), None, INPUT, size, model_size=M)
        assert chosen.cpu().tolist() == [0] * 5
        assert np.array_equal(planes.cpu().numpy(), (LC.upsample(low[:, 0], M, INPUT, size) > 0).astype(np.uint8))
    planes, chosen = lowres.select_masks(to_dev(torch.zeros((0, 3) + LOW)), to_dev(torch.zeros((0, 3))), INPUT, (5, 9), model_size=M)
    assert tuple(planes.shape) == (0, 5, 9) and chosen.numel() == 0


# ------------------------------------------------------------------------------------------ L5
@pytest.mark.parametrize('stability', [0.95, 0.7, 0.0])
@pytest.mark.parametrize('size', SIZES)
def test_frames_equal_the_filter_on_the_statements_planes(size, stability):
    """three batches per frame (planes with NaN and +-inf, a batch without a live plane, B = 0); the same filter takes the
    frame twice; stability 0.0 switches that drop off"""
    batches = frame(21)
    state, nms = statement_frame(size, batches, stability=stability)
    want = EP.proposal_finish(state, nms)
    if size[0] >= 33:                                                  # the case has what it is about
        assert (stability == 0.95 or (len(state.rows) > 2 and want.masks.shape[0] > 0)) and (stability == 0.0 or state.account['dropped_by_stability'] > 2)
    assert state.account['dropped_by_iou'] >= 5
    flt = ProposalFilter(*size, capacity=256, stability_score_thresh=stability)
    same(filtered(flt, batches), want)
    same(filtered(flt, batches), want)


def test_thresholds_at_or_below_zero_switch_the_drops_off():
    size = (33, 70)
    batches = frame(23, 10)
    state, nms = statement_frame(size, batches, stability=-1.0, pred_iou_thresh=0.0)
    want = EP.proposal_finish(state, nms)
    assert state.passed == 15 and 'dropped_by_iou' not in state.account                 # NaN predictions and NaN planes included
    flt = ProposalFilter(*size, capacity=256, stability_score_thresh=-1.0, pred_iou_thresh=0.0)
    same(filtered(flt, batches), want)


def test_only_live_planes_are_evaluated():
    size = (33, 70)
    low, iou = LC.logits(31, 16, LOW, specials=False), LC.iou_preds(31, 16)
    dead = ~(iou > np.float32(0.88))
    assert 3 <= int(dead.sum()) < 16
    state, nms = statement_frame(size, [('low', low, iou)], stability=0.7)
    want = EP.proposal_finish(state, nms)
    flt = ProposalFilter(*size, capacity=64, stability_score_thresh=0.7)
    for fill in (np.nan, np.inf, 3.0):
        other = low.copy()
        other[dead] = fill
        same(filtered(flt, [('low', other, iou)]), want)


def test_more_planes_than_one_decide_launch():
    """1100 planes of 9 x 7 from low 8 x 8, M = 32 in one `add_lowres`: cut into launches of 1024 planes behind the same
    device-side count; 63 bytes a plane, so every arena slot is misaligned"""
    size, low_size, m, input_size = (9, 7), (8, 8), 32, (32, 25)
    low = LC.logits(41, 1100, low_size, specials=False)
    iou = np.tile(LC.iou_preds(41, 50), 22)
    batches = [('low', low, iou)]
    state, nms = statement_frame(size, batches, capacity=1100, m=m, input_size=input_size, stability=0.5)
    want = EP.proposal_finish(state, nms)
    assert state.passed > 200 and max(want.index.tolist()) > 150
    flt = ProposalFilter(*size, capacity=1100, stability_score_thresh=0.5)
    same(filtered(flt, batches, m=m, input_size=input_size), want)


def test_a_mixed_frame_of_add_and_add_lowres():
    size = (33, 70)
    full = PC.batch(size[0], size[1], 12, 5, 0.8)
    batches = [frame(51, 10)[0], ('full', full[0].numpy(), full[1].numpy()), frame(52, 9)[0]]
    state, nms = statement_frame(size, batches, stability=0.8)
    want = EP.proposal_finish(state, nms)
    assert want.masks.shape[0] >= 2 and state.passed > 6
    same(filtered(ProposalFilter(*size, capacity=64, stability_score_thresh=0.8), batches), want)


def test_overflow_is_counted_and_stays_inside_the_arena():
    size = (33, 70)
    batches = frame(21)
    state, _ = statement_frame(size, batches, stability=0.0)
    assert state.passed > 4
    n = 4 * size[0] * size[1]
    buf = to_dev(torch.full((16 + 3 + n + 16,), 0xA5, dtype=torch.uint8))
    flt = ProposalFilter(*size, capacity=4, stability_score_thresh=0.0, arena=buf[19:19 + n])
    with pytest.raises(DevaHipError, match=rf'\b{state.passed} masks passed'):
        filtered(flt, batches)
    host = buf.cpu()
    assert bool((host[:19] == 0xA5).all()) and bool((host[19 + n:] == 0xA5).all())
    few = [('low', batches[0][1][:6], batches[0][2][:6])]
    state, nms = statement_frame(size, few, capacity=4, stability=0.95)
    same(filtered(ProposalFilter(*size, capacity=4, arena=buf[19:19 + n]), few), EP.proposal_finish(state, nms))


# ------------------------------------------------------------------------------------------ fused == unfused, byte for byte
def _poisoned(nbytes, offset, guard=256):
    buf = torch.full((guard + offset + nbytes + guard,), 0xA5, dtype=torch.uint8)
    return to_dev(buf), guard + offset


def _raw_frame(size, batches, capacity, shift, fused, **over):
    """begin and the batches by hand, with the arena (`shift` bytes off a 16-byte boundary) and the scratch inside poisoned
    buffers -> (arena bytes, scratch bytes) on the host after the last batch; the guard bands must come back untouched.
    fused: deva_lowres_proposal_batch; otherwise deva_lowres_upsample, then deva_proposal_batch on its planes."""
    p = PC.params(**over)
    L, LL = lib(), lowres.lib()
    h, w = size
    nbytes = L.deva_proposal_scratch(capacity)
    sizes = dict(arena=capacity * h * w, scratch=nbytes)
    bufs = {k: _poisoned(v, shift if k == 'arena' else 0) for k, v in sizes.items()}
    ptr = {k: b.data_ptr() + at for k, (b, at) in bufs.items()}
    assert ptr['scratch'] % 16 == 0 and ptr['arena'] % 16 == shift
    check(L.deva_proposal_begin(capacity, ptr['scratch'], nbytes, None), 'deva_proposal_begin')
    geo = lowres.Geometry(LOW[0], LOW[1], M, INPUT[0], INPUT[1], h, w, 0)
    keep_alive = []
    for _, low, iou in batches:
        low, iou = to_dev(torch.from_numpy(low)), to_dev(torch.from_numpy(iou))
        b = low.shape[0]
        args = (p['pred_iou_thresh'], p['stability_score_thresh'], p['stability_score_offset'], p['mask_threshold'], ptr['arena'],
                capacity, ptr['scratch'], nbytes, None)
        if fused:
            lowres.check(LL.deva_lowres_proposal_batch(low.data_ptr() if b else None, iou.data_ptr() if b else None, b, ctypes.byref(geo),
                                                       *args), 'deva_lowres_proposal_batch')
        else:
            planes = torch.empty((b, h, w), dtype=torch.float32, device=low.device)
            lowres.check(LL.deva_lowres_upsample(low.data_ptr() if b else None, b, ctypes.byref(geo), planes.data_ptr() if b else None, None),
                         'deva_lowres_upsample')
            check(L.deva_proposal_batch(planes.data_ptr() if b else None, iou.data_ptr() if b else None, b, h, w, *args), 'deva_proposal_batch')
            keep_alive.append(planes)
        keep_alive.append((low, iou))
    torch.cuda.synchronize()
    out = {}
    for k, (b, a) in bufs.items():
        host = b.cpu()
        assert bool((host[:a] == 0xA5).all()) and bool((host[a + sizes[k]:] == 0xA5).all()), k
        out[k] = host[a:a + sizes[k]]
    return out['arena'], out['scratch']


@pytest.mark.parametrize('size,shift,capacity', [((33, 70), 0, 32), ((33, 70), 7, 32), ((65, 129), 15, 32), ((5, 9), 1, 32), ((1, 9), 3, 32),
                                                 ((1, 1), 0, 32), ((33, 70), 5, 3)])
def test_arena_table_and_count_are_byte_identical_to_the_unfused_route(size, shift, capacity):
    """the arena and the whole scratch (records, slots, count, table; what neither route touches stays poison) after
    deva_lowres_proposal_batch equal what deva_proposal_batch leaves on deva_lowres_upsample's planes; capacity 3 overflows"""
    if DRYRUN:
        pytest.skip('raw pointers: needs the library')
    batches = frame(61, 20)
    fused = _raw_frame(size, batches, capacity, shift, True, stability=0.7)
    unfused = _raw_frame(size, batches, capacity, shift, False, stability=0.7)
    assert torch.equal(fused[0], unfused[0]) and torch.equal(fused[1], unfused[1])
    count = int(fused[1][36864:36868].view(torch.int32)[0])              # proposal_plan.h: off_count behind the records and the slots
    state, _ = statement_frame(size, batches, capacity=capacity, stability=0.7)
    assert count == state.passed and (count > capacity) == (capacity == 3)
    stored = min(count, capacity)
    assert torch.equal(fused[0][:stored * size[0] * size[1]].view(stored, *size), state.arena[:stored])
    assert bool((fused[0][stored * size[0] * size[1]:] == 0xA5).all())


# ------------------------------------------------------------------------------------------ the two real geometries
@pytest.fixture(scope='module')
def real_cases():
    """low 256 x 256, M = 1024 to 1080 x 1920 and 480 x 854, 4 planes each: the statement's planes, computed once"""
    out = {}
    for low_size, m, input_size, size in REAL:
        low = LC.logits(71, 4, low_size)
        low[1] = LC.smooth_logits(72, 1, low_size)[0]                   # (planes 0 and 1 are finite: the comparison with ATen takes them)
        out[size] = (low, m, input_size, LC.upsample(low, m, input_size, size))
    return out


@pytest.mark.parametrize('size', [c[3] for c in REAL])
def test_real_geometries(real_cases, size):
    low, m, input_size, want = real_cases[size]
    iou = np.array([0.95, 0.9, 0.99, 0.93], dtype=np.float32)
    low_d = to_dev(torch.from_numpy(low))
    got = lowres.upsample_logits(low_d, input_size, size, model_size=m)
    assert np.array_equal(bits(got), bits(want))
    p = PC.params(stability=0.5)
    nms = p.pop('box_nms_thresh')
    state = EP.proposal_state(size[0], size[1], 8, 'cpu')
    EP.proposal_begin(state)
    EP.proposal_batch(state, torch.from_numpy(want), torch.from_numpy(iou), **p)
    flt = ProposalFilter(*size, capacity=8, stability_score_thresh=0.5)
    flt.add_lowres(low_d, to_dev(torch.from_numpy(iou)), input_size, model_size=m)
    same(flt.finish(), EP.proposal_finish(state, nms))
    planes, _ = lowres.select_masks(low_d[None], to_dev(torch.from_numpy(iou[None])), input_size, size, model_size=m)
    assert np.array_equal(planes[0].cpu().numpy(), (want[2] > 0).astype(np.uint8))


@pytest.mark.parametrize('size', [c[3] for c in REAL])
def test_against_atens_chain_on_the_device(real_cases, size):
    """values within 4 x the bound measured on the CPU (tests/lowres_case.py), bytes equal outside it"""
    low, m, input_size, _ = real_cases[size]
    low_d = to_dev(torch.from_numpy(low[:2]))                           # the two finite planes
    got = lowres.upsample_logits(low_d, input_size, size, model_size=m)
    aten = LC.aten_chain(low_d, m, input_size, size)
    bound = LC.ATEN_FACTOR * LC.ATEN_BOUND
    worst = float((got - aten).abs().max())
    near = (aten.abs() <= bound)
    print(f'{size}: worst |device - ATen on the device| = {worst:.3e} (bound {bound:.3e}), within the bound of 0: {float(near.float().mean()):.2e}')
    planes, _ = lowres.select_masks(low_d[:, None], None, input_size, size, model_size=m)
    assert float(near.float().mean()) <= LC.ATEN_EXCUSED_MAX
    assert bool(((planes > 0) == (aten > 0))[~near].all())
    assert worst <= bound, worst
