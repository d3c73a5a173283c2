"""The run-length encoder (csrc/mask_runs/mask_runs.hip, `deva.hip.mask_runs`) on the device against the numpy statement of
its rules (tests/runs_case.py) for exact equality -- integers, so there is no tolerance -- with every output inside a
sentinel-filled buffer, and the interface on top of it: strings, the pending form, chunks, the round trip through
`rle.decode`, `ops.mask_rle` on disjoint planes, and a recorded run played back through `RecordedProcessor`.  With
DEVA_TEST_DRYRUN=1 the same code runs on the CPU contract (tests/emu_runs.py)."""
import os

import numpy as np
import pytest
import torch

import emu_detections as ED
import emu_frame_result as EF
import emu_prompts as EM
import emu_proposals as EP
import emu_rle as EL
import emu_runs as ER
import emu_text as ET
import gpu_util
import prompt_case as PC
import rle_case as LC
import runs_case as RC
import text_case as TC
from deva.hip import mask_runs, ops, rle
from gpu_util import dev

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DRYRUN = os.environ.get('DEVA_TEST_DRYRUN') == '1'
SENTINEL = -0x5A5A5A5B          # in every int32 word of a guarded buffer
SENTINEL64 = (SENTINEL & 0xFFFFFFFF) << 32 | (SENTINEL & 0xFFFFFFFF)
PAD = 16
TORCH = {np.dtype(np.uint8): torch.uint8, np.dtype(np.float32): torch.float32, np.dtype(np.bool_): torch.bool}


@pytest.fixture(autouse=True)
def _emulated_when_dry(monkeypatch):
    if DRYRUN:
        EF.install(monkeypatch)
        ED.install(monkeypatch)
        EL.install(monkeypatch)
        ER.install(monkeypatch)
        EP.install(monkeypatch)
        EM.install(monkeypatch)
        ET.install(monkeypatch)
        monkeypatch.setattr(torch.Tensor, 'cuda', lambda self, *a, **k: self)


def on_device(planes, lead=0):
    """the planes on the device, their first element `lead` elements into a larger buffer"""
    planes = np.ascontiguousarray(planes)
    flat = torch.zeros(lead + planes.size + 64, dtype=TORCH[planes.dtype], device=dev())
    flat[lead:lead + planes.size] = torch.from_numpy(planes.reshape(-1)).to(dev())
    return flat[lead:lead + planes.size].view(*planes.shape)


def guard(count, dtype):
    """-> (the whole buffer, sentinel-filled; its middle `count` elements)"""
    whole = torch.full((count + 2 * PAD,), SENTINEL if dtype == torch.int32 else SENTINEL64 - (1 << 64), dtype=dtype, device=dev())
    return whole, whole[PAD:PAD + count]


def untouched(whole, count, what, written=None):
    """everything outside the middle `count` elements (and inside it from `written` on) still holds the sentinel"""
    host = whole.cpu()
    fill = host[0].item()
    written = count if written is None else written
    assert (host[:PAD] == fill).all() and (host[PAD + written:] == fill).all(), f'{what}: written outside its range'


def check_call(planes, threshold, what, lead=0, capacity=None, first=None):
    """count + write with every output guarded -> the statement's dict; `capacity`: of `bounds` (default: exact)"""
    want = RC.statement(planes, threshold, 0 if first is None else first)
    n = planes.shape[0]
    held = want['total'] - (first or 0)
    capacity = want['total'] if capacity is None else capacity
    n_all, n_out = guard(n, torch.int32)
    base_all, base = guard(n, torch.int64)
    total_all, total = guard(1, torch.int64)
    stats_all, stats = guard(5 * n, torch.int32)
    bounds_all, bounds = guard(want['total'] + 3, torch.int32)        # (three more than an exact capacity may use)
    first_dev = None if first is None else torch.tensor([first], dtype=torch.int64, device=dev())
    device_planes = on_device(planes, lead)
    counted = mask_runs.count(device_planes, threshold, stats=True, first=first_dev,
                              out={'n': n_out, 'base': base, 'total': total, 'stats': stats.view(n, 5)})
    assert counted.n is n_out and counted.total is total
    mask_runs.write(counted, bounds, capacity)
    assert np.array_equal(n_out.cpu().numpy(), want['n']), (what, 'n')
    assert np.array_equal(base.cpu().numpy(), want['base']), (what, 'base')
    assert int(total.cpu()[0]) == want['total'], (what, 'total', int(total.cpu()[0]), want['total'])
    assert np.array_equal(stats.view(n, 5).cpu().numpy(), want['stats']), (what, 'stats')
    lo, hi = first or 0, min(capacity, want['total'])
    got = bounds.cpu().numpy()
    assert np.array_equal(got[lo:hi], want['bounds'][:max(hi - lo, 0)]), (what, 'bounds', np.flatnonzero(got[lo:hi] != want['bounds'][:max(hi - lo, 0)])[:8])
    assert (got[:lo] == SENTINEL).all() and (got[max(hi, lo):] == SENTINEL).all(), f'{what}: bounds written outside [first, capacity)'
    for whole, count_, name in ((n_all, n, 'n'), (base_all, n, 'base'), (total_all, 1, 'total'), (stats_all, 5 * n, 'stats'),
                                (bounds_all, want['total'] + 3, 'bounds')):
        untouched(whole, count_, f'{what}: {name}')
    assert held == int(want['n'].sum())
    return want


def check_strings(planes, threshold, what, **kw):
    """`encode` in its three forms against the statement; the text also against the per-value loop for masks it can walk"""
    device_planes = on_device(planes)
    want = RC.records(planes, threshold, 'counts', stats=True)
    assert mask_runs.encode(device_planes, threshold=threshold, form='counts', stats=True, **kw) == want, what
    texts = mask_runs.encode(device_planes, threshold=threshold, **kw)
    raw = mask_runs.encode(device_planes, threshold=threshold, form='bytes', **kw)
    for k, (text, body, rec) in enumerate(zip(texts, raw, want)):
        assert set(text) == {'size', 'counts'} and text['size'] == rec['size'] == body['size']
        assert isinstance(text['counts'], str) and body['counts'] == text['counts'].encode('ascii')
        assert rle.parse_counts(text['counts']).tolist() == rec['counts'], (what, k)
        if len(rec['counts']) <= 50000:          # (the string encoder of the tests is a loop over counts)
            assert text['counts'] == EF.coco_string(rec['counts']), (what, k)


# ------------------------------------------------------------------------------------------ the table
@pytest.mark.parametrize('h,w', RC.GEOMETRIES, ids=[f'{h}x{w}' for h, w in RC.GEOMETRIES])
def test_rows_equal_the_numpy_statement(h, w):
    names, planes = RC.byte_stack(h, w)
    check_call(planes, None, f'{h}x{w} uint8')
    check_strings(planes, None, f'{h}x{w} uint8')
    for threshold in RC.THRESHOLDS:
        _, logits = RC.float_stack(h, w, threshold)
        check_call(logits, threshold, f'{h}x{w} float32 > {threshold}')
    check_strings(logits, RC.THRESHOLDS[-1], f'{h}x{w} float32')
    if h * w > 128 * 144:
        return
    check_call(planes != 0, None, f'{h}x{w} bool')
    # E7: the same planes one element into a larger buffer; rows and planes begin at other residues of 16 bytes
    check_call(planes, None, f'{h}x{w} uint8, one element in', lead=1)
    check_call(logits, RC.THRESHOLDS[-1], f'{h}x{w} float32, one element in', lead=1)
    check_call(planes, None, f'{h}x{w} uint8, 16 bytes in', lead=16)


def test_the_aligned_geometry_is_on_the_vector_path():
    """128 x 144: every row of an aligned buffer begins on a 16-byte boundary (144 and 4 * 144 are multiples of 16), so
    every piece inside a tile is a 16-byte load; one element in, none is"""
    h, w = 128, 144
    assert (h, w) in RC.GEOMETRIES and w % 16 == 0
    planes = on_device(RC.byte_stack(h, w)[1])
    assert DRYRUN or planes.data_ptr() % 16 == 0
    assert DRYRUN or on_device(RC.byte_stack(h, w)[1], lead=1).data_ptr() % 16 == 1


# ------------------------------------------------------------------------------------------ the scans
def test_the_per_mask_scan_takes_a_second_step():
    h, w = RC.SCAN_GEOMETRY
    rng = np.random.default_rng(5)
    planes = (rng.random((3, h, w)) < 0.5).astype(np.uint8)
    planes[1] = RC.checkerboard(h, w)[0]
    check_call(planes, None, f'{h}x{w}: two scan steps')


def test_the_cross_mask_scan_takes_a_second_step():
    h, w = RC.SCAN_MASKS_SIZE
    planes = RC.many_small(RC.SCAN_MASKS, h, w)
    want = check_call(planes, None, f'{RC.SCAN_MASKS} masks of {h}x{w}')
    assert (want['n'] == 0).sum() > 40 and want['base'][-1] > 10000
    check_call(planes[:RC.SCAN_MASKS - 1], None, 'one step exactly', first=12345)
    check_strings(planes, None, 'many masks')


def test_the_checkerboard_has_a_boundary_at_every_position():
    """H * W - 1 boundaries a mask (p = 0 holds a 0): every word of the scratch is full and every offset counts"""
    h, w = 130, 200
    planes = np.concatenate([RC.checkerboard(h, w), 1 - RC.checkerboard(h, w), RC.checkerboard(h, w)])
    want = check_call(planes, None, 'checkerboards')
    assert want['n'].tolist() == [h * w - 1, h * w, h * w - 1]
    assert want['bounds'][:h * w - 1].tolist() == list(range(1, h * w))


# ------------------------------------------------------------------------------------------ E5
def test_capacity_exact_one_short_and_none():
    h, w = 65, 129
    names, planes = RC.byte_stack(h, w)
    total = RC.statement(planes)['total']
    for capacity in (total, total - 1, total // 2, 0):
        check_call(planes, None, f'capacity {capacity} of {total}', capacity=capacity)
    check_call(planes, None, 'a first boundary given', first=777, capacity=total + 777)
    check_call(planes, None, 'a first boundary given, short', first=777, capacity=total)
    device_planes = on_device(planes)
    want = RC.records(planes, None, 'string', stats=True)
    for capacity in (total, total + 5):
        pending = mask_runs.encode(device_planes, stats=True, capacity=capacity)
        assert isinstance(pending, mask_runs.PendingRuns) and pending.finish() == want and pending.finish() is pending.finish()
    for capacity in (total - 1, 0):
        pending = mask_runs.encode(device_planes, capacity=capacity)
        with pytest.raises(mask_runs.DevaHipError, match=rf'{total} run boundaries, the capacity is {capacity}\b'):
            pending.finish()
    assert mask_runs.encode(device_planes[:0]) == [] and mask_runs.encode(device_planes[:0], capacity=4).finish() == []


# ------------------------------------------------------------------------------------------ chunks
def test_a_call_above_the_limit_is_walked_in_chunks():
    h, w = 33, 67
    names, planes = RC.byte_stack(h, w)
    per_mask = mask_runs.runs_scratch(1, (h, w))
    for kw in (dict(max_masks=3), dict(max_masks=1), dict(max_scratch=2 * per_mask + 5), dict(max_scratch=per_mask, max_masks=4)):
        top = mask_runs.runs_limits()
        parts = mask_runs.chunks(len(names), (h, w), kw.get('max_masks', top.max_masks), kw.get('max_scratch', top.max_scratch))
        assert len(parts) > 1, kw
        check_strings(planes, None, f'chunks {kw}', **kw)
        total = RC.statement(planes)['total']
        assert mask_runs.encode(on_device(planes), capacity=total, stats=True, **kw).finish() == RC.records(planes, None, 'string', stats=True)
    with pytest.raises(mask_runs.DevaHipError, match='above the limit of one call'):
        mask_runs.encode(on_device(planes), max_scratch=per_mask - 1)


# ------------------------------------------------------------------------------------------ round trips
def test_decode_of_encode_is_the_plane():
    h, w = 65, 129
    names, planes = RC.byte_stack(h, w)
    got = rle.decode(rle.encode(on_device(planes)), device=dev())
    assert np.array_equal(got.cpu().numpy(), (planes != 0).astype(np.uint8))
    _, logits = RC.float_stack(h, w, 0.0)
    got = rle.decode(rle.encode(on_device(logits), threshold=0.0, form='bytes'), (48, 95), dtype=torch.float32, device=dev())
    assert np.array_equal(got.cpu().numpy(), LC.nearest((planes != 0).astype(np.float32), 48, 95))


@pytest.mark.parametrize('dtype', [torch.int64, torch.int32, torch.int16], ids=['int64', 'int32', 'int16'])
def test_disjoint_planes_equal_mask_rle_of_their_index_plane(dtype):
    from deva.inference.frame_results import rle_strings
    h, w = 65, 129
    labels, ids = RC.disjoint(h, w)
    held = set(np.unique(labels).tolist())
    assert ids[-1] not in held and len(held & set(ids)) >= 3
    index = np.zeros((h, w), dtype=np.int16)
    for c, i in enumerate(ids, start=1):
        index[labels == i] = c
    n, bounds = ops.mask_rle(torch.from_numpy(index).to(dev()), len(ids) + 1)
    want = [{'size': [h, w], 'counts': t} for t in rle_strings(n.cpu().numpy(), bounds.cpu().numpy(), h * w)[1:]]
    planes = np.stack([labels == i for i in ids])
    assert rle.encode(on_device(planes)) == want
    assert rle.encode_labels(torch.from_numpy(labels).to(dev()).to(dtype), ids) == want
    assert want[-1]['counts'] == EF.coco_string([h * w])                    # the id that no pixel holds
    assert rle.encode_labels(torch.from_numpy(labels).to(dev()).to(dtype), ids[::-1], form='counts') == RC.records(planes[::-1], None, 'counts')
    assert rle.encode_labels(torch.from_numpy(labels).to(dev()).to(dtype), []) == []


# ------------------------------------------------------------------------------------------ record, then play back
def _seen(core, into):
    real = core.incorporate_detection

    def wrapped(image, mask, segments_info, **kw):
        into.append((mask.cpu().clone(), [(o.id, list(o.category_ids), list(o.scores)) for o in segments_info], kw))
        return real(image, mask, segments_info, **kw)
    core.incorporate_detection = wrapped
    return core


def _play(processor, frames, names):
    produced = []
    for ti, (image_np, name) in enumerate(zip(frames, names)):
        produced += processor.process_frame(image_np, ti, name)
    return produced + processor.flush()


def _same_run(first, second, first_seen, second_seen):
    assert len(first_seen) == len(second_seen) >= 3
    for (mask, infos, kw), (mask2, infos2, kw2) in zip(first_seen, second_seen):
        assert mask.dtype == mask2.dtype == torch.int64 and torch.equal(mask, mask2)
        assert infos == infos2 and kw == kw2                                  # ids, category ids and scores, exactly
    assert [name for name, _ in first] == [name for name, _ in second]
    for (_, prob), (_, prob2) in zip(first, second):
        assert torch.equal(prob.cpu(), prob2.cpu())


@pytest.mark.parametrize('setting', ['online', 'semionline'])
def test_a_recorded_text_run_plays_back(setting, recipe_state_dict, tmp_path):
    from deva.inference.automatic import RecordedProcessor
    from deva.inference.detections import CocoResults, DetectionRecorder
    from deva.inference.inference_core import DEVAInferenceCore
    from deva.inference.with_text import TextPromptedProcessor
    from deva.model.network import DEVA
    net = DEVA(gpu_util.net_config(**TC.loop_config(setting)))
    net.load_weights(recipe_state_dict[0])
    net = net.to(dev()).eval()
    make_core = lambda: DEVAInferenceCore(net, gpu_util.net_config(**TC.loop_config(setting)))   # noqa: E731
    frames, rects = TC.clip()
    names = [f'{t:05d}.jpg' for t in range(len(frames))]
    recorder, first_seen, second_seen = DetectionRecorder(str(tmp_path / 'detections.json')), [], []
    np.random.seed(11)
    first = _play(TextPromptedProcessor(_seen(make_core(), first_seen), TC.FakeDetector(frames, rects, TC.HALVES), TC.FakeBoxSegmenter(),
                                        recorder=recorder), frames, names)
    detected = 3 if setting == 'online' else 9                               # every buffered frame's detection, not the vote
    assert len({a['image_id'] for a in recorder.annotations}) == detected and any('category_id' in a for a in recorder.annotations)
    results = CocoResults(recorder.write())
    np.random.seed(11)
    second = _play(RecordedProcessor(_seen(make_core(), second_seen), results), frames, names)
    _same_run(first, second, first_seen, second_seen)


@pytest.mark.parametrize('setting', ['online', 'semionline'])
def test_a_recorded_automatic_run_plays_back(setting, recipe_state_dict, tmp_path):
    from deva.inference.automatic import AutomaticProcessor, RecordedProcessor
    from deva.inference.detections import CocoResults, DetectionRecorder
    from deva.inference.inference_core import DEVAInferenceCore
    from deva.model.network import DEVA
    net = DEVA(gpu_util.net_config(**PC.loop_config(setting)))
    net.load_weights(recipe_state_dict[0])
    net = net.to(dev()).eval()
    make_core = lambda: DEVAInferenceCore(net, gpu_util.net_config(**PC.loop_config(setting)))   # noqa: E731
    frames, rects = PC.clip()
    names = [f'{t:05d}.jpg' for t in range(len(frames))]
    recorder, first_seen, second_seen = DetectionRecorder(), [], []
    np.random.seed(11)
    first = _play(AutomaticProcessor(_seen(make_core(), first_seen), PC.FakeSegmenter(frames, rects), capacity=512, recorder=recorder),
                  frames, names)
    assert recorder.annotations and not any('category_id' in a for a in recorder.annotations)
    results = CocoResults(recorder.write(str(tmp_path / 'detections.json')))
    np.random.seed(11)
    second = _play(RecordedProcessor(_seen(make_core(), second_seen), results, incorporate_keywords={'incremental': True}), frames, names)
    _same_run(first, second, first_seen, second_seen)
    assert all(kw == {'incremental': True} for _, _, kw in second_seen)
