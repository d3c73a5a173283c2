"""The run-length decoder (csrc/rle/rle_decode.hip, `deva.hip.rle`) on the device against the numpy statement of its rules
(tests/rle_case.py) for exact equality -- zeros and ones, so there is no tolerance -- and the interface on top of it:
the project's own encoder and saver read back, detections from a results list, the float planes of the vote.  With
DEVA_TEST_DRYRUN=1 the same code runs on the CPU contract."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import emu_detections as ED
import emu_frame_result as EF
import emu_rle as EL
import result_case as ResultCase
import rle_case as LC
from deva.hip import ops, rle
from gpu_util import dev

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DRYRUN = os.environ.get('DEVA_TEST_DRYRUN') == '1'
SENTINEL = 0xA5
NP = {torch.uint8: np.uint8, torch.float32: np.float32}


@pytest.fixture(autouse=True)
def _emulated_when_dry(monkeypatch):
    if DRYRUN:
        EF.install(monkeypatch)
        ED.install(monkeypatch)
        EL.install(monkeypatch)


def same(got, want, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    assert np.array_equal(got, want), (what, np.argwhere(got != want)[:8].tolist(), got[got != want][:8], want[got != want][:8])
    return got


def guarded(n, oh, ow, dtype, lead):
    """-> (flat uint8 buffer filled with the sentinel, the [n,oh,ow] view that begins `lead` bytes into it)"""
    nbytes = n * oh * ow * torch.empty((), dtype=dtype).element_size()
    flat = torch.full((lead + nbytes + 256,), SENTINEL, dtype=torch.uint8, device=dev())
    return flat, flat[lead:lead + nbytes].view(dtype).view(n, oh, ow)


def decode_guarded(rles, size, dtype, want, lead, what, **kw):
    """decode into the middle of a sentinel buffer: every element inside is the statement's, no byte outside is touched"""
    n, oh, ow = want.shape
    flat, out = guarded(n, oh, ow, dtype, lead)
    assert rle.decode(rles, size, dtype=dtype, out=out, **kw) is out
    same(out, want, what)
    host = flat.cpu().numpy()
    inside = want.size * want.itemsize
    assert (host[:lead] == SENTINEL).all() and (host[lead + inside:] == SENTINEL).all(), f'{what}: a byte outside the output was written'


# ------------------------------------------------------------------------------------------ the table
@pytest.mark.parametrize('h,w', LC.GEOMETRIES, ids=[f'{h}x{w}' for h, w in LC.GEOMETRIES])
def test_rows_equal_the_numpy_statement(h, w):
    names, all_counts = LC.row(h, w)
    rles = LC.as_rles(all_counts, h, w)
    want = LC.decoded(all_counts, h, w)
    # 251 and 16 bytes in: planes and rows that begin at every residue of 16; the float planes 4 and 12 bytes off
    for dtype, leads in ((torch.uint8, (251, 16)), (torch.float32, (260, 12))):
        for lead in leads:
            decode_guarded(rles, None, dtype, want.astype(NP[dtype]), lead, f'{h}x{w} {dtype} {lead} bytes in')
    got = rle.decode(rles, device=dev())               # and the tensor the call allocates itself
    assert got.dtype == torch.uint8 and got.is_contiguous() and tuple(got.shape) == (len(names), h, w)
    same(got, want, 'allocated by the call')


@pytest.mark.parametrize('source,size', LC.RESIZES, ids=[f'{s[0]}x{s[1]}->{o[0]}x{o[1]}' for s, o in LC.RESIZES])
def test_resize_equals_interpolate_nearest_of_the_statement(source, size):
    h, w = source
    names, all_counts = LC.row(h, w)
    rles = LC.as_rles(all_counts, h, w)
    planes = torch.from_numpy(LC.planes(all_counts, h, w))
    for dtype, lead in ((torch.uint8, 253), (torch.float32, 264)):
        want = F.interpolate(planes.to(dtype)[None], size=size, mode='nearest')[0].contiguous().numpy()      # on the CPU
        assert np.array_equal(want, LC.decoded(all_counts, h, w, size, NP[dtype]))
        decode_guarded(rles, size, dtype, want, lead, f'{source}->{size} {dtype}')


def test_one_full_frame():
    """1080 x 1920, 8 masks, straight and to 480 x 854: 510 tiles a mask, the grid-stride loop, two masks of two million
    runs and one of four"""
    h, w, size = 1080, 1920, (480, 854)
    yy, _ = np.mgrid[:h, :w]
    all_counts = [LC.counts_of(LC.blobs(h, w, 1)), LC.counts_of(LC.blobs(h, w, 2)), [1] * (h * w), [h] * w, LC.counts_of(yy & 1),
                  LC.mid_column_run(h, w), LC.zero_counts(h, w), LC.counts_of(LC.corners(h, w))]
    rles = [{'size': [h, w], 'counts': np.asarray(c)} for c in all_counts]
    planes = LC.planes(all_counts, h, w)
    same(rle.decode(rles, device=dev()), planes, 'straight')
    want = F.interpolate(torch.from_numpy(planes)[None], size=size, mode='nearest')[0].numpy()
    same(rle.decode(rles, size, device=dev()), want, 'resized')
    same(rle.decode(rles[:2], size, dtype=torch.float32, device=dev()), want[:2].astype(np.float32), 'resized, float')


# ------------------------------------------------------------------------------------------ chunks
def test_a_call_above_the_limit_is_walked_in_chunks():
    h, w = 33, 67
    names, all_counts = LC.row(h, w)
    rles = LC.as_rles(all_counts, h, w)
    want = LC.decoded(all_counts, h, w, (48, 95))
    most = max(len(c) for c in all_counts) + 3
    for kw in (dict(max_masks=3), dict(max_masks=1), dict(max_words=most), dict(max_words=2 * most, max_masks=4)):
        parsed = rle.parse_checked(rles)
        top = rle.rle_limits()
        parts = rle.chunks(parsed.per_mask, kw.get('max_masks', top.max_masks), kw.get('max_words', top.max_words))
        assert len(parts) > 1, kw
        decode_guarded(rles, (48, 95), torch.uint8, want, 249, f'chunks {kw}', **kw)
    with pytest.raises(rle.DevaHipError, match='runs are above the limit of one call'):
        rle.decode(rles, device=dev(), max_words=most - 1)


# ------------------------------------------------------------------------------------------ the project's own encoder
def test_round_trip_through_mask_rle_and_rle_strings():
    from deva.inference.frame_results import rle_strings
    h, w = 33, 67
    names, all_counts = LC.row(h, w)
    index = np.zeros((h, w), dtype=np.int16)
    for c, plane in enumerate(LC.planes(all_counts, h, w)[2:], start=1):      # painted over one another, from the corners on
        index[(plane != 0) & ((np.arange(h)[:, None] * 7 + np.arange(w)[None, :] * 3 + c) % 4 != 0)] = c
    channels = len(all_counts) - 2 + 1 + 1                                     # and a last channel that is absent
    assert len(np.unique(index)) == channels - 1
    n, bounds = ops.mask_rle(torch.from_numpy(index).to(dev()), channels)
    texts = rle_strings(n.cpu().numpy(), bounds.cpu().numpy(), h * w)
    assert texts[0] is None
    got = rle.decode([{'size': [h, w], 'counts': t} for t in texts[1:]], device=dev())
    same(got, np.stack([index == c for c in range(1, channels)]).astype(np.uint8), 'index == c')
    assert not got[-1].any()


def test_read_video_json_gives_the_savers_frames_back(tmp_path):
    """the clip of tests/result_case.py (object 3 vanishes on frame 2) through `FrameResultSaver(dataset='burst')`, then
    `read_video_json`: per frame and segment exactly `labels == id`, and the records' areas and boxes are
    `FrameResult.segments`'"""
    from deva.inference.frame_results import FrameResultSaver, read_video_json
    from deva.inference.object_info import ObjectInfo
    from deva.inference.object_manager import ObjectManager
    long_id, objects, _ = ResultCase.BURST
    om = ResultCase.object_manager(ObjectManager, ObjectInfo, long_id, objects)
    saver = FrameResultSaver(str(tmp_path), 'clip', dataset='burst', object_manager=om, palette=ResultCase.palette())
    results = []
    for t, prob in enumerate(ResultCase.probabilities()):
        prob = prob.to(dev())
        saver.save_mask(prob, ResultCase.NAMES[t])
        results.append(om.frame_result(prob, labels=True))
    saver.end()
    assert saver.error is None
    frames = list(read_video_json(saver.video_json, device=dev()))
    assert [f[0] for f in frames] == ResultCase.NAMES
    segments_seen = 0
    for (name, ids, scores, planes), result, entry in zip(frames, results, saver.video_json['segmentations']):
        live = [s for s in result.segments if s['area'] > 0]
        assert ids == [s['id'] for s in live] and scores == [s['score'] for s in live]
        labels = result.labels.cpu().numpy()
        same(planes, np.stack([labels == i for i in ids]).astype(np.uint8), name)
        rec = rle.records([s['rle'] for s in entry['segmentations']])
        assert rec.area.tolist() == [s['area'] for s in live]
        assert rec.bbox.tolist() == [[int(v) for v in s['bbox']] for s in live]
        segments_seen += len(ids)
    assert segments_seen == 3 * ResultCase.FRAMES - 1                           # object 3 is absent once
    # the float form at another size, from the JSON as a file would hold it
    import json
    again = list(read_video_json(json.loads(json.dumps(saver.video_json)), (60, 80), dtype=torch.float32, device=dev()))
    want = F.interpolate(frames[0][3].cpu()[None].float(), size=(60, 80), mode='nearest')[0].numpy()
    same(again[0][3], want, 'float planes at 60 x 80')


# ------------------------------------------------------------------------------------------ detections
def _frame_of_twelve(h, w):
    """12 overlapping seeded masks with scores and categories, one of them empty, as a results list of one image"""
    rng = np.random.default_rng(12)
    yy, xx = np.mgrid[:h, :w]
    anns, all_counts = [], []
    for k in range(12):
        cy, cx, ry, rx = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(h / 10, h / 4), rng.uniform(w / 10, w / 4)
        mask = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1
        if k == 5:
            mask[:] = False
        counts = LC.counts_of(mask)
        all_counts.append(counts)
        anns.append({'image_id': 4, 'category_id': int(rng.integers(1, 5)), 'score': float(np.float32(rng.uniform(0.2, 1.0))),
                     'segmentation': {'size': [h, w], 'counts': EF.coco_string(counts)}})
    return anns, all_counts


def _infos(objects):
    return [(o.id, o.category_ids, o.scores) for o in objects]


@pytest.mark.parametrize('size', [None, (48, 95)], ids=['straight', 'resized'])
def test_rle_detections_equal_the_assembly_of_the_statements_planes(size):
    from deva.inference import detections as D
    h, w = 65, 129
    anns, all_counts = _frame_of_twelve(h, w)
    planes = torch.from_numpy(LC.decoded(all_counts, h, w, size)).to(dev())
    scores = [a['score'] for a in anns]
    assert planes.flatten(1).any(1).sum() == 11 and (planes.sum(0) > 1).any()            # they overlap, and one is empty
    want_mask, want_objects = D.assemble_with_text(planes, scores, [a['category_id'] for a in anns])
    mask, objects = D.rle_detections(anns, size, policy='text')
    assert mask.dtype == torch.int64 and torch.equal(mask, want_mask) and _infos(objects) == _infos(want_objects) and len(objects) > 3
    for policy, suppress in (('large', True), ('small', False)):
        want_mask, want_objects = D.assemble_automatic(planes, scores, suppress_small_objects=suppress, overlap_threshold=0.7)
        mask, objects = D.rle_detections(anns, size, policy=policy, overlap_threshold=0.7)
        assert torch.equal(mask, want_mask) and _infos(objects) == _infos(want_objects) and len(objects) > 3, (policy, len(objects))
    # a score threshold leaves annotations out before anything is decoded; the results file serves the frame
    keep = [k for k, s in enumerate(scores) if s >= 0.6]
    want_mask, want_objects = D.assemble_with_text(planes[keep], [scores[k] for k in keep], [anns[k]['category_id'] for k in keep])
    results = D.CocoResults(anns + [dict(anns[0], image_id=9)])
    mask, objects = results.detections(4, size, score_threshold=0.6)
    assert 0 < len(keep) < 12 and torch.equal(mask, want_mask) and _infos(objects) == _infos(want_objects)
    mask, objects = D.rle_detections(anns, (5, 6), score_threshold=2.0, device=dev())
    assert tuple(mask.shape) == (5, 6) and mask.dtype == torch.int64 and not mask.any() and objects == []
    with pytest.raises(ValueError, match='no `size`'):
        D.rle_detections([], None)


def test_rle_masks_are_the_float_planes_of_the_vote():
    from deva.inference.consensus_associated import rle_masks
    h, w = 33, 67
    names, all_counts = LC.row(h, w)
    got = rle_masks(LC.as_rles(all_counts, h, w), (66, 134), device=dev())
    assert got.dtype == torch.float32
    same(got, LC.decoded(all_counts, h, w, (66, 134), np.float32), 'rle_masks')
