"""The region kernels (csrc/regions/regions.hip, `deva.hip.regions`) on the device against the numpy statement of their rules
(tests/region_case.py): labels, cleaned planes and records for exact equality -- integers, so there is no tolerance -- and
the generator's `postprocess_small_regions` through `ProposalFilter(min_mask_region_area=...)` and `AutomaticProcessor`
against the three statements in a row: the proposal filter's, the regions', the NMS's.  With DEVA_TEST_DRYRUN=1 the same
code runs on the CPU contract."""
import os
import types

import numpy as np
import pytest
import torch

import emu_detections as ED
import emu_proposals as EP
import emu_regions as ER
import prompt_case as PromptCase
import proposal_case as PC
import region_case as RC
from deva.hip import ops, regions
from gpu_util import dev

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DRYRUN = os.environ.get('DEVA_TEST_DRYRUN') == '1'
T = regions.region_plan(8, 8, 1).tile      # the tile edge of the local stage, as the plan exports it (host only)


@pytest.fixture(autouse=True)
def _emulated_when_dry(monkeypatch):
    if DRYRUN:
        EP.install(monkeypatch)
        ED.install(monkeypatch)
        ER.install(monkeypatch)


def up(a):
    return torch.from_numpy(np.array(a)).to(dev())          # (a copy: the kernels work in place, and a host tensor shares memory)


def same(got, want, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    assert np.array_equal(got, want), (what, np.argwhere(got != want)[:8].tolist(), got[got != want][:8], want[got != want][:8])
    return got


# ------------------------------------------------------------------------------------------ geometry
# every row: all patterns, the diagonal pair across every tile corner in all four orientations, one plane per outcome
# (tests/test_regions_cpu.py asserts the outcomes on the statement).  29 x 53: 1537 bytes a plane, so every second plane
# starts at an odd byte.  T + 1 and 2 T + 3: a tile edge one pixel from the end, three tiles with a sliver.
GEOMETRY = [(1, 9, 'one row'), (9, 1, 'one column'), (2, 2, 'a single 2 x 2 neighbourhood'), (29, 53, 'inside one tile row, odd plane starts'),
            (T + 1, 2 * T + 3, 'tile edges both ways, a one-row sliver'), (2 * T + 3, T + 1, 'the same, upright'),
            (T, T, 'one tile exactly'), (T - 1, T - 1, 'one tile minus a row and a column')]


@pytest.mark.parametrize('h,w,what', GEOMETRY, ids=[f'{g[0]}x{g[1]}' for g in GEOMETRY])
def test_rows_equal_the_numpy_statement(h, w, what):
    assert T == 32          # the rows of tests/region_case.py (and the CPU test's coverage check) are built for this tile
    names, planes, min_area = RC.row(h, w, T)
    want_planes, want_records, want_labels, want_zero_labels = RC.expected(h, w, T)
    assert len(names) >= 5
    same(regions.label_components(up(planes)), want_labels, 'labels')
    same(regions.label_components(up(planes), of_zeros=True), want_zero_labels, 'labels of the zeros')
    got_planes, got_records = regions.remove_small_regions(up(planes), min_area)
    records = same(got_records, want_records, 'records')
    same(got_planes, want_planes, 'planes')
    if (h, w) != (2, 2):
        assert records[:, 1].any() and records[:, 2].any() and (records[:, 0] == 0).any()
    # min_area 1 removes nothing and changes nothing; above H * W every component is small
    for area in (1, h * w + 1):
        want = RC.clean(planes, area)
        got = regions.remove_small_regions(up(planes * 255), area)        # and 0 / 255 bytes are 0 / 1 afterwards (R1)
        same(got[0], want[0], f'planes at min_area {area}')
        recs = same(got[1], want[1], f'records at min_area {area}')
        if area == 1:
            assert not recs[:, :3].any() and np.array_equal(want[0], planes)
        else:
            assert recs[:, 0].all()


def test_a_full_frame_of_blobs():
    """480 x 854, three planes: the grid-stride loops of every stage (15 x 27 tiles), components far above 65 535 pixels"""
    planes = np.stack([RC.blobs(480, 854, seed) for seed in (1, 2, 3)])
    want_planes, want_records = RC.clean(planes, 100)
    want_labels = RC.label_planes(planes, of_zeros=True)
    assert np.bincount(want_labels.ravel())[1:].max() > 65535
    same(regions.label_components(up(planes), of_zeros=True), want_labels, 'labels')
    got = regions.remove_small_regions(up(planes), 100)
    records = same(got[1], want_records, 'records')
    same(got[0], want_planes, 'planes')
    assert (records[:, 1] > 0).all() and (records[:, 2] > 0).all() and (records[:, 3] > 65535).any()


def test_areas_above_65535():
    """a body of 67 599 pixels and beside it a block of 66 000 around a hole of 64 964: each stays at a min_area equal to its
    area and goes one above it (the counts are exact int32 sums, R7)"""
    plane = np.zeros((400, 700), dtype=np.uint8)         # (the background is larger still)
    plane[10:270, 10:270] = 1
    plane[269, 269] = 0                      # the body: 260 * 260 - 1
    plane[20:240, 280:580] = 1               # the block: 220 * 300 ...
    plane[21:239, 281:579] = 0               # ... hollowed: a ring of 1 036 around a hole of 218 * 298
    want = {area: RC.clean(plane, area) for area in (64964, 64965, 67599, 67600)}
    assert want[64964][1].tolist()[:4] == [1, 0, 1036, 67599]           # the hole stays, the ring around it is an island of 1 036
    assert want[64965][1].tolist()[:4] == [1, 64964, 0, 67599 + 66000]  # the hole fills, and the block is large enough
    assert want[67599][1].tolist()[:4] == [1, 64964, 66000, 67599]      # the body is not below its own area
    assert want[67600][1].tolist()[:4] == [1, 64964, 66000, 67599]      # everything is small: the largest stays
    for area, (want_plane, want_record) in want.items():
        got = regions.remove_small_regions(up(plane), area)
        same(got[1], want_record, f'record at {area}')
        same(got[0], want_plane, f'plane at {area}')


# ------------------------------------------------------------------------------------------ hygiene
@pytest.fixture(scope='module')
def five():
    names, planes, min_area = RC.row(29, 53, T)
    pick = [names.index(n) for n in ('blobs', 'only-filled', 'only-removed', 'keep-largest', 'both')]
    want = RC.expected(29, 53, T)
    return planes[pick], min_area, want[0][pick], want[1][pick]


def test_two_scratch_passes_equal_one(five):
    """K = 5 with a budget of two planes: three passes on the same scratch, the last one short"""
    planes, min_area, want_planes, want_records = five
    one = regions.region_scratch_bytes(29, 53)
    assert regions.region_plan(29, 53, 5, 2 * one + 7)[4:6] == (2, 3)
    for budget in (2 * one + 7, one, 5 * one):
        scratch = torch.zeros(budget, dtype=torch.uint8, device=dev())
        got = regions.remove_small_regions(up(planes), min_area, scratch=scratch)
        same(got[1], want_records, f'records with {budget} bytes')
        same(got[0], want_planes, f'planes with {budget} bytes')


def test_two_runs_sentinel_planes_and_exact_scratch(five):
    planes, min_area, want_planes, want_records = five
    k, h, w = planes.shape
    need = regions.region_scratch_bytes(h, w, k)
    scratch = torch.full((need + 256,), 0xA5, dtype=torch.uint8, device=dev())
    runs = []
    for _ in range(2):
        buf = torch.full((k + 2, h, w), 0xAB, dtype=torch.uint8, device=dev())        # a sentinel plane on either side
        buf[1:k + 1] = up(planes)
        records = torch.full((k + 2, 8), -7, dtype=torch.int32, device=dev())
        got = regions.remove_small_regions(buf[1:k + 1], min_area, scratch=scratch[:need], records=records[1:k + 1])
        assert got[0].data_ptr() == buf[1:].data_ptr() and got[1].data_ptr() == records[1:].data_ptr()      # in place
        same(buf[1:k + 1], want_planes, 'planes')
        runs.append(same(records[1:k + 1], want_records, 'records'))
        assert bool((buf[0] == 0xAB).all()) and bool((buf[k + 1] == 0xAB).all())
        assert bool((records[0] == -7).all()) and bool((records[k + 1] == -7).all())
    assert np.array_equal(runs[0], runs[1])
    assert bool((scratch[need:] == 0xA5).all())            # nothing is written past what the size function announces
    labels = torch.full((k + 2, h, w), -7, dtype=torch.int32, device=dev())
    out = regions.label_components(up(planes), out=labels[1:k + 1])
    assert out.data_ptr() == labels[1:].data_ptr()
    same(labels[1:k + 1], RC.label_planes(planes), 'labels')
    assert bool((labels[0] == -7).all()) and bool((labels[k + 1] == -7).all())
    # a single plane [H,W] gives a single record [8]
    got = regions.remove_small_regions(up(planes[4]), min_area)
    assert tuple(got[0].shape) == (h, w) and tuple(got[1].shape) == (8,)
    same(got[1], want_records[4], 'one record')
    same(regions.label_components(up(planes[4])), RC.labels(planes[4] != 0), 'labels of one plane')
    # no planes is no work
    got = regions.remove_small_regions(torch.zeros((0, h, w), dtype=torch.uint8, device=dev()), min_area)
    assert tuple(got[1].shape) == (0, 8)
    assert tuple(regions.label_components(torch.zeros((0, h, w), dtype=torch.uint8, device=dev())).shape) == (0, h, w)


def test_labels_of_the_zeros_are_the_labels_of_the_complement(five):
    planes = five[0]
    zeros = regions.label_components(up(planes), of_zeros=True).cpu()
    assert torch.equal(zeros, regions.label_components(up(1 - planes)).cpu())
    assert torch.equal(zeros, regions.label_components(up((planes == 0).astype(np.uint8) * 255)).cpu())        # any non-zero byte is mask
    assert bool(((zeros > 0) == torch.from_numpy(planes == 0)).all())


# ------------------------------------------------------------------------------------------ the pipeline
H, W = 37, 53


def _statement(batches, params, min_area, region_nms_thresh=None):
    """the proposal statement, then the region statement, then the NMS statement -> (ProposalResult, kept records)"""
    p = dict(params)
    nms = p.pop('box_nms_thresh')
    state = EP.proposal_state(H, W, 4096, 'cpu')
    EP.proposal_begin(state)
    for logits, iou in batches:
        EP.proposal_batch(state, logits, iou, **p)
    found = EP.proposal_finish(state, nms)
    if len(found.masks) == 0:
        return found, np.zeros((0, 8), np.int32), found
    planes, records = RC.clean(found.masks.numpy(), min_area)
    keep = EP.nms(records[:, 4:8], (1 - records[:, 0]).astype(np.float32), nms if region_nms_thresh is None else region_nms_thresh)
    sel = torch.tensor(keep, dtype=torch.int64)
    return (ops.ProposalResult(torch.from_numpy(planes)[sel], found.iou_preds[sel], found.stability[sel],
                               torch.from_numpy(records[keep][:, 4:8].copy()), found.index[sel]), records[keep], found)


def _filter(batches, params, **kw):
    flt = _new_filter(params, **kw)
    for logits, iou in batches:
        flt.add(logits.to(dev()), iou.to(dev()))
    return flt, flt.finish()


def _new_filter(params, **kw):
    from deva.inference.proposals import ProposalFilter
    return ProposalFilter(H, W, capacity=256, **params, **kw)


def _same_result(got, want):
    same(got.masks, want.masks.numpy(), 'masks')
    assert torch.equal(got.iou_preds.cpu().view(torch.int32), want.iou_preds.view(torch.int32))
    assert torch.equal(got.stability.cpu().view(torch.int32), want.stability.view(torch.int32))
    assert got.boxes.dtype == torch.int32 and torch.equal(got.boxes.cpu(), want.boxes.to(torch.int32).view(-1, 4))
    assert got.index.dtype == torch.int32 and torch.equal(got.index.cpu(), want.index)


def _speckled_frame(b, seed):
    """the ramps of tests/proposal_case.py with what a segmenter adds to them: a far speck on every third plane, a pinhole at
    the disc's centre on the planes after those"""
    logits, iou = PC.batch(H, W, b, seed)
    logits = logits.clone()
    centres = PC.draw(H, W, b, seed)[0]
    for k in range(b):
        if k % 3 == 0:
            logits[k, H - 2, W - 2] = 4.0
        elif k % 3 == 1:
            logits[k, int(centres[k][0]), int(centres[k][1])] = -1.0
    return [(logits, iou), PC.barren(H, W, seed), (torch.zeros(0, H, W), torch.zeros(0))]


@pytest.mark.parametrize('b,min_area', [(24, 12), (67, 40), (3, 200)])
def test_filter_with_small_regions_is_the_three_statements_in_a_row(b, min_area):
    batches = _speckled_frame(b, 100 + b)
    params = PC.params(0.8)
    want, want_regions, before = _statement(batches, params, min_area)
    flt, got = _filter(batches, params, min_mask_region_area=min_area)
    _same_result(got, want)
    assert flt.last_regions.dtype == torch.int32 and np.array_equal(flt.last_regions.numpy(), want_regions)
    changed = want_regions[:, 0]
    assert (np.diff(changed) >= 0).all()                # the masks that needed no fixing first, then the fixed ones
    if b > 3:   # the case does what it is there for: fixed and clean masks both survive, and the second NMS drops some
        assert 0 < changed.sum() < len(changed) and len(changed) < len(before.masks)
        assert want_regions[:, 1].any() and want_regions[:, 2].any()
    # the next frame on the same filter: the buffers are reused
    want2, regions2, _ = _statement(batches[:1], params, min_area)
    flt.add(batches[0][0].to(dev()), batches[0][1].to(dev()))
    _same_result(flt.finish(), want2)
    assert np.array_equal(flt.last_regions.numpy(), regions2)


def _square_planes(specks):
    """logit planes of one clean square (+8 / -8: stability 1), plane k with the far pixels specks[k] set as well"""
    logits = torch.full((len(specks), H, W), -8.0)
    logits[:, 8:24, 10:26] = 8.0
    for k, at in enumerate(specks):
        for y, x in at:
            logits[k, y, x] = 8.0
    return logits


def test_a_duplicate_that_appears_only_after_the_clean_up():
    """A is a clean square, B the same square plus a far speck and the better prediction: the first NMS keeps both (B's box
    is far larger), the clean-up makes the boxes coincide, and B, the one that needed fixing, goes"""
    batches = [(_square_planes([[], [(33, 50)]]), torch.tensor([0.90, 0.99]))]
    params = PC.params(0.8)
    want, want_regions, before = _statement(batches, params, 5)
    assert before.index.tolist() == [1, 0] and want.index.tolist() == [0] and want_regions.tolist() == [[0, 0, 0, 256, 10, 8, 25, 23]]
    flt, got = _filter(batches, params, min_mask_region_area=5)
    _same_result(got, want)
    assert flt.last_regions.tolist() == want_regions.tolist()
    # without the option both stay
    assert _filter(batches, params)[1].index.tolist() == [1, 0]
    # a threshold of its own for the second NMS: at 1.0 nothing overlaps more, both stay, the clean one first
    flt, got = _filter(batches, params, min_mask_region_area=5, region_nms_thresh=1.0)
    _same_result(got, _statement(batches, params, 5, 1.0)[0])
    assert got.index.tolist() == [0, 1] and flt.last_regions[:, 0].tolist() == [0, 1]


def test_of_two_fixed_duplicates_the_earlier_stays():
    batches = [(_square_planes([[(33, 50)], [(2, 50)], [(34, 2), (35, 2)]]), torch.tensor([0.90, 0.99, 0.95]))]
    params = PC.params(0.8)
    want, want_regions, before = _statement(batches, params, 5)
    assert before.index.tolist() == [1, 2, 0] and want.index.tolist() == [1]       # the earlier in the first NMS's order
    assert want_regions.tolist() == [[1, 0, 1, 256, 10, 8, 25, 23]]
    flt, got = _filter(batches, params, min_mask_region_area=5)
    _same_result(got, want)
    assert flt.last_regions.tolist() == want_regions.tolist()


def test_without_the_option_nothing_changes(monkeypatch):
    """min_mask_region_area = 0 is today's filter: the same bits from the same library calls in the same order, and not one
    into the region library"""
    calls = []
    for module in (ops, regions):
        real_check = module.check
        monkeypatch.setattr(module, 'check', lambda code, what, _real=real_check: (calls.append(what), _real(code, what))[1])
    batches = _speckled_frame(24, 124)
    params = PC.params(0.8)
    results, traces = [], []
    for kw in ({}, dict(min_mask_region_area=0), dict(min_mask_region_area=0, region_nms_thresh=0.5)):
        del calls[:]
        flt, got = _filter(batches, params, **kw)
        results.append(got)
        traces.append(list(calls))
        assert flt.last_regions is None and flt._regions is None
    for got, trace in zip(results[1:], traces[1:]):
        _same_result(got, ops.ProposalResult(*(t.cpu() for t in results[0])))
        assert trace == traces[0] and not any('regions' in what for what in trace)
    if not DRYRUN:
        assert len(traces[0]) >= 5              # begin, three batches, finish, gather
        del calls[:]
        _filter(batches, params, min_mask_region_area=12)
        more = [what for what in calls[len(traces[0]):] if what != 'deva_regions_scratch_bytes']       # (host only: a size)
        assert calls[:len(traces[0])] == traces[0] and more == ['deva_regions_clean', 'deva_box_nms']


class SpeckledSegmenter(PromptCase.FakeSegmenter):
    """the stand-in segmenter of the automatic tests, with a pinhole in every rectangle and a speck in a corner of every
    plane that found one"""

    def predict_points(self, points_px):
        logits, iou = super().predict_points(points_px)
        logits = logits.cpu()
        for k in range(len(logits)):
            if float(iou[k]) > 0.9:
                ys, xs = np.nonzero(logits[k].numpy() > 0)
                logits[k, int(ys.mean()), int(xs.mean())] = -8.0
                logits[k, 1 + k % 3, 1] = 8.0
        return logits.to(points_px.device), iou


def test_a_detection_frame_through_the_automatic_processor():
    """`AutomaticProcessor(..., min_mask_region_area=...)`.segment on the first frame of the automatic tests' clip (nothing
    tracked: the whole grid is asked) equals `assemble_automatic` applied to the statement's planes"""
    from deva.inference import detections
    from deva.inference.automatic import AutomaticProcessor
    frames, rects = PromptCase.clip()
    cfg = PromptCase.loop_config('online')
    core = types.SimpleNamespace(config=cfg)           # `segment` reads the configuration alone
    processor = AutomaticProcessor(core, SpeckledSegmenter(frames, rects), capacity=256, min_mask_region_area=6)
    mask, segments = processor.segment(frames[0], None, device=dev())
    h, w = frames[0].shape[:2]
    # the statement: the same batches through the three statements, then the assembly this package already has
    seg = SpeckledSegmenter(frames, rects)
    seg.set_image(frames[0])
    points = (detections.prompt_grid(cfg['SAM_NUM_POINTS_PER_SIDE'], 'cpu').numpy() * np.array([w, h])[None, :]).astype(np.float32)
    state = EP.proposal_state(h, w, 4096, 'cpu')
    EP.proposal_begin(state)
    for first in range(0, len(points), cfg['SAM_NUM_POINTS_PER_BATCH']):
        logits, iou = seg.predict_points(torch.from_numpy(points[first:first + cfg['SAM_NUM_POINTS_PER_BATCH']]))
        EP.proposal_batch(state, logits, iou, pred_iou_thresh=cfg['SAM_PRED_IOU_THRESHOLD'], stability_score_thresh=0.95,
                          stability_score_offset=1.0, mask_threshold=0.0)
    found = EP.proposal_finish(state, 0.7)
    planes, records = RC.clean(found.masks.numpy(), 6)
    assert records[:, 0].all() and records[:, 1].all() and records[:, 2].all()          # every mask had a pinhole and a speck
    keep = EP.nms(records[:, 4:8], (1 - records[:, 0]).astype(np.float32), 0.7)
    assert 0 < len(keep) <= len(planes)
    want_mask, want_segments = detections.assemble_automatic(up(planes[keep]), found.iou_preds[torch.tensor(keep)].to(dev()), (h, w),
                                                             suppress_small_objects=cfg['suppress_small_objects'],
                                                             overlap_threshold=cfg['SAM_OVERLAP_THRESHOLD'])
    assert torch.equal(mask.cpu(), want_mask.cpu()) and len(segments) == len(want_segments) >= 2
    assert [(s.id, s.scores) for s in segments] == [(s.id, s.scores) for s in want_segments]
    assert np.array_equal(processor._filter.last_regions.numpy(), records[keep])
    # and it differs from what the processor finds without the option: the specks and pinholes are in its masks
    plain = AutomaticProcessor(core, SpeckledSegmenter(frames, rects), capacity=256)
    plain_mask, _ = plain.segment(frames[0], None, device=dev())
    assert not torch.equal(plain_mask.cpu(), mask.cpu())
