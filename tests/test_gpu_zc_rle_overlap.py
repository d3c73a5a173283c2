"""The run-length overlap (csrc/rle_overlap/rle_overlap.hip, `deva.hip.rle_overlap`) on the device against the numpy
statement of its rules (tests/overlap_case.py) for exact equality -- integers, so there is no tolerance -- with every
output inside a sentinel-filled buffer (so a pair that the box test drops is seen to be written, and nothing beside the
tables is).  With DEVA_TEST_DRYRUN=1 the same code runs on the CPU contract (tests/emu_overlap.py)."""
import os

import numpy as np
import pytest
import torch

import emu_overlap as EO
import overlap_case as OC
import rle_case as LC
from deva.hip import rle, rle_overlap as ro
from gpu_util import dev

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DRYRUN = os.environ.get('DEVA_TEST_DRYRUN') == '1'
SENTINEL = -0x5A5A5A5B          # in every int32 word of a guarded buffer: garbage where a table is to be written
PAD = 16


@pytest.fixture(autouse=True)
def _emulated_when_dry(monkeypatch):
    if DRYRUN:
        EO.install(monkeypatch)


def guard(count):
    """-> (the whole buffer, sentinel-filled; its middle `count` elements)"""
    whole = torch.full((count + 2 * PAD,), SENTINEL, dtype=torch.int32, device=dev())
    return whole, whole[PAD:PAD + count]


def untouched(whole, count, what):
    host = whole.cpu()
    assert (host[:PAD] == SENTINEL).all() and (host[PAD + count:] == SENTINEL).all(), f'{what}: written outside its range'


def check_call(dt, gt, h, w, what, want=None, **kw):
    """one `intersections` with every output guarded and pre-filled with garbage -> the statement's tables"""
    want = OC.statement(dt, gt, h, w) if want is None else want
    n_d, n_g = len(dt), len(gt)
    inter_all, inter = guard(n_d * n_g)
    d_all, area_d = guard(n_d)
    g_all, area_g = guard(n_g)
    out = {'inter': inter.view(n_d, n_g), 'area_d': area_d, 'area_g': area_g}
    got = rle.intersections(OC.as_rles(dt, h, w), OC.as_rles(gt, h, w), out=out, source_size=(h, w), **kw)
    assert got[0].data_ptr() == inter.data_ptr() and got[1].data_ptr() == area_d.data_ptr() and got[2].data_ptr() == area_g.data_ptr()
    for name, t, b in zip(('inter', 'area_d', 'area_g'), got, want):
        assert np.array_equal(t.cpu().numpy().astype(np.int64), b), f'{what}: {name}'
    untouched(inter_all, n_d * n_g, what + ': inter')
    untouched(d_all, n_d, what + ': area_d')
    untouched(g_all, n_g, what + ': area_g')
    return want


@pytest.mark.parametrize('size', OC.GEOMETRIES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_every_kind_of_mask_against_every_kind(size):
    """empty, full, zero counts first, in the middle and last, stripes, the checkerboard (one run a pixel: at 480 x 854
    far above the LDS threshold), blobs; the reversed list on the other side, so identical masks meet as well"""
    h, w = size
    dt, gt = OC.geometry_case(h, w)
    inter, area_d, area_g = check_call(dt, gt, h, w, f'{h}x{w}')
    names = LC.row(h, w)[0]
    full, empty = names.index('full'), names.index('empty')
    assert area_d[full] == h * w and area_d[empty] == 0 and (inter[empty] == 0).all() and np.array_equal(inter[full], area_g)
    for k in range(len(dt)):                                   # gt is dt reversed: identical masks overlap in their area
        assert inter[k, len(dt) - 1 - k] == area_d[k]


@pytest.mark.parametrize('shape', ['1x1', '1x7', '7x1', 'below', 'at', 'above', '0x3', '3x0'])
def test_table_shapes_around_the_d_chunk_of_a_workgroup(shape):
    chunk = ro.overlap_limits().d_chunk
    n_d, n_g = {'below': (chunk - 1, 3), 'at': (chunk, 3), 'above': (chunk + 1, 3)}.get(shape) or tuple(int(v) for v in shape.split('x'))
    h, w = 63, 65
    pool = OC.small_blobs(h, w, n_d + n_g, seed=7)
    dt, gt = pool[:n_d], pool[n_d:n_d + n_g]
    if n_d > 2:
        dt[1] = LC.counts_of(LC.blobs(h, w, 3))
        dt[-1] = [0, h * w]                                    # the last detection of the table (of a chunk of its own when 'above') meets everything
    inter, _, area_g = check_call(dt, gt, h, w, shape)
    assert inter.shape == (n_d, n_g) and (n_d <= 2 or (np.array_equal(inter[-1], area_g) and area_g.all()))


def test_masks_that_touch_in_one_pixel_and_identical_masks():
    for h, w in ((2, 2), (1, 9), (9, 1), (63, 65)):
        dt, gt = OC.touching(h, w)
        inter = check_call(dt, gt + dt, h, w, f'touching {h}x{w}')[0]
        assert inter.tolist() == [[1, 0, h * w // 2 + 1]]


def test_box_disjoint_pairs_are_written_zero_over_garbage():
    for h, w in ((2, 4), (63, 65), (480, 854)):
        dt, gt = OC.box_disjoint(h, w)
        boxes_d, boxes_g = OC.boxes_of(dt, h, w), OC.boxes_of(gt, h, w)
        assert boxes_d[0][2] < boxes_g[0][0]                   # the first pair's boxes share no pixel ...
        inter = check_call(dt, gt, h, w, f'box-disjoint {h}x{w}')[0]           # ... and the sentinel in its place is gone
        assert inter[0, 0] == 0 and inter[0, 2] > 0 and inter[1, 1] == w and inter[1, 0] > 0


@pytest.mark.parametrize('side', ['gt', 'dt', 'both'])
def test_run_counts_on_both_sides_of_the_lds_threshold(side):
    """L - 1, L and L + 1 runs (the column checkerboard cut short, on the smallest frame that holds L + 1 runs) against
    blobs and against each other: a g of L runs is walked in LDS, one of L + 1 on global memory"""
    top = ro.overlap_limits().lds_runs
    h, w = OC.threshold_frame(top)
    edge = [OC.run_counts(r, h, w) for r in (top - 1, top, top + 1)]
    assert [len(c) for c in edge] == [top - 1, top, top + 1]
    others = OC.small_blobs(h, w, 3, seed=11) + [[0, h * w]]
    dt, gt = {'gt': (others, edge), 'dt': (edge, others), 'both': (edge, edge)}[side]
    inter, area_d, _ = check_call(dt, gt, h, w, f'threshold ({side})')
    if side == 'both':
        assert np.array_equal(np.diag(inter), area_d) and area_d[2] == h * w // 2   # a mask against itself; the whole checkerboard


def test_a_two_run_mask_against_a_mask_above_the_threshold_in_both_orders():
    top = ro.overlap_limits().lds_runs
    h, w = OC.threshold_frame(top)
    few, many = [[h * w // 2, h * w - h * w // 2]], [OC.run_counts(top + 1, h, w)]
    assert check_call(few, many, h, w, 'few x many')[0].tolist() == [[h * w // 4]]
    assert check_call(many, few, h, w, 'many x few')[0].tolist() == [[h * w // 4]]


@pytest.fixture(scope='module')
def blobs_1080():
    """64 x 64 blob masks at 1080 x 1920 and the statement's tables, computed once"""
    h, w = 1080, 1920
    pool = OC.small_blobs(h, w, 128, seed=3, radius=150)
    dt, gt = pool[:64], pool[64:]
    return dt, gt, OC.statement(dt, gt, h, w, direct=False)


def test_64_by_64_blobs_at_1080p(blobs_1080):
    dt, gt, want = blobs_1080
    assert 0 < np.count_nonzero(want[0]) < want[0].size        # some pairs overlap, some boxes are apart
    check_call(dt, gt, 1080, 1920, '64x64 at 1080p', want=want)


def test_chunked_calls_equal_the_single_call():
    h, w = 63, 65
    dt, gt = OC.geometry_case(h, w)
    most = max(len(c) for c in dt + gt)
    want = OC.statement(dt, gt, h, w)
    for kw in (dict(max_masks=1), dict(max_masks=3), dict(max_words=most + 3), dict(max_masks=4, max_words=2 * most + 5)):
        check_call(dt, gt, h, w, f'chunked {kw}', want=want, **kw)


def test_a_block_of_a_wider_table_leaves_the_gap_alone():
    """O3: inter[d * pitch + g] with pitch > G; the words between the rows keep their sentinel"""
    h, w = 33, 67
    dt, gt = OC.small_blobs(h, w, 5, seed=1), OC.small_blobs(h, w, 4, seed=2)
    want = OC.statement(dt, gt, h, w)
    table = torch.full((5, 9), SENTINEL, dtype=torch.int32, device=dev())
    parsed = [rle.parse_checked(OC.as_rles(c, h, w), (h, w)) for c in (dt, gt)]
    on_gpu = dev().type == 'cuda'
    sides = [ro._side(p, 0, int(p.per_mask.size), k, on_gpu) for k, p in enumerate(parsed)]
    sides = [s._replace(device=s.host.to(dev())) for s in sides]
    scratch = torch.empty(sides[1].words - sides[1].n - 1, dtype=torch.int32, device=dev())
    area_d, area_g = torch.empty(5, dtype=torch.int32, device=dev()), torch.empty(4, dtype=torch.int32, device=dev())
    ro._launch(sides[0], sides[1], h, w, scratch, table[:, 2:6], area_d, area_g, None)
    host = table.cpu().numpy()
    assert np.array_equal(host[:, 2:6], want[0]) and (host[:, :2] == SENTINEL).all() and (host[:, 6:] == SENTINEL).all()
    assert np.array_equal(area_d.cpu().numpy(), want[1]) and np.array_equal(area_g.cpu().numpy(), want[2])


def test_iou_and_the_pending_form():
    h, w = 63, 65
    dt, gt = OC.geometry_case(h, w)
    want = OC.statement(dt, gt, h, w)
    rles_d, rles_g = OC.as_rles(dt, h, w), OC.as_rles(gt, h, w)
    crowd = [k % 3 == 0 for k in range(len(gt))]
    kw = dict(device=dev())
    assert np.array_equal(rle.iou(rles_d, rles_g, **kw), OC.iou(*want))
    assert np.array_equal(rle.iou(rles_d, rles_g, crowd, **kw), OC.iou(*want, crowd))
    queued = [rle.intersections(rles_d[k:], rles_g, pending=True, **kw) for k in range(3)]      # queued without a wait, copied once
    for k, pending in enumerate(queued):
        got = pending.finish()
        assert np.array_equal(got[0], want[0][k:]) and np.array_equal(got[1], want[1][k:]) and np.array_equal(got[2], want[2])
