"""The pair counts (csrc/pair_metrics/pair_counts.hip, `deva.hip.pair_metrics.pair_counts`) on the device against the numpy
statement of their rules (tests/pair_case.py: one boolean plane, one boundary map and one dilation per object and side),
every table for exact equality -- integer adds, so there is no tolerance -- and the unsupervised scorer end to end: a short
clip through `DEVAInferenceCore.step` and `FrameResultSaver(dataset='unsup_davis17', frame_hook=...)` feeding
`ProposalLimiter` and `UnsupervisedVideoScorer` online, against `limit_directory` + `score_directory` on the PNGs that run
wrote.  With DEVA_TEST_DRYRUN=1 the same code runs on the CPU contract."""
import os

import numpy as np
import pytest
import torch

import emu_frame_result as EF
import emu_pairs as EP
import emu_vos as EV
import pair_case as PC
import vos_case as VC
from deva.hip import pair_metrics, vos_metrics
from gpu_util import dev

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DRYRUN = os.environ.get('DEVA_TEST_DRYRUN') == '1'


@pytest.fixture(autouse=True)
def _emulated_when_dry(monkeypatch):
    if DRYRUN:
        EF.install(monkeypatch)
        EV.install(monkeypatch)
        EP.install(monkeypatch)


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def same(got, want):
    out = []
    for g, w, name in zip(got, want, ('singles', 'pairs')):
        g = g.cpu().numpy() if isinstance(g, torch.Tensor) else g
        assert g.dtype == np.uint32 and g.shape == w.shape, (name, g.shape, w.shape)
        assert np.array_equal(g, w), (name, np.argwhere(g != w)[:8].tolist(), g[g != w][:8], w[g != w][:8])
        out.append(g)
    assert not out[1][..., 3].any()
    return out


def run(h, w, n_gt, n_pred, radius, seed, **case_kw):
    """one case in the workload's own encodings (uint8 ground truth, int64 prediction) against the statement"""
    gt, pred, gt_ids, pred_ids = PC.case(h, w, n_gt, n_pred, seed, **case_kw)
    r = VC.radius_of(h, w) if radius is None else radius
    want = PC.counts(gt, pred, gt_ids, pred_ids, r)
    kw = {} if radius is None else dict(radius=radius)
    got = same(pair_metrics.pair_counts(up(gt.astype(np.uint8)), up(pred), gt_ids.tolist(), pred_ids.tolist(), **kw), want)
    return got, (gt, pred, gt_ids, pred_ids)


# ------------------------------------------------------------------------------------------ geometry
# (H, W, objects, proposals, radius, what it guards); radius None: the rule of bound_th = 0.008
GEOMETRY = [(1, 9, 2, 3, 1, 'one row: no S neighbour'),
            (9, 1, 2, 3, 1, 'one column: no E neighbour'),
            (2, 2, 2, 2, 1, 'a single 2 x 2 neighbourhood'),
            (24, 40, 3, 5, 1, 'the five-pixel disk'),
            (37, 53, 5, 7, 3, 'odd sizes, no multiple of the strip, the largest radius a lane searches by itself'),
            (120, 214, 4, 7, None, 'the rule gives 2'),
            (70, 90, 4, 6, 30, 'a disk that leaves the image on every side'),
            (480, 854, 4, 6, 8, 'the workload\'s own shape')]


@pytest.mark.parametrize('h,w,n_gt,n_pred,radius,what', GEOMETRY, ids=[f'{c[0]}x{c[1]}-{c[2]}x{c[3]}-r{c[4]}' for c in GEOMETRY])
def test_tables_equal_the_numpy_statement(h, w, n_gt, n_pred, radius, what):
    if radius is None:
        assert VC.radius_of(h, w) == 2 == vos_metrics.boundary_radius(h, w)
    (singles, pairs), (gt, pred, gt_ids, pred_ids) = run(h, w, n_gt, n_pred, radius, 2000 + h)
    assert singles[:n_gt, 0].sum() == np.isin(gt, gt_ids).sum() and singles[n_gt:, 0].sum() == np.isin(pred, pred_ids).sum()
    assert pairs[..., 0].sum() == (np.isin(gt, gt_ids) & np.isin(pred, pred_ids)).sum()
    if min(h, w) > 2:       # the case exercises what it is there for: several pairs overlap and match on both sides
        assert (pairs[..., 0] > 0).sum() >= 2 and (pairs[..., 1] > 0).sum() >= 2 and (pairs[..., 2] > 0).sum() >= 2, what
    if radius == 30:        # and a wide disk matches pairs that share no pixel
        assert ((pairs[..., 1] > 0) & (pairs[..., 0] == 0)).any(), what


@pytest.fixture(scope='module')
def middle():
    gt, pred, gt_ids, pred_ids = PC.case(96, 128, 5, 8, 31)
    return gt, pred, gt_ids, pred_ids


@pytest.mark.parametrize('radius', [0, 1, 3, 4, 8, 9, 18])
def test_radius_classes(radius, middle):
    """0: the pixel alone; 1, 3: a lane's own box; 4 and above: the wave's lanes together, one to six trips of 256 cells"""
    gt, pred, gt_ids, pred_ids = middle
    pred = np.roll(pred, (2, 5), axis=(0, 1))        # far enough that every class finds more than the one before
    want = PC.counts(gt, pred, gt_ids, pred_ids, radius)
    same(pair_metrics.pair_counts(up(gt.astype(np.uint8)), up(pred), gt_ids.tolist(), pred_ids.tolist(), radius=radius), want)
    if radius:
        less = PC.counts(gt, pred, gt_ids, pred_ids, {1: 0, 3: 1, 4: 3, 8: 4, 9: 8, 18: 9}[radius])[1]
        assert want[1][..., 1].sum() > less[..., 1].sum()


@pytest.mark.parametrize('n_gt,n_pred', [(1, 1), (3, 20), (64, 64), (64, 1)])
def test_table_sizes(n_gt, n_pred):
    """64 x 64: the LDS tables at their largest, bits 32 and above on both sides"""
    (singles, pairs), _ = run(96, 128, n_gt, n_pred, 2, 500 + n_gt + n_pred)
    if n_gt == 64:
        assert (singles[32:64, 0] > 0).sum() >= 5 and (pairs[32:, :, 1] > 0).sum() >= (5 if n_pred > 1 else 1)
    if n_pred == 64:
        assert (singles[64 + 32:, 0] > 0).sum() >= 5 and (pairs[:, 32:, 2] > 0).sum() >= 5


# ------------------------------------------------------------------------------------------ proposal structure
def test_split_merge_absent_and_unlisted():
    gt, pred, gt_ids, pred_ids = PC.case(37, 53, 5, 5, 7, pred_ids=[7, 19, 31, 40, 52])
    pred = pred.copy()
    a, b, c = sorted(pred_ids.tolist(), key=lambda i: -(pred == i).sum())[:3]      # the three largest proposals
    middle = int(np.median(np.nonzero(pred == a)[1]))
    pred[:, middle:][pred[:, middle:] == a] = 60                 # a split: the right half of proposal a becomes 60
    pred[pred == b] = c                                          # a merge: b and c are one proposal, b keeps its slot without a pixel
    gt = np.where(gt == gt_ids[3], 0, gt)                        # a ground-truth object absent from the frame
    table_p = sorted(pred_ids.tolist() + [60, 77])               # 77: listed, nowhere
    gt32, pred32 = gt.astype(np.int32), pred.astype(np.int32)
    gt32[::7, ::5], pred32[::6, ::4] = -3, -2**31                # unlisted values on both sides: negatives, and the 255 of the case
    assert (gt32 == 255).any() and (pred32 == 255).any()
    want = PC.counts(gt32, pred32, gt_ids, table_p, 3)
    singles, pairs = same(pair_metrics.pair_counts(up(gt32), up(pred32), gt_ids.tolist(), table_p, radius=3), want)
    n = len(gt_ids)
    assert not singles[3].any() and not pairs[3].any()                                       # the absent object
    for listed_nowhere in (table_p.index(b), table_p.index(77)):
        assert not singles[n + listed_nowhere].any() and not pairs[:, listed_nowhere].any()
    assert singles[n + table_p.index(60), 0] > 0 and (pairs[:, table_p.index(c), 0] > 0).sum() >= 2      # the split, the merge


def test_ids_near_the_top_of_int32():
    big_g = np.array([5, 70000, 2**31 - 2, 2**31 - 1], dtype=np.int64)
    big_p = np.array([2**31 - 3, 2**31 - 2, 2**31 - 1], dtype=np.int64)
    gt, pred, gt_ids, pred_ids = PC.case(37, 53, 4, 3, 11, gt_ids=big_g, pred_ids=big_p)
    pred = pred.copy()
    pred[3::5, ::4] = 2**31              # one past the last id an int32 holds
    pred[4::5, ::4] = 2**40 + 5          # its low 32 bits are a listed id of the other table
    want = PC.counts(gt, pred, gt_ids, pred_ids, 3)
    singles, _ = same(pair_metrics.pair_counts(up(gt.astype(np.int32)), up(pred), gt_ids.tolist(), pred_ids.tolist(), radius=3), want)
    assert (singles[:, 0] > 0).all()


@pytest.mark.parametrize('offset,matched', [((3, 4), True), ((4, 4), False), ((0, 5), True), ((5, 1), False)])
def test_exact_distance_of_a_pair(offset, matched):
    """single-pixel objects, radius 5: 9 + 16 = 25 <= 25 matches, 16 + 16 = 32 does not.  (A single pixel has the boundary
    pixels (y, x), (y, x - 1), (y - 1, x), (y - 1, x - 1), so the statement, not a hand count, says how many match.)"""
    gt, pred = np.zeros((40, 48), dtype=np.int64), np.zeros((40, 48), dtype=np.int64)
    gt[20, 20] = 1
    pred[20 + offset[0] + 1, 20 + offset[1] + 1] = 9       # the nearest boundary pixels of the two are `offset` apart
    want = PC.counts(gt, pred, [1], [9], 5)
    assert (want[1][0, 0, 1] > 0) == matched and want[0][:, 1].tolist() == [4, 4]
    same(pair_metrics.pair_counts(up(gt.astype(np.uint8)), up(pred), [1], [9], radius=5), want)


# ------------------------------------------------------------------------------------------ encodings
@pytest.fixture(scope='module')
def small():
    gt, pred, gt_ids, pred_ids = PC.case(37, 53, 4, 6, 1037)
    return gt, pred, gt_ids, pred_ids, PC.counts(gt, pred, gt_ids, pred_ids, 3)


@pytest.mark.parametrize('pred_enc', ['u8', 'i32', 'i64', 'index'])
@pytest.mark.parametrize('gt_enc', ['u8', 'i32'])
def test_every_encoding_pair(gt_enc, pred_enc, small):
    gt, pred, gt_ids, pred_ids, want = small
    gt_arg = up(gt.astype(np.uint8 if gt_enc == 'u8' else np.int32))
    if pred_enc == 'index':   # two channels share the first proposal; entries 65535 and n_pred (>= n_pred) are none
        index, lut, channel_ids = VC.channel_form(pred, pred_ids, 3)
        n = len(pred_ids)
        assert (index == n + 1).any() and (index == 1).any() and (lut >= n).sum() == 3 and (lut == n).sum() == 1
        listed = np.where(np.isin(pred, pred_ids), pred, 0)
        assert all(np.array_equal(a, b) for a, b in zip(PC.counts(gt, listed, gt_ids, pred_ids, 3), want))     # (255 is unlisted anyway)
        assert all(np.array_equal(a, b) for a, b in zip(PC.counts(gt, index, gt_ids, n, 3, pred_lut=lut), want))
        for ids_arg in (pred_ids.tolist(), n):        # the table is not read with the channel plane: its length will do
            same(pair_metrics.pair_counts(gt_arg, up(index), gt_ids.tolist(), ids_arg, radius=3, pred_lut=up(lut)), want)
    else:
        dtype = {'u8': np.uint8, 'i32': np.int32, 'i64': np.int64}[pred_enc]
        same(pair_metrics.pair_counts(gt_arg, up(pred.astype(dtype)), gt_ids.tolist(), pred_ids.tolist(), radius=3), want)


# ------------------------------------------------------------------------------------------ identities
def test_one_table_on_both_sides_is_boundary_counts():
    gt, pred, ids = VC.case(64, 96, 40, 1064)
    for radius in (2, 5):
        singles, pairs = (t.cpu().numpy() for t in pair_metrics.pair_counts(up(gt.astype(np.uint8)), up(pred), ids.tolist(), ids.tolist(),
                                                                            radius=radius))
        records = vos_metrics.boundary_counts(up(gt.astype(np.uint8)), up(pred), ids.tolist(), radius=radius).cpu().numpy()
        n = len(ids)
        diag = np.arange(n)
        rebuilt = np.stack([pairs[diag, diag, 0], singles[:n, 0], singles[n:, 0], singles[:n, 1], singles[n:, 1], pairs[diag, diag, 1],
                            pairs[diag, diag, 2], np.zeros(n, dtype=np.uint32)], axis=1)
        assert np.array_equal(rebuilt, records) and records[32:, 5].sum() > 0


def test_every_pair_is_a_boundary_counts_call_on_relabelled_planes(small):
    gt, pred, gt_ids, pred_ids, want = small
    singles, pairs = want
    for g, gid in enumerate(gt_ids.tolist()):
        for p, pid in enumerate(pred_ids.tolist()):
            rec = vos_metrics.boundary_counts(up((gt == gid).astype(np.uint8)), up((pred == pid).astype(np.uint8)), [1], radius=3)
            assert np.array_equal(rec.cpu().numpy()[0].astype(np.int64), PC.record(singles, pairs, g, p)), (gid, pid)


# ------------------------------------------------------------------------------------------ hygiene
def test_dirty_outputs_exact_scratch_and_two_runs(small):
    gt, pred, gt_ids, pred_ids, want = small
    if DRYRUN:
        pytest.skip('the library owns the scratch and the outputs')
    n_gt, n_pred = len(gt_ids), len(pred_ids)
    need = pair_metrics.pair_scratch_bytes(37, 53)
    assert need == 16 * 37 * 53
    scratch = torch.full((need + 64,), 0xFF, dtype=torch.uint8, device=dev())
    one = torch.full((n_gt + n_pred + 3, 2), -1, dtype=torch.int32, device=dev()).view(torch.uint32)      # 0xFF everywhere, 3 guard rows
    two = torch.full((n_gt + 2, n_pred, 4), -1, dtype=torch.int32, device=dev()).view(torch.uint32)       # 2 guard rows
    out = (one[:n_gt + n_pred], two[:n_gt])
    runs = []
    for _ in range(2):
        got = pair_metrics.pair_counts(up(gt.astype(np.uint8)), up(pred), gt_ids.tolist(), pred_ids.tolist(), radius=3,
                                       scratch=scratch[:need], out=out)
        assert got[0] is out[0] and got[1] is out[1]
        runs.append(same(got, want))
    assert all(np.array_equal(a, b) for a, b in zip(*runs))
    assert (scratch[need:] == 0xFF).all()                 # nothing is written past what the size function announces
    assert (one[n_gt + n_pred:].view(torch.int32) == -1).all() and (two[n_gt:].view(torch.int32) == -1).all()
    tables = (up(gt_ids.astype(np.int32)), up(pred_ids.astype(np.int32)))
    same(pair_metrics.pair_counts(up(gt.astype(np.uint8)), up(pred), *tables, radius=3, validate=False), want)


# ------------------------------------------------------------------------------------------ end to end
H, W, FRAMES, OBJECTS = 96, 128, 6, [1, 2, 3, 4, 5]


def test_clip_through_the_saver_the_limiter_and_the_scorer(peaky_state_dict, tmp_path):
    """the smoke-size clip of test_gpu_u_vos_quality.py, saved as an unsupervised run: `DEVAInferenceCore.step` ->
    `FrameResultSaver(dataset='unsup_davis17', frame_hook=...)` -> `ProposalLimiter.add_frame(areas)` ->
    `UnsupervisedVideoScorer.add_frame(FrameResult, gt, keep=...)`, against the offline forms on the PNGs that run wrote:
    `limit_directory`, then `score_directory` on its output.  The limiter keeps 3 of the 5 tracks, so the two orders of
    work -- drop online through the channel table, or relabel the files first -- must agree on every integer; the
    proposal ids differ (the tracker's ids online, the limiter's 1 .. 3 offline) and are compared through its mapping."""
    from PIL import Image
    from deva.inference.frame_results import FrameResultSaver
    from deva.inference.inference_core import DEVAInferenceCore
    from deva.inference.unsup_quality import ProposalLimiter, UnsupervisedVideoScorer, limit_directory, score_directory
    from deva.model.network import DEVA
    from workload import synth
    cfg = synth.base_config(mem_every=2)
    net = DEVA(cfg)
    net.load_weights(peaky_state_dict)
    core = DEVAInferenceCore(net.to(dev()).eval(), cfg)
    mask = synth.box_mask(H, W, len(OBJECTS))
    truth = [np.roll(mask.numpy(), (t, t), axis=(0, 1)).astype(np.uint8) for t in range(FRAMES)]
    truth_dev = [up(p) for p in truth]
    limiter = ProposalLimiter(3, distinct=True)
    scorer = UnsupervisedVideoScorer()
    scorer.start_video('clip', [1, 2, 3, 4])
    fed = []

    def hook(name, result, annotation):      # the saver's worker: the frame's file is written, its planes still on the device
        t = int(name[:-4])
        assert result.index is not None and result.index.dtype == torch.int16
        keep = limiter.add_frame({s['id']: s['area'] for s in result.segments})
        scorer.add_frame(result, truth_dev[t], keep=keep)
        fed.append(t)

    saver = FrameResultSaver(str(tmp_path / 'run'), 'clip', dataset='unsup_davis17', object_manager=core.object_manager, frame_hook=hook)
    stream = synth.FrameStream(H, W, seed=1)
    for t in range(FRAMES):
        prob = core.step(stream.next().to(dev()), mask.to(dev()) if t == 0 else None, OBJECTS if t == 0 else None)
        saver.save_mask(prob, f'{t:05d}.jpg')
    saver.end()
    assert fed == list(range(FRAMES)) and saver.error is None
    scorer.end_video()
    online = scorer.result()

    for t, plane in enumerate(truth):
        os.makedirs(tmp_path / 'truth' / 'clip', exist_ok=True)
        img = Image.fromarray(np.where(plane <= 4, plane, 0).astype(np.uint8), mode='P')     # four objects are annotated
        img.putpalette([v for i in range(256) for v in (i, 255 - i, (7 * i) % 256)])
        img.save(tmp_path / 'truth' / 'clip' / f'{t:05d}.png')
    maps = limit_directory(str(tmp_path / 'run'), str(tmp_path / 'limited'), 3, distinct=True)
    assert maps['clip'] == limiter.mapping() and len(maps['clip']) == 3 and limiter.full
    offline = score_directory(str(tmp_path / 'limited'), str(tmp_path / 'truth'), ['clip'])
    a, b = online['frames']['clip'], offline['frames']['clip']
    renamed = [None if p is None else maps['clip'][p] for p in a['proposals']]
    order = [renamed.index(p) for p in b['proposals']]                   # the offline rows in the online numbering
    assert sorted(x for x in renamed if x is not None) == [1, 2, 3] and b['proposals'] == [1, 2, 3, None]
    assert np.array_equal(a['counts'][order], b['counts']) and np.array_equal(a['score'][order], b['score'])
    assert {g: None if p is None else maps['clip'][p] for g, p in a['assignment'].items()} == b['assignment']
    assert online['global'] == offline['global'] and online['sequences'] == offline['sequences']
    # the run scored something, and the pair table was needed: some object is assigned a proposal
    assert a['counts'][..., 0].sum() > 0 and a['counts'][..., 5].sum() > 0 and any(p is not None for p in a['assignment'].values())
    assert sum(p is None for p in a['assignment'].values()) == 1        # 3 proposals for 4 objects: one padded row (U2)
