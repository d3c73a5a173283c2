"""The DAVIS counts (csrc/vos_metrics/boundary_counts.hip, `deva.hip.vos_metrics.boundary_counts`) on the device against
the numpy statement of their rules (tests/vos_case.py: one boolean plane per object, the toolkits' boundary map, dilation
by shifted ORs), every record for exact equality -- integer adds, so there is no tolerance -- and the scorer end to end: a
short clip through `DEVAInferenceCore.step` and `FrameResultSaver(frame_hook=...)` with `VideoObjectScorer` fed online
from the channel plane, against the statement applied to the PNGs that run wrote.  With DEVA_TEST_DRYRUN=1 the same code
runs on the CPU contract."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

import emu_frame_result as EF
import emu_vos as EV
import vos_case as VC
from deva.hip import vos_metrics
from gpu_util import dev

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DRYRUN = os.environ.get('DEVA_TEST_DRYRUN') == '1'


@pytest.fixture(autouse=True)
def _emulated_when_dry(monkeypatch):
    if DRYRUN:
        EF.install(monkeypatch)
        EV.install(monkeypatch)


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def same(got, want):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.dtype == np.uint32 and got.shape == want.shape
    assert np.array_equal(got, want), (np.argwhere(got != want)[:8].tolist(), got[got != want][:8], want[got != want][:8])
    assert not got[:, 7].any()
    return got


def run(h, w, n, radius, seed, bound_th=None):
    """one case in the workload's own encodings (uint8 ground truth, int64 prediction) against the statement"""
    gt, pred, ids = VC.case(h, w, n, seed)
    r = VC.radius_of(h, w) if radius is None else radius
    want = VC.counts(gt, pred, ids, r)
    kw = dict(radius=radius) if bound_th is None else dict(bound_th=bound_th)
    got = same(vos_metrics.boundary_counts(up(gt.astype(np.uint8)), up(pred), ids.tolist(), **kw), want)
    return got, (gt, pred, ids)


# (H, W, objects, radius, what it guards); radius None: the rule of bound_th = 0.008
CASES = [(37, 53, 5, 3, 'odd sizes, objects cut by every image edge and the corner'),
         (24, 40, 3, None, 'the rule gives 1: the five-pixel disk'),
         (64, 96, 40, 5, 'bits 32 and above'),
         (33, 65, 64, 2, 'every bit of the word'),
         (33, 65, 70, 2, 'more than 64 ids: chunks in the binding'),
         (17, 19, 2, 8, 'a disk wider than the image'),
         (1, 9, 2, 1, 'one row: no S neighbour'),
         (9, 1, 2, 1, 'one column: no E neighbour'),
         (70, 150, 6, 20, 'a disk across several workgroups\' pixels'),
         (120, 214, 7, None, 'the rule gives 2'),
         (480, 854, 3, None, 'the workload\'s own shape: the rule gives 8')]


@pytest.mark.parametrize('h,w,n,radius,what', CASES, ids=[f'{c[0]}x{c[1]}-{c[2]}obj-r{c[3]}' for c in CASES])
def test_records_equal_the_numpy_statement(h, w, n, radius, what):
    if radius is None:
        assert VC.radius_of(h, w) == {(24, 40): 1, (120, 214): 2, (480, 854): 8}[(h, w)] == vos_metrics.boundary_radius(h, w)
    got, (gt, pred, ids) = run(h, w, n, radius, 1000 + h)
    assert got[:, 1].sum() == np.isin(gt, ids).sum() and got[:, 2].sum() == np.isin(pred, ids).sum()
    seen = (got[:, 1] > 0) & (got[:, 2] > 0) & (got[:, 5] > 0)
    assert seen.sum() >= (1 if min(h, w) == 1 else 2) and (n < 33 or seen[32:].sum() >= 5), what       # the case exercises what it is there for
    if radius is None:       # the rule through bound_th, as a radius in pixels, gives the same records
        r = VC.radius_of(h, w)
        assert np.array_equal(vos_metrics.boundary_counts(up(gt.astype(np.int32)), up(pred), ids.tolist(), bound_th=r).cpu().numpy(), got)


@pytest.fixture(scope='module')
def small():
    gt, pred, ids = VC.case(37, 53, 5, 1037)
    return gt, pred, ids, VC.counts(gt, pred, ids, 3)


@pytest.mark.parametrize('pred_enc', ['u8', 'i32', 'i64', 'index'])
@pytest.mark.parametrize('gt_enc', ['u8', 'i32'])
def test_every_encoding_pair(gt_enc, pred_enc, small):
    gt, pred, ids, want = small
    gt_arg = up(gt.astype(np.uint8 if gt_enc == 'u8' else np.int32))
    if pred_enc == 'index':   # two channels share the first object; entries 65535 and n (>= n) are none
        index, lut, channel_ids = VC.channel_form(pred, ids, 3)
        assert (index == len(ids) + 1).any() and (index == 1).any() and (lut >= len(ids)).sum() == 3
        listed = np.where(np.isin(pred, ids), pred, 0)
        want = VC.counts(gt, listed, ids, 3)
        assert np.array_equal(want, VC.counts(gt, index, ids, 3, pred_lut=lut))
        got = vos_metrics.boundary_counts(gt_arg, up(index), ids.tolist(), radius=3, pred_lut=up(lut))
    else:
        dtype = {'u8': np.uint8, 'i32': np.int32, 'i64': np.int64}[pred_enc]
        got = vos_metrics.boundary_counts(gt_arg, up(pred.astype(dtype)), ids.tolist(), radius=3)
    same(got, want)


def test_values_that_no_table_lists(small):
    """negative values, values beyond int32 in an int64 plane, a table of large ids"""
    gt, pred, ids, _ = small
    big = np.array([7, 300, 70000, 2**31 - 2, 2**31 - 1], dtype=np.int64)
    gt_big, pred_big = np.concatenate([[0], big])[gt % 6], np.concatenate([[0], big])[pred % 6]      # 255 % 6 = 3: listed
    pred_big = pred_big.copy()
    pred_big[::5, ::3] = -3
    pred_big[1::5, ::4] = 2**31            # one past the last id an int32 holds
    pred_big[2::5, ::4] = -2**31 - 1
    pred_big[3::5, ::4] = 2**40 + 7        # its low 32 bits are a listed id
    want = VC.counts(gt_big, pred_big, big, 3)
    same(vos_metrics.boundary_counts(up(gt_big.astype(np.int32)), up(pred_big), big.tolist(), radius=3), want)
    gt_neg = gt_big.copy()
    gt_neg[::4, ::2] = -7
    same(vos_metrics.boundary_counts(up(gt_neg.astype(np.int32)), up(pred_big), big.tolist(), radius=3),
         VC.counts(gt_neg, pred_big, big, 3))


@pytest.mark.parametrize('binary', [True, 'gt', 'pred'])
def test_binary_planes(binary, small):
    """DAVIS 2016 / saliency: 0 / 255 planes, every non-zero value is the single object (id 3 here)"""
    gt, pred, ids, _ = small
    gt_b = binary in (True, 'gt')
    pred_b = binary in (True, 'pred')
    gt_arg = np.where(gt != 0, 255, 0) if gt_b else gt
    pred_arg = np.where(pred != 0, 255, 0) if pred_b else pred
    want = VC.counts(gt_arg, pred_arg, [3], 3, gt_binary=gt_b, pred_binary=pred_b)
    assert np.array_equal(want, VC.counts(gt != 0 if gt_b else gt == 3, pred != 0 if pred_b else pred == 3, [1], 3))
    same(vos_metrics.boundary_counts(up(gt_arg.astype(np.uint8)), up(pred_arg.astype(np.uint8)), [3], radius=3, binary=binary), want)
    if binary is True:      # the channel plane: every channel but 0 is the object
        index, lut, _ = VC.channel_form(pred, ids, 5)
        got = vos_metrics.boundary_counts(up(gt_arg.astype(np.int32)), up(index), [3], radius=3, binary=True, pred_lut=up(lut))
        same(got, VC.counts(gt_arg, index, [3], 3, gt_binary=True, pred_binary=True))


def test_absent_objects_and_a_perfect_prediction(small):
    gt, pred, ids, want = small
    # object 2 absent from the prediction, object 4 from both sides, 9 and 200 listed but nowhere
    pred2 = np.where(np.isin(pred, (2, 4)), 0, pred)
    gt2 = np.where(gt == 4, 0, gt)
    table = [1, 2, 3, 4, 5, 9, 200]
    got = same(vos_metrics.boundary_counts(up(gt2.astype(np.uint8)), up(pred2), table, radius=3), VC.counts(gt2, pred2, table, 3))
    assert got[1, 1] > 0 and got[1, 3] > 0 and not got[1, [0, 2, 4, 5, 6]].any()
    assert not got[[3, 5, 6]].any()
    # the prediction is the ground truth: every boundary pixel is matched, at radius 0 already
    for r in (0, 3):
        got = same(vos_metrics.boundary_counts(up(gt.astype(np.uint8)), up(gt), ids.tolist(), radius=r), VC.counts(gt, gt, ids, r))
        assert np.array_equal(got[:, 0], got[:, 1]) and np.array_equal(got[:, 3], got[:, 5]) and np.array_equal(got[:, 4], got[:, 6])
        assert got[:, 3].sum() > 0
    # radius 0 on the shifted prediction: only coinciding boundary pixels match
    same(vos_metrics.boundary_counts(up(gt.astype(np.uint8)), up(pred), ids.tolist(), radius=0), VC.counts(gt, pred, ids, 0))


@pytest.mark.parametrize('radius', [4, 8, 11, 12, 30])
def test_far_predictions_reach_the_outer_boxes(radius):
    """the prediction is the ground truth moved by (5, 9): nothing is matched within the box a lane searches itself
    (radius 3), part within the wave's first box (8), the rest only in the whole box"""
    gt, _, ids = VC.case(70, 150, 6, 21)
    pred = np.roll(gt, (5, 9), axis=(0, 1))
    want = VC.counts(gt, pred, ids, radius)
    inner = VC.counts(gt, pred, ids, 3)
    assert want[:, 5].sum() > inner[:, 5].sum() + 50
    if radius > 8:
        assert want[:, 5].sum() > VC.counts(gt, pred, ids, 8)[:, 5].sum() + 50
    same(vos_metrics.boundary_counts(up(gt.astype(np.uint8)), up(pred), ids.tolist(), radius=radius), want)


def test_dirty_scratch_and_a_reused_output(small):
    gt, pred, ids, want = small
    if DRYRUN:
        pytest.skip('the library owns the scratch')
    need = vos_metrics.boundary_scratch_bytes(37, 53)
    scratch = torch.full((need + 64,), 0xFF, dtype=torch.uint8, device=dev())
    out = torch.full((5, 8), 7, dtype=torch.int32, device=dev()).view(torch.uint32)
    for _ in range(2):
        assert vos_metrics.boundary_counts(up(gt.astype(np.uint8)), up(pred), ids.tolist(), radius=3, scratch=scratch, out=out) is out
        same(out, want)
    assert (scratch[need:] == 0xFF).all()                 # nothing is written past what the size function announces
    ids_dev = up(ids.astype(np.int32))
    same(vos_metrics.boundary_counts(up(gt.astype(np.uint8)), up(pred), ids_dev, radius=3, validate=False), want)


def test_chunks_with_the_channel_plane():
    """70 objects through the channel plane: the binding re-bases the channel table for every chunk of 64"""
    gt, pred, ids = VC.case(33, 65, 70, 77)
    index, lut, _ = VC.channel_form(pred, ids, 1)
    want = VC.counts(gt, index, ids, 2, pred_lut=lut)
    got = same(vos_metrics.boundary_counts(up(gt.astype(np.uint8)), up(index), ids.tolist(), radius=2, pred_lut=up(lut)), want)
    assert got[64:, 2].sum() > 0


# ------------------------------------------------------------------------------------------ end to end
H, W, FRAMES, OBJECTS = 96, 128, 6, [1, 2, 3, 4, 5]


def test_clip_through_the_saver_and_the_scorer(peaky_state_dict, tmp_path):
    """the smoke-size clip (96 x 128, `synth.FrameStream(seed=1)`, mem_every=2) with 5 objects: `DEVAInferenceCore.step` ->
    `FrameResultSaver(frame_hook=...)` -> `VideoObjectScorer.add_frame(FrameResult, gt)`; annotations: the first frame's
    boxes drifting one pixel a frame.  Counts equal the statement on the PNGs exactly; J, F, the statistics and the table
    within 1e-12 (both sides evaluate the same expressions on the same integers: the margin covers the order of a mean)"""
    from deva.inference.frame_results import FrameResultSaver
    from deva.inference.inference_core import DEVAInferenceCore
    from deva.inference.vos_quality import GLOBAL_HEADER, VideoObjectScorer
    from deva.model.network import DEVA
    from workload import synth
    cfg = synth.base_config(mem_every=2)
    net = DEVA(cfg)
    net.load_weights(peaky_state_dict)
    core = DEVAInferenceCore(net.to(dev()).eval(), cfg)
    mask = synth.box_mask(H, W, len(OBJECTS))
    truth = [np.roll(mask.numpy(), (t, t), axis=(0, 1)).astype(np.uint8) for t in range(FRAMES)]
    truth_dev = [up(p) for p in truth]
    scorer = VideoObjectScorer()
    scorer.start_video('clip', OBJECTS)
    fed = []

    def hook(name, result, annotation):      # the saver's worker: the frame's file is written, its planes still on the device
        t = int(name[:-4])
        assert result.index is not None and result.index.dtype == torch.int16 and result.channel_ids.tolist()[1:] == OBJECTS
        scorer.add_frame(result, truth_dev[t])
        fed.append(t)

    saver = FrameResultSaver(str(tmp_path), 'clip', dataset='unsup_davis17', object_manager=core.object_manager, frame_hook=hook)
    stream = synth.FrameStream(H, W, seed=1)
    for t in range(FRAMES):
        prob = core.step(stream.next().to(dev()), mask.to(dev()) if t == 0 else None, OBJECTS if t == 0 else None)
        saver.save_mask(prob, f'{t:05d}.jpg')
    saver.end()
    assert fed == list(range(FRAMES)) and saver.error is None
    scorer.end_video()
    res = scorer.result()

    written = [np.array(Image.open(tmp_path / 'clip' / f'{t:05d}.png')) for t in range(FRAMES)]
    radius = VC.radius_of(H, W)
    assert radius == 2 and written[0].dtype == np.uint8
    want = np.stack([VC.counts(g, p, OBJECTS, radius) for g, p in zip(truth, written)])
    got = res['frames']['clip']
    assert np.array_equal(got['counts'], want) and got['ids'] == OBJECTS
    per_object = []
    for k in range(len(OBJECTS)):
        jf = [VC.jf(rec) for rec in want[1:-1, k]]
        j, f = [a for a, _ in jf], [b for _, b in jf]
        per_object.append(('clip', k + 1, j, f))
        assert np.allclose(got['J'][k], j, rtol=0, atol=1e-12) and np.allclose(got['F'][k], f, rtol=0, atol=1e-12)
        seq = res['sequences'][f'clip_{k + 1}']
        assert abs(seq['J-Mean'] - VC.statistics(j)[0]) <= 1e-12 and abs(seq['F-Mean'] - VC.statistics(f)[0]) <= 1e-12
    table = VC.table(per_object)
    print('clip:', dict(zip(GLOBAL_HEADER, (float('%.4f' % v) for v in table))))
    assert np.allclose([res['global'][k] for k in GLOBAL_HEADER], table, rtol=0, atol=1e-12, equal_nan=True)
    # the run scored something (the recipe's weights are no tracker: low numbers, but not an empty comparison)
    assert (want[1:-1, :, 0].sum(axis=0) > 0).sum() >= 3 and want[1:-1, :, 5].sum() > 0 and want[1:-1, :, 6].sum() > 0
    assert 0.0 < res['global']['J-Mean'] < 1.0 and 0.0 < res['global']['F-Mean'] < 1.0
    # the offline form on the tree the run wrote gives the same result
    from deva.inference.vos_quality import score_directory
    for t, plane in enumerate(truth):
        os.makedirs(tmp_path / 'truth' / 'clip', exist_ok=True)
        Image.fromarray(plane).save(tmp_path / 'truth' / 'clip' / f'{t:05d}.png')
    offline = score_directory(str(tmp_path), str(tmp_path / 'truth'), ['clip'])
    assert np.array_equal(offline['frames']['clip']['counts'], want) and offline['global'] == res['global']
