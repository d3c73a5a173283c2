"""The joint count (csrc/metrics/panoptic_counts.hip, `deva.hip.metrics.panoptic_counts`) on the device against its CPU
contract (tests/emu_panoptic.py), bit for bit -- integer adds, so there is no tolerance -- with counts.sum() == H * W, and
the scorer end to end: the semi-online clip through `FrameResultSaver('vipseg', id_postprocessor=StuffMerger(...))` with
`VideoPanopticScorer` fed online from the channel plane, against `score_directory` on the tree that run wrote.  The chain
is: reference == offline (tests/test_panoptic_quality_cpu.py, on the golden), offline == online (here).  With
DEVA_TEST_DRYRUN=1 the same code runs on the CPU contract."""
import json
import os

import numpy as np
import pytest
import torch

import emu_frame_result as EF
import emu_panoptic as EP
import panoptic_case as PC
from deva.hip import metrics
from gpu_util import dev
from test_gpu_i_drivers import network  # noqa: F401  (the drivers' way to the network, a fixture)
from test_panoptic_quality_cpu import _same

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DRYRUN = os.environ.get('DEVA_TEST_DRYRUN') == '1'
SIZES = [(1, 1), (7, 13), (33, 47), (270, 480)]


@pytest.fixture(autouse=True)
def _emulated_when_dry(monkeypatch):
    if DRYRUN:
        EF.install(monkeypatch)
        EP.install(monkeypatch)


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def narrow(pred):
    """a predicted id plane for the encodings that hold 24 / 31 bits: the ids outside become one unlisted id"""
    return np.where((pred < 0) | (pred >= 2**24), 16777214, pred)


def run(gt, gt_table, pred, pred_table, gt_enc, pred_enc, seed=0):
    """one call in the given encodings against the contract -> the table (numpy)"""
    h, w = gt.shape
    gt_arg = PC.rgb(gt) if gt_enc == 'rgb' else gt.astype(np.int32)
    lut = None
    if pred_enc == 'index':
        pred_arg, lut, stands_for = PC.channel_form(pred, pred_table, seed)
        want = EP.counts(gt_arg, gt_table, pred_arg, pred_lut=lut, n_pred=len(pred_table))
        assert np.array_equal(want, EP.counts(gt_arg, gt_table, stands_for, pred_table))    # the form stands for these ids
    else:
        pred_arg = {'rgb': lambda: PC.rgb(narrow(pred)), 'i32': lambda: narrow(pred).astype(np.int32),
                    'i64': lambda: pred.astype(np.int64)}[pred_enc]()
        want = EP.counts(gt_arg, gt_table, pred_arg, pred_table)
    got = metrics.panoptic_counts(up(gt_arg), gt_table, up(pred_arg), len(pred_table) if lut is not None else pred_table,
                                  None if lut is None else up(lut))
    assert got.dtype == torch.uint32 and tuple(got.shape) == (len(gt_table) + 2, len(pred_table) + 2)
    got = got.cpu().numpy()
    assert int(got.sum(dtype=np.int64)) == h * w
    assert np.array_equal(got, want), (np.argwhere(got != want)[:5], got[got != want][:5], want[got != want][:5])
    return got


@pytest.fixture(scope='module')
def small_cases():
    return {size: PC.planes(size[0], size[1], 5, 7, 100 + size[0]) for size in SIZES}


@pytest.mark.parametrize('pred_enc', ['rgb', 'i32', 'i64', 'index'])
@pytest.mark.parametrize('gt_enc', ['rgb', 'i32'])
@pytest.mark.parametrize('size', SIZES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_every_encoding_pair_is_bit_identical(size, gt_enc, pred_enc, small_cases):
    """33 x 47 and 7 x 13: odd widths, every RGB row starts off a 16-byte boundary and the last strip is cut;
    270 x 480: 32 workgroups"""
    gt, gt_table, pred, pred_table = small_cases[size]
    first = run(gt, gt_table, pred, pred_table, gt_enc, pred_enc, seed=size[0])
    if size == (33, 47):     # called twice: the same bytes (the table is initialised by the call)
        assert np.array_equal(first, run(gt, gt_table, pred, pred_table, gt_enc, pred_enc, seed=size[0]))


@pytest.mark.parametrize('n_gt,n_pred', [(0, 0), (1, 1), (0, 1022), (1022, 1), (1022, 1022)])
def test_table_lengths(n_gt, n_pred):
    gt, gt_table, pred, pred_table = PC.planes(64, 96, n_gt, n_pred, 7)
    assert metrics.panoptic_plan(64, 96, n_gt, n_pred).path == ('global' if n_gt * n_pred > 1022 else 'lds')
    got = run(gt, gt_table, pred, pred_table, 'rgb', 'i64')
    if n_gt == 1022:
        assert (got[302:].sum(axis=1) > 0).all()        # the ids beyond the first 300 were each given a pixel: all found
    run(gt, gt_table, pred, pred_table, 'i32', 'index')


@pytest.mark.parametrize('size', [(33, 47), (270, 480)], ids=lambda s: f'{s[0]}x{s[1]}')
def test_at_and_above_the_lds_limit(size):
    """the last table that is counted in LDS and the first that goes to the global table directly"""
    n_gt = 100
    n = max(k for k in range(1, 1023) if metrics.panoptic_plan(size[0], size[1], n_gt, k).path == 'lds')
    at, over = metrics.panoptic_plan(size[0], size[1], n_gt, n), metrics.panoptic_plan(size[0], size[1], n_gt, n + 1)
    assert at.path == 'lds' and metrics.LDS_LIMIT - 4 * (n_gt + 3) < at.lds_bytes <= metrics.LDS_LIMIT and over.path == 'global'
    for n_pred in (n, n + 1):
        gt, gt_table, pred, pred_table = PC.planes(size[0], size[1], n_gt, n_pred, 11)
        run(gt, gt_table, pred, pred_table, 'i32', 'i64')
        run(gt, gt_table, pred, pred_table, 'rgb', 'index')


@pytest.mark.parametrize('gt_enc,pred_enc', [('rgb', 'index'), ('i32', 'i64'), ('rgb', 'rgb')])
def test_degenerate_planes(gt_enc, pred_enc):
    h, w = 270, 480
    gt_table, pred_table = PC.id_pool(5, 1), PC.id_pool(7, 2)
    # a constant plane: every add lands on one bin
    got = run(np.full((h, w), gt_table[3], dtype=np.int32), gt_table, np.full((h, w), pred_table[6]), pred_table, gt_enc, pred_enc)
    assert got[5, 8] >= h * w * 0.98 and np.count_nonzero(got) <= 2      # (the channel form strays 1 % to slot 1)
    # a one-pixel checkerboard: no run ever merges
    yy, xx = np.mgrid[0:h, 0:w]
    board = (yy + xx) % 2
    run(np.where(board, gt_table[0], gt_table[4]).astype(np.int32), gt_table, np.where(board, pred_table[1], 0), pred_table,
        gt_enc, pred_enc)
    # only unlisted ids on both sides
    got = run(np.where(board, 5555555, 6666).astype(np.int32), gt_table, np.where(xx % 3 == 0, 777777, 8888), pred_table,
              gt_enc, pred_enc)
    assert got[1, 1] == h * w


def test_channel_table_with_shared_and_out_of_range_entries():
    h, w = 33, 47
    rng = np.random.default_rng(3)
    gt = rng.integers(0, 4, size=(h, w)).astype(np.int32)
    index = rng.integers(-2, 12, size=(h, w)).astype(np.int16)           # channels -2 .. 11 of a table of 9
    lut = np.array([0, 2, 3, 3, 2, 1, 4, 5, 65535], dtype=np.uint16)     # shared slots 2 and 3; 5 = P and 65535: slot 1
    want = EP.counts(gt, [1, 2, 3], index, pred_lut=lut, n_pred=3)
    assert want[:, 1].sum() == int(((index < 0) | (index >= 9) | np.isin(index, (5, 7, 8))).sum())
    got = metrics.panoptic_counts(up(gt), [1, 2, 3], up(index), 3, up(lut)).cpu().numpy()
    assert np.array_equal(got, want) and got.sum() == h * w
    out = torch.full((5, 5), 7, dtype=torch.int32, device=dev()).view(torch.uint32)      # a preallocated, dirty table
    assert metrics.panoptic_counts(up(gt), [1, 2, 3], up(index), 3, up(lut), out=out) is out
    assert np.array_equal(out.cpu().numpy(), want)


@pytest.mark.parametrize('size', [(720, 1280), (1080, 1920)], ids=lambda s: f'{s[0]}x{s[1]}')
def test_full_frames_against_bincount(size):
    """40 x 40 segments at the VIPSeg 720P size and at 1080p, RGB ground truth: against np.bincount of the slot pairs"""
    h, w = size
    gt, gt_table, pred, pred_table = PC.planes(h, w, 40, 40, 5)
    pred = narrow(pred)

    def slots(plane, table):
        at = np.clip(np.searchsorted(table, plane), 0, len(table) - 1)
        return np.where(plane == 0, 0, np.where(table[at] == plane, at + 2, 1))
    want = np.bincount((slots(gt.astype(np.int64), gt_table) * 42 + slots(pred, pred_table)).reshape(-1), minlength=42 * 42)
    want = want.reshape(42, 42).astype(np.uint32)
    index, lut, stands_for = PC.channel_form(pred, pred_table, 9)
    want_fast = np.bincount((slots(gt.astype(np.int64), gt_table) * 42 + slots(stands_for, pred_table)).reshape(-1),
                            minlength=42 * 42).reshape(42, 42).astype(np.uint32)
    gt_rgb = up(PC.rgb(gt))
    got = metrics.panoptic_counts(gt_rgb, gt_table, up(PC.rgb(pred)), pred_table).cpu().numpy()
    fast = metrics.panoptic_counts(gt_rgb, gt_table, up(index), 40, up(lut)).cpu().numpy()
    assert np.array_equal(got, want) and np.array_equal(fast, want_fast) and got.sum() == h * w == fast.sum()


# ------------------------------------------------------------------------------------------ end to end
def test_online_scorer_on_the_semionline_clip_equals_score_directory(network, tmp_path, monkeypatch):  # noqa: F811
    from deva.inference.frame_results import FrameResultSaver
    from deva.inference.inference_core import DEVAInferenceCore
    from deva.inference.object_info import ObjectInfo
    from deva.inference.panoptic_quality import StuffMerger, VideoPanopticScorer, score_directory
    import driver_loops
    net, config, _ = network
    frames, dets = driver_loops.semionline_clip()
    gt_planes, gt_infos = PC.ground_truth(dets)
    gt_dev = [up(p) for p in gt_planes]
    cfg = dict(config, mem_every=2, max_missed_detection_count=2, max_num_objects=-1, num_voting_frames=3)
    scorer = VideoPanopticScorer(PC.CATEGORIES)
    scorer.start_video('clip')
    fed = []

    def hook(name, result, annotation):      # the saver's worker: the frame's files are written, its planes still on the device
        t = int(name[:-4])
        assert result.index is not None and result.index.dtype == torch.int16 and len(result.channel_ids) >= 1
        scorer.add_frame(result, annotation['segments_info'], gt_dev[t], gt_infos[t])
        fed.append(t)

    saver = {}

    def save(processor, prob, name):
        if not saver:
            saver['s'] = FrameResultSaver(str(tmp_path), 'clip', dataset='vipseg', object_manager=processor.object_manager,
                                          id_postprocessor=StuffMerger({c['id']: c['isthing'] == 1 for c in PC.CATEGORIES}),
                                          frame_hook=hook)
        saver['s'].save_mask(prob, name)

    PC.semionline_with_saver(lambda c: DEVAInferenceCore(net, config=c), cfg, frames, dets, lambda **kw: ObjectInfo(**kw), save,
                             num_voting_frames=3, detection_every=5, device=dev())
    saver['s'].end()
    assert fed == list(range(frames.shape[0]))
    scorer.end_video()
    online = scorer.result()
    with open(tmp_path / 'pred.json', 'w') as f:
        json.dump({'annotations': [saver['s'].video_json]}, f)
    truth, gt_json = PC.write_truth(str(tmp_path), 'clip', gt_planes, gt_infos)
    offline = score_directory(str(tmp_path), truth, gt_json)
    assert _same(online, offline)
    assert sorted(f for f in os.listdir(tmp_path) if f.endswith('.txt')) == sorted(scorer.texts())
    for name, text in scorer.texts().items():
        with open(tmp_path / name) as f:
            assert f.read() == text, name
    # the run scored something: the thing and the stuff box are found in every window
    for k in scorer.windows:
        per_class = online['vpq'][k]['per_class']
        assert per_class[2]['tp'] + per_class[2]['fn'] > 0 and per_class[5]['tp'] + per_class[5]['fn'] > 0
    assert online['stq']['Length_per_seq'] == [frames.shape[0]]
