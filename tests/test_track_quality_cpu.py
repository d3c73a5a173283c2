"""`deva.inference.track_quality` without a GPU: the rules T1-T9 by hand on a clip of two frames, the scorer against the
statement of tests/track_case.py (brute-force assignment) on random small clips, the assignment against brute force and
against scipy, the groups, the BURST files and `merge_burst_predictions`.  The mask overlaps come from the CPU contract of
the overlap library (tests/emu_overlap.py)."""
import itertools
import json
import math
import os

import numpy as np
import pytest
import torch

import emu_overlap as EO
import rle_case as LC
import track_case as TC
from deva.inference import track_quality as TQ

torch.set_grad_enabled(False)


@pytest.fixture(autouse=True)
def _emulated(monkeypatch):
    EO.install(monkeypatch)


def rles_of(masks):
    return {k: {'size': list(m.shape), 'counts': LC.counts_of(m)} for k, m in masks.items()}


def feed(scorer, name, clip, categories=None):
    scorer.start_video(name, categories)
    for gt, pred in clip:
        scorer.add_frame(rles_of(pred), rles_of(gt))
    return scorer.end_video()


def same(got, want, tol=1e-12):
    for f in ('HOTA_TP', 'HOTA_FN', 'HOTA_FP'):
        assert got[f].tolist() == list(want[f]), f
    for f in TC.FIELDS:
        assert np.abs(np.asarray(got[f]) - np.asarray(want[f])).max() <= tol, f
        assert abs(got['summary'][f] - want['summary'][f]) <= tol, f


def _row(*spans, n=10):
    p = np.zeros((1, n), dtype=bool)
    for lo, hi in spans:
        p[0, lo:hi] = True
    return p


# ------------------------------------------------------------------------------------------ by hand
def test_t_rules_by_hand_on_two_frames_two_gt_tracks_three_predicted_tracks():
    """masks on a 1 x 10 row.  frame 0: A = [0,4), B = [6,10) against 1 = [0,4), 2 = [6,8), 3 = [4,6): sim(A,1) = 1,
    sim(B,2) = 1/2; frame 1: A = [0,4) against 1 = [0,2), 2 = [3,4): sim 1/2 and 1/4.
    T2: counts A 2, B 1; 1: 2, 2: 2, 3: 1.  T3: pmc(A,1) = 1 + (1/2)/(3/4) = 5/3, pmc(A,2) = 1/3, pmc(B,2) = 1.
    T4: A(A,1) = (5/3)/(7/3) = 5/7, A(A,2) = 1/11, A(B,2) = 1/2.  T5: A-1 and B-2 on frame 0, A-1 on frame 1.
    T6: alpha <= 0.5: TP 3, FN 0, FP 2, mc(A,1) = 2, mc(B,2) = 1; above: TP 1 (A-1 on frame 0), FN 2, FP 4."""
    clip = [({'A': _row((0, 4)), 'B': _row((6, 10))}, {'1': _row((0, 4)), '2': _row((6, 8)), '3': _row((4, 6))}),
            ({'A': _row((0, 4))}, {'1': _row((0, 2)), '2': _row((3, 4))})]
    sims = TC.sims_of(clip)
    assert sims[0][2] == [[1.0, 0.0, 0.0], [0.0, 0.5, 0.0]] and sims[1][2] == [[0.5, 0.25]]
    scorer = TQ.TrackQualityScorer(device='cpu')
    rec = feed(scorer, 'hand', clip)['all']
    low, high = slice(0, 10), slice(10, 19)
    assert len(TQ.ALPHAS) == 19 and abs(TQ.ALPHAS[9] - 0.5) < 1e-15 and abs(TQ.ALPHAS[18] - 0.95) < 1e-15
    assert rec['HOTA_TP'].tolist() == [3] * 10 + [1] * 9 and rec['HOTA_FN'].tolist() == [0] * 10 + [2] * 9
    assert rec['HOTA_FP'].tolist() == [2] * 10 + [4] * 9
    for f, lo, hi in (('AssA', 5 / 6, 1 / 3), ('AssRe', 1.0, 1 / 2), ('AssPr', 5 / 6, 1 / 2), ('LocA', 2 / 3, 1.0), ('DetA', 3 / 5, 1 / 7),
                      ('DetRe', 1.0, 1 / 3), ('DetPr', 3 / 5, 1 / 5), ('HOTA', math.sqrt(1 / 2), math.sqrt(1 / 21)),
                      ('OWTA', math.sqrt(5 / 6), 1 / 3)):
        assert np.allclose(rec[f][low], lo, rtol=0, atol=1e-15) and np.allclose(rec[f][high], hi, rtol=0, atol=1e-15), f
        assert abs(rec['summary'][f] - (10 * lo + 9 * hi) / 19) < 1e-15, f
    same(rec, TC.combined([TC.sequence(sims)]))
    assert (rec['gt_tracks'], rec['pred_tracks'], rec['gt_dets'], rec['pred_dets'], rec['frames']) == (2, 3, 3, 5, 2)
    whole = scorer.result()['all']
    same(whole, TC.combined([TC.sequence(sims)]))
    assert list(whole['sequences']) == ['hand']


def test_frames_without_ground_truth_or_prediction_count_fp_or_fn_only():
    clip = [({}, {'1': _row((0, 4)), '2': _row((5, 6))}), ({'A': _row((0, 4)), 'B': _row((5, 9))}, {}), ({}, {})]
    rec = feed(TQ.TrackQualityScorer(device='cpu'), 'gaps', clip)['all']
    assert rec['HOTA_TP'].tolist() == [0] * 19 and rec['HOTA_FP'].tolist() == [2] * 19 and rec['HOTA_FN'].tolist() == [2] * 19
    assert rec['summary']['HOTA'] == 0.0 and rec['summary']['LocA'] == 1.0
    same(rec, TC.combined([TC.sequence(TC.sims_of(clip))]))


# ------------------------------------------------------------------------------------------ against the statement
def test_the_scorer_equals_the_statement_on_random_small_clips():
    rng = np.random.default_rng(11)
    clips = {f'clip{k}': TC.random_clip(rng, n_gt=int(rng.integers(1, 4)), n_pred=int(rng.integers(1, 5))) for k in range(12)}
    scorer = TQ.TrackQualityScorer(device='cpu')
    for name, clip in clips.items():
        same(feed(scorer, name, clip)['all'], TC.combined([TC.sequence(TC.sims_of(clip))]))
    same(scorer.result()['all'], TC.score(clips)['all'])
    assert any(r['HOTA_TP'][0] > 0 for r in scorer.result()['all']['sequences'].values())


def test_groups_restrict_the_ground_truth_and_keep_every_prediction():
    clip = TC.synthetic_clip(h=24, w=32, frames=4, n_gt=3, n_pred=4, seed=2)
    categories = {'100': 7, '101': 8, '102': 7}
    groups = {'common': [7], 'uncommon': [8, 9], 'none': [1]}
    scorer = TQ.TrackQualityScorer(groups, device='cpu')
    feed(scorer, 'v', clip, categories)
    got, want = scorer.result(), TC.score({'v': clip}, groups, {'v': categories})
    for g in groups:
        same(got[g], want[g])
    assert got['none']['HOTA_TP'].tolist() == [0] * 19 and got['none']['HOTA_FP'][0] == sum(len(p) for _, p in clip)
    assert got['common']['gt_tracks'] == 2 and got['uncommon']['gt_tracks'] == 1 and got['common']['pred_tracks'] == 4
    with pytest.raises(ValueError, match='groups need the `track_category_ids`'):
        TQ.TrackQualityScorer(groups).start_video('w')
    assert 'not TrackEval' in TQ.__doc__ and "this project's rule" in TQ.__doc__


def test_the_scorer_is_fed_in_order():
    scorer = TQ.TrackQualityScorer(device='cpu')
    with pytest.raises(ValueError, match='no video has been started'):
        scorer.add_frame({}, {})
    with pytest.raises(ValueError, match='no video has been started'):
        scorer.end_video()
    scorer.start_video('a')
    with pytest.raises(ValueError, match="video 'a' has not been ended"):
        scorer.start_video('b')
    with pytest.raises(ValueError, match="video 'a' has not been ended"):
        scorer.result()
    scorer.end_video()
    with pytest.raises(ValueError, match='scored already'):
        scorer.start_video('a')


# ------------------------------------------------------------------------------------------ the assignment
def _brute(score):
    pairs = TC.best_pairs(score.tolist())
    return sum(score[r, c] for r, c in pairs)


def test_the_assignment_against_brute_force():
    rng = np.random.default_rng(4)
    for _ in range(150):
        n_g, n_p = int(rng.integers(1, 6)), int(rng.integers(1, 6))
        score = rng.random((n_g, n_p)) * (rng.random((n_g, n_p)) < 0.7)
        rows, cols = TQ.assign_pairs(score)
        assert len(rows) == len(cols) == min(n_g, n_p) and len(set(rows)) == len(rows) and len(set(cols)) == len(cols)
        assert rows == sorted(rows) and abs(sum(score[r, c] for r, c in zip(rows, cols)) - _brute(score)) < 1e-12
    assert TQ.assign_pairs(np.zeros((0, 3))) == ([], []) and TQ.assign_pairs(np.zeros((3, 0))) == ([], [])
    assert TC.best_pairs([[1.0, 5.0], [2.0, 0.0], [9.0, 9.5]]) == [(0, 1), (2, 0)] and TQ.assign_pairs([[1.0, 5.0], [2.0, 0.0], [9.0, 9.5]]) == ([0, 2], [1, 0])


def test_the_assignment_against_scipy():
    optimize = pytest.importorskip('scipy.optimize')
    rng = np.random.default_rng(9)
    for _ in range(100):
        score = rng.random((int(rng.integers(1, 12)), int(rng.integers(1, 12))))
        rows, cols = TQ.assign_pairs(score)
        r, c = optimize.linear_sum_assignment(-score)
        assert abs(score[rows, cols].sum() - score[r, c].sum()) < 1e-12 and rows == r.tolist() and cols == c.tolist()


# ------------------------------------------------------------------------------------------ the files
def _burst_files(tmp_path, clips, categories):
    """a ground-truth file and a tree of pred.json files as the saver's `video_json`, from clips of planes"""
    sequences = []
    for name, clip in clips.items():
        dataset, seq_name = name.split('/')
        h, w = next(iter(clip[0][0].values())).shape
        frames = [{k: {'rle': LC.coco_string(LC.counts_of(m)), 'extra': 1} for k, m in gt.items()} for gt, _ in clip]
        sequences.append({'dataset': dataset, 'seq_name': seq_name, 'height': h, 'width': w, 'fps': 6, 'segmentations': frames,
                          'track_category_ids': categories[name], 'annotated_image_paths': [f'{t:05d}.jpg' for t in range(len(clip))]})
        video = {'dataset': dataset, 'seq_name': seq_name, 'segmentations': [
            {'file_name': f'{t:05d}.jpg', 'segmentations': [{'id': int(k), 'score': 0.5, 'rle': {'size': [h, w], 'counts': LC.coco_string(LC.counts_of(m))}}
                                                           for k, m in pred.items()]} for t, (_, pred) in enumerate(clip)]}
        os.makedirs(tmp_path / 'pred' / dataset / seq_name)
        (tmp_path / 'pred' / dataset / seq_name / 'pred.json').write_text(json.dumps(video))
    gt_file = {'sequences': sequences, 'split': 'val', 'category_names': {'7': 'x'}}
    (tmp_path / 'gt.json').write_text(json.dumps(gt_file))
    return gt_file


def test_merge_burst_predictions_and_score_burst_json_on_a_tree_of_two_sequences(tmp_path):
    clips = {'YFCC100M/v_1': TC.synthetic_clip(h=24, w=32, frames=4, n_gt=3, n_pred=4, seed=5),
             'AVA/clip_2': TC.synthetic_clip(h=20, w=28, frames=3, n_gt=2, n_pred=3, seed=6)}
    categories = {'YFCC100M/v_1': {'100': 7, '101': 8, '102': 7}, 'AVA/clip_2': {'100': 8, '101': 7}}
    gt_file = _burst_files(tmp_path, clips, categories)
    out = tmp_path / 'merged.json'
    merged = TQ.merge_burst_predictions(str(tmp_path / 'gt.json'), str(tmp_path / 'pred'), str(out))
    # the statement, from the script's lines: load the ground truth; per sequence empty its 'segmentations'; per frame of
    # <pred>/<dataset>/<seq_name>/pred.json a dict id -> {'rle': the counts text}; every id gets category 0; dump
    want = json.loads(json.dumps(gt_file))
    for seq in want['sequences']:
        video = json.load(open(tmp_path / 'pred' / seq['dataset'] / seq['seq_name'] / 'pred.json'))
        seq['segmentations'], ids = [], {}
        for frame in video['segmentations']:
            this = {}
            for entry in frame['segmentations']:
                this[entry['id']] = {'rle': entry['rle']['counts']}
                ids[entry['id']] = 0
            seq['segmentations'].append(this)
        seq['track_category_ids'] = ids
    assert out.read_text() == json.dumps(want) and merged == want
    on_disk = json.load(open(out))
    assert on_disk['split'] == 'val' and on_disk['sequences'][0]['fps'] == 6 and set(on_disk['sequences'][1]['track_category_ids'].values()) == {0}
    assert all(isinstance(k, str) for k in on_disk['sequences'][0]['segmentations'][0])
    # scoring the merged file against the ground truth
    got = TQ.score_burst_json(str(out), str(tmp_path / 'gt.json'), device='cpu')
    same(got['all'], TC.score(clips)['all'])
    assert list(got['all']['sequences']) == ['YFCC100M/v_1', 'AVA/clip_2']
    groups = {'common': [7], 'uncommon': [8]}
    got = TQ.score_burst_json(on_disk, gt_file, groups, device='cpu')
    want = TC.score(clips, groups, categories)
    for g in groups:
        same(got[g], want[g])
    short = json.loads(json.dumps(on_disk))
    short['sequences'][1]['segmentations'].pop()
    with pytest.raises(ValueError, match=r'sequence AVA/clip_2: 2 predicted frames, 3 in the ground truth'):
        TQ.score_burst_json(short, gt_file, device='cpu')
    del short['sequences'][0]
    with pytest.raises(ValueError, match=r'sequence YFCC100M/v_1: the prediction does not hold it'):
        TQ.score_burst_json(short, gt_file, device='cpu')
