"""`deva.inference.track_quality` on the device: a synthetic clip of 6 frames at 96 x 128 with 4 ground-truth and 5
predicted tracks, its masks encoded on the device (`rle.encode`) and scored through `TrackQualityScorer` (one
`rle.intersections` a frame, queued without a wait), against the statement of tests/track_case.py: every count equal and
every float within 1e-12 (the same fp64 arithmetic on the same integers; the sums may be taken in another order).
`score_burst_json` on files written from that clip gives the same record.  With DEVA_TEST_DRYRUN=1 the same code runs on
the CPU contracts (tests/emu_runs.py, tests/emu_overlap.py)."""
import json
import os

import numpy as np
import pytest
import torch

import emu_overlap as EO
import emu_runs as ER
import track_case as TC
from deva.hip import rle
from deva.inference import track_quality as TQ
from gpu_util import dev

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DRYRUN = os.environ.get('DEVA_TEST_DRYRUN') == '1'
TOL = 1e-12


@pytest.fixture(autouse=True)
def _emulated_when_dry(monkeypatch):
    if DRYRUN:
        EO.install(monkeypatch)
        ER.install(monkeypatch)


@pytest.fixture(scope='module')
def clip():
    """the clip and the statement's record, computed once"""
    c = TC.synthetic_clip(96, 128, frames=6, n_gt=4, n_pred=5, seed=0)
    assert len(c) == 6 and len({g for gt, _ in c for g in gt}) == 4 and len({p for _, pred in c for p in pred}) == 5
    return c, TC.score({'clip': c})['all']


def encoded(masks):
    """{id: bool plane} -> {id: {'size', 'counts'}} through the device encoder"""
    if not masks:
        return {}
    planes = torch.from_numpy(np.stack(list(masks.values()))).to(dev())
    return dict(zip(masks, rle.encode(planes)))


def same(got, want):
    for f in ('HOTA_TP', 'HOTA_FN', 'HOTA_FP'):
        assert got[f].tolist() == list(want[f]), f
    for f in TC.FIELDS:
        assert np.abs(np.asarray(got[f]) - np.asarray(want[f])).max() <= TOL, f
        assert abs(got['summary'][f] - want['summary'][f]) <= TOL, f


def test_the_scorer_on_the_synthetic_clip(clip):
    frames, want = clip
    assert want['HOTA_TP'][0] > 0 and want['HOTA_FN'][-1] > 0 and want['HOTA_FP'][0] > 0 and 0.05 < want['summary']['HOTA'] < 0.95
    scorer = TQ.TrackQualityScorer(device=dev())
    scorer.start_video('clip')
    for gt, pred in frames:
        scorer.add_frame(encoded(pred), encoded(gt))
    same(scorer.end_video()['all'], want)
    same(scorer.result()['all'], want)


def test_score_burst_json_on_files_written_from_the_clip(clip, tmp_path):
    frames, want = clip
    sides = []
    for which in (0, 1):
        segs = [{k: {'rle': r['counts']} for k, r in encoded(frame[which]).items()} for frame in frames]
        sides.append({'sequences': [{'dataset': 'SYN', 'seq_name': 'clip', 'height': 96, 'width': 128, 'segmentations': segs,
                                     'track_category_ids': {k: 1 for frame in frames for k in frame[which]}}]})
    gt_path, pred_path = tmp_path / 'gt.json', tmp_path / 'pred.json'
    gt_path.write_text(json.dumps(sides[0]))
    pred_path.write_text(json.dumps(sides[1]))
    got = TQ.score_burst_json(str(pred_path), str(gt_path), device=dev())
    same(got['all'], want)
    same(got['all']['sequences']['SYN/clip'], want)
    grouped = TQ.score_burst_json(str(pred_path), str(gt_path), {'common': [1], 'uncommon': [2]}, device=dev())
    same(grouped['common'], want)
    assert grouped['uncommon']['HOTA_TP'].tolist() == [0] * 19
