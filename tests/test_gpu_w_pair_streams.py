"""Does every launch of `pair_counts` go to the caller's stream?  The probe of tests/stream_probe.py as
tests/test_gpu_v_streams.py uses it: the call runs on a side stream that is still blocked behind a delay kernel while its
inputs hold decoys (a second valid case from another seed), and must be bit-identical to the default-stream run.  Both
clearing memsets and both kernels are behind the one stream argument; a launch on the null stream would read the decoys."""
import os

import numpy as np
import pytest
import torch

import emu_pairs as EP
import pair_case as PC
import stream_probe as SP
import vos_case as VC
from deva.hip import pair_metrics
from gpu_util import dev

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DRYRUN = os.environ.get('DEVA_TEST_DRYRUN') == '1'


@pytest.fixture(autouse=True)
def _emulated_when_dry(monkeypatch):
    if DRYRUN:
        EP.install(monkeypatch)


def _inputs(seed):
    gt, pred, gt_ids, pred_ids = PC.case(29, 53, 4, 6, seed)
    return gt, pred, gt_ids, pred_ids


@pytest.mark.parametrize('form', ['planes', 'channel plane'])
def test_pair_counts_on_a_blocked_side_stream(form):
    (gt, pred, gt_ids, pred_ids), (gt2, pred2, _, _) = _inputs(5), _inputs(6)
    table_g = torch.from_numpy(gt_ids.astype(np.int32)).to(dev())
    table_p = torch.from_numpy(pred_ids.astype(np.int32)).to(dev())
    if form == 'planes':
        real = dict(gt=torch.from_numpy(gt.astype(np.int32)), pred=torch.from_numpy(pred))
        decoy = dict(gt=torch.from_numpy(gt2.astype(np.int32)), pred=torch.from_numpy(pred2))

        def run(i, mark):
            return pair_metrics.pair_counts(i['gt'], i['pred'], table_g, table_p, radius=4, validate=False)
    else:
        index, lut, _ = VC.channel_form(pred, pred_ids, 1)
        index2, _, _ = VC.channel_form(pred2, pred_ids, 2)
        lut_d = torch.from_numpy(lut).to(dev())
        real = dict(gt=torch.from_numpy(gt.astype(np.uint8)), pred=torch.from_numpy(index))
        decoy = dict(gt=torch.from_numpy(gt2.astype(np.uint8)), pred=torch.from_numpy(index2))

        def run(i, mark):
            return pair_metrics.pair_counts(i['gt'], i['pred'], table_g, len(pred_ids), radius=2, pred_lut=lut_d, validate=False)
    want = SP.probe(run, real, decoy, f'pair_counts ({form})')
    # the default-stream run the probe compared with is the statement's
    listed = np.where(np.isin(pred, pred_ids), pred, 0)
    singles, pairs = PC.counts(gt, listed, gt_ids, pred_ids, 4 if form == 'planes' else 2)
    assert [path for path, _ in want] == ['out[0]', 'out[1]']
    assert np.array_equal(want[0][1].numpy(), singles) and np.array_equal(want[1][1].numpy(), pairs)
