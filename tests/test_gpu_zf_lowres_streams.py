"""Do the launches of `deva.hip.lowres` go to the caller's stream?  The probe of tests/stream_probe.py as
tests/test_gpu_ze_rle_text_streams.py uses it: each of the three streamed entry points runs on a side stream that is still
blocked behind a delay kernel and must be bit-identical to the default-stream run.  The probed buffers are the ones the call
reads: the inputs are copied over decoys (other valid logits and scores of the same shapes) in stream order before the
call and the decoys are put back after it, so a launch that left for the null stream would resize the decoys.  The
control at the end shows that the probe sees exactly that."""
import os

import numpy as np
import pytest
import torch

import emu_lowres as EL
import emu_proposals as EP
import lowres_case as LC
import stream_probe as SP
from deva.hip import lowres, ops
from deva.inference.proposals import ProposalFilter

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DRYRUN = os.environ.get('DEVA_TEST_DRYRUN') == '1'
needs_streams = pytest.mark.skipif(DRYRUN, reason='needs real streams: nothing to observe on the emulated ops')
LOW, M, INPUT = (16, 16), 64, (36, 64)
SIZES = [(33, 70), (5, 9)]       # the tile path and the point path


@pytest.fixture(autouse=True)
def _emulated_when_dry(monkeypatch):
    if DRYRUN:
        EP.install(monkeypatch)
        EL.install(monkeypatch)


def _inputs(seed, planes=12):
    return dict(low=torch.from_numpy(LC.logits(seed, planes, LOW)), iou=torch.from_numpy(LC.iou_preds(seed, planes)))


def _upsample(size):
    return lambda i, mark: lowres.upsample_logits(i['low'], INPUT, size, model_size=M)


@pytest.mark.parametrize('size', SIZES)
def test_upsample_on_a_blocked_side_stream(size):
    SP.probe(_upsample(size), _inputs(81), _inputs(82), f'upsample_logits {size}')


@pytest.mark.parametrize('size', SIZES)
def test_select_on_a_blocked_side_stream(size):
    def inputs(seed):
        i = _inputs(seed)
        return dict(low=i['low'].view(4, 3, *LOW), scores=torch.from_numpy(np.random.default_rng(seed).uniform(0, 1, (4, 3)).astype(np.float32)))
    assert not np.array_equal(LC.choice(inputs(83)['scores'].numpy()), LC.choice(inputs(84)['scores'].numpy()))

    def run(i, mark):
        return lowres.select_masks(i['low'], i['scores'], INPUT, size, model_size=M)
    SP.probe(run, inputs(83), inputs(84), f'select_masks {size}')


@pytest.mark.parametrize('size', SIZES)
def test_a_filtered_frame_on_a_blocked_side_stream(size):
    """begin, the three launches of `add_lowres` and the launches of `finish` up to its one wait"""
    flt = ProposalFilter(*size, capacity=32, stability_score_thresh=0.7)

    def run(i, mark):
        flt.reset()
        flt.add_lowres(i['low'], i['iou'], INPUT, model_size=M)
        state = flt._ready(None)
        mark()                                                          # `finish` waits for its copy of the result table
        found = flt.finish()
        return found.masks, found.iou_preds, found.stability, found.boxes, found.index, state.arena.clone()
    SP.probe(run, _inputs(85), _inputs(86), f'add_lowres {size}')


@needs_streams
def test_control_a_launch_on_the_null_stream_is_reported(monkeypatch):
    """the same call with a null stream handle inside the side-stream context: it cannot wait for the delay, resizes the
    decoys, and the probe must say so (and say nothing when the handle is the caller's stream)"""
    SP.probe(_upsample(SIZES[0]), _inputs(87), _inputs(88), 'control: upsample on the current stream')
    monkeypatch.setattr(lowres, '_stream', lambda device=None: None)
    with pytest.raises(SP.Mismatch) as caught:
        SP.probe(_upsample(SIZES[0]), _inputs(87), _inputs(88), 'control: upsample on the null stream')
    print('caught:', caught.value)
    monkeypatch.setattr(lowres, '_stream', ops._stream)
