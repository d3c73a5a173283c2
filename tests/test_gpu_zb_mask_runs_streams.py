"""Do the launches and copies of `deva.hip.mask_runs.encode` go to the caller's stream?  The probe of tests/stream_probe.py
as tests/test_gpu_z_rle_streams.py uses it: the call runs on a side stream that is still blocked behind a delay kernel and
must be bit-identical to the default-stream run.  The probed buffer is the one the call reads: the planes are copied over
decoys (other valid planes) in stream order before the call and the decoys are put back after it, so a launch that left for
the null stream would encode the decoys.  The default form waits once, for the total: `before_wait` marks there, so
everything up to it (the count pass and its scans) was enqueued while the stream was blocked; the `capacity=` form does
not wait at all, and its `finish()` is called after the mark."""
import os

import numpy as np
import pytest
import torch

import emu_runs as ER
import runs_case as RC
import stream_probe as SP
from deva.hip import mask_runs

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DRYRUN = os.environ.get('DEVA_TEST_DRYRUN') == '1'
H, W = 33, 67
THRESHOLD = RC.THRESHOLDS[-1]


@pytest.fixture(autouse=True)
def _emulated_when_dry(monkeypatch):
    if DRYRUN:
        ER.install(monkeypatch)


def _as_tensors(records):
    """the records of `encode(form='counts', stats=True)` as what the probe compares: tensors and host scalars"""
    return [(torch.tensor(r['counts'], dtype=torch.int64), r['area'], str(r['bbox'])) for r in records]


@pytest.mark.parametrize('dtype', ['uint8', 'float32'])
@pytest.mark.parametrize('form', ['default', 'capacity'])
def test_encode_on_a_blocked_side_stream(form, dtype):
    if dtype == 'uint8':
        planes, threshold = RC.byte_stack(H, W)[1], None
        decoy = np.ascontiguousarray(planes[::-1, ::-1, ::-1])
    else:
        planes, threshold = RC.float_stack(H, W, THRESHOLD)[1], THRESHOLD
        decoy = np.ascontiguousarray(-planes[::-1, ::-1, ::-1])
        decoy[np.isnan(decoy)] = 3.0
    want = RC.records(planes, threshold, 'counts', stats=True)
    assert RC.records(decoy, threshold, 'counts', stats=True) != want
    total = RC.statement(planes, threshold)['total']

    def run(i, mark):
        if form == 'default':
            return _as_tensors(mask_runs.encode(i['planes'], threshold=threshold, form='counts', stats=True, before_wait=mark))
        pending = mask_runs.encode(i['planes'], threshold=threshold, form='counts', stats=True, capacity=total + 7)
        mark()
        return _as_tensors(pending.finish())
    got = SP.probe(run, dict(planes=torch.from_numpy(planes)), dict(planes=torch.from_numpy(decoy)), f'encode ({form}, {dtype})')
    # the default-stream run the probe compared with is the statement's
    flat = SP.flatten(_as_tensors(want))
    assert [p for p, _ in got] == [p for p, _ in flat]
    assert all(torch.equal(a, b) if isinstance(a, torch.Tensor) else a == b for (_, a), (_, b) in zip(got, flat))
