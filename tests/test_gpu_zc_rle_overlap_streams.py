"""Do the two launches and the two host-to-device copies of `deva.hip.rle.intersections` go to the caller's stream?  The
probe of tests/stream_probe.py as tests/test_gpu_z_rle_streams.py uses it: the call runs on a side stream that is still
blocked behind a delay kernel, and must be bit-identical to the default-stream run.  What the call reads on the device it
brings along itself (the run arrays and boxes), so the probed buffers are the ones it writes: the probe fills them with a
sentinel in stream order before the call and with decoys (the tables of the sides swapped round and mirrored: valid, and
different) after it.  A launch on the null stream would run ahead of the delay, and the sentinel would then be laid over
its output.  The `pending=True` form copies the tables to the host on the same stream; its `finish()` follows the mark."""
import os

import numpy as np
import pytest
import torch

import emu_overlap as EO
import overlap_case as OC
import stream_probe as SP
from deva.hip import rle

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DRYRUN = os.environ.get('DEVA_TEST_DRYRUN') == '1'
H, W = 33, 67


@pytest.fixture(autouse=True)
def _emulated_when_dry(monkeypatch):
    if DRYRUN:
        EO.install(monkeypatch)


@pytest.mark.parametrize('form', ['device', 'pending'])
def test_intersections_on_a_blocked_side_stream(form):
    dt, gt = OC.geometry_case(H, W)
    rles_d, rles_g = OC.as_rles(dt, H, W), OC.as_rles(gt, H, W)
    want = OC.statement(dt, gt, H, W)
    names = ('inter', 'area_d', 'area_g')
    real = {n: torch.full(t.shape, 7, dtype=torch.int32) for n, t in zip(names, want)}              # the sentinel
    decoy = {n: torch.from_numpy(np.ascontiguousarray(t[::-1] + 1).astype(np.int32)) for n, t in zip(names, want)}

    def run(i, mark):
        if form == 'device':
            return [t.clone() for t in rle.intersections(rles_d, rles_g, out=i)]                     # (the probe lays the decoys over `out` next)
        pending = rle.intersections(rles_d, rles_g, out=i, pending=True)
        mark()
        return [torch.from_numpy(t) for t in pending.finish()]
    got = SP.probe(run, real, decoy, f'intersections ({form})')
    # the default-stream run the probe compared with is the statement's
    assert len(got) == 3
    for (_, t), b in zip(got, want):
        assert np.array_equal(t.numpy().astype(np.int64), b)
