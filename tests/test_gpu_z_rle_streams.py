"""Do the launch and the one host-to-device copy of `deva.hip.rle.decode` go to the caller's stream?  The probe of
tests/stream_probe.py as tests/test_gpu_y_region_streams.py uses it: the call runs on a side stream that is still blocked
behind a delay kernel, and must be bit-identical to the default-stream run.  What the call reads on the device it brings
along itself (the run array), so the probed buffer is the one it writes: the probe fills it with a sentinel in stream order
before the call and with decoys (the mirrored planes: valid, and different everywhere that matters) after it.  A launch
on the null stream would run ahead of the delay, and the sentinel would then be laid over its output."""
import os

import numpy as np
import pytest
import torch

import emu_rle as EL
import rle_case as LC
import stream_probe as SP
from deva.hip import rle

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DRYRUN = os.environ.get('DEVA_TEST_DRYRUN') == '1'
H, W = 33, 67


@pytest.fixture(autouse=True)
def _emulated_when_dry(monkeypatch):
    if DRYRUN:
        EL.install(monkeypatch)


@pytest.mark.parametrize('dtype', [torch.uint8, torch.float32], ids=['uint8', 'float32'])
@pytest.mark.parametrize('size', [None, (48, 95)], ids=['straight', 'resized'])
def test_decode_on_a_blocked_side_stream(size, dtype):
    names, all_counts = LC.row(H, W)
    rles = LC.as_rles(all_counts, H, W)
    want = LC.decoded(all_counts, H, W, size)
    decoy = torch.from_numpy(np.ascontiguousarray(want[::-1, :, ::-1])).to(dtype)
    sentinel = torch.full(want.shape, 7, dtype=dtype)

    def run(i, mark):
        return rle.decode(rles, size, dtype=dtype, out=i['out']).clone()        # (the probe lays the decoys over `out` next)
    got = SP.probe(run, dict(out=sentinel), dict(out=decoy), f'decode ({size}, {dtype})')
    # the default-stream run the probe compared with is the statement's
    assert [path for path, _ in got] == ['out']
    assert got[0][1].dtype == dtype and np.array_equal(got[0][1].numpy(), want.astype(got[0][1].numpy().dtype))
