"""Do the launches of `deva.hip.jpeg` go to the caller's stream?  The probe of tests/stream_probe.py as
tests/test_gpu_zg_png_streams.py uses it: the call runs on a side stream that is still blocked behind a delay kernel and
must be bit-identical to the default-stream run.  The probed buffer is the plane the call reads: it is copied over a
decoy (another picture of the same shape) in stream order before the call and the decoy is put back after it, so a
launch that left for the null stream would code the decoy.  `capacity=` keeps the call from waiting; its pinned copies
and the overflow's second placement are part of what is compared.  The control at the end shows that the probe sees a
misrouted launch."""
import os

import numpy as np
import pytest
import torch

import emu_jpeg as EJPEG
import jpeg_case as JC
import stream_probe as SP
from deva.hip import jpeg, ops

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DRYRUN = os.environ.get('DEVA_TEST_DRYRUN') == '1'
needs_streams = pytest.mark.skipif(DRYRUN, reason='needs real streams: nothing to observe on the emulated ops')
SIZE = (72, 1100)        # five intervals at 4:2:0 of 414 blocks: two steps each; nine at 4:4:4


@pytest.fixture(autouse=True)
def _emulated_when_dry(monkeypatch):
    if DRYRUN:
        EJPEG.install(monkeypatch)


def _inputs(seed):
    return dict(plane=torch.from_numpy(JC.overlay(*SIZE, seed=seed)))


def _as_tensor(data: bytes) -> torch.Tensor:
    return torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy())


def _encode(capacity, **parameters):
    def run(i, mark):
        pending = jpeg.encode(i['plane'], capacity=capacity, **parameters)
        mark()                                                              # `finish` waits for its copies
        return _as_tensor(pending.finish()), pending.total, pending.overflowed
    return run


@pytest.mark.parametrize('subsampling', ['4:2:0', '4:4:4'])
def test_encode_on_a_blocked_side_stream(subsampling):
    want = SP.probe(_encode(1 << 16, subsampling=subsampling), _inputs(91), _inputs(92), f'jpeg.encode {subsampling}')
    data = dict(want)['out[0]'].numpy().tobytes()
    assert data == JC.encode(_inputs(91)['plane'].numpy(), 75, subsampling, 0)


def test_an_overflowing_encode_on_a_blocked_side_stream():
    """the first copy is cut at 100 bytes; `finish` places the intervals again from the scratch the side stream filled"""
    want = SP.probe(_encode(100, quality=90, restart=7), _inputs(93), _inputs(94), 'jpeg.encode over capacity')
    assert dict(want)['out[2]'] is True


def test_scan_with_the_stream_argument_on_a_blocked_side_stream():
    """`stream=`: the launches go to the stream that is passed, here the probe's own (the current one)"""
    def run(i, mark):
        pending = jpeg.scan(i['plane'], capacity=1 << 16, stream=torch.cuda.current_stream() if not DRYRUN else None)
        mark()
        return _as_tensor(pending.finish()), pending.blocks
    SP.probe(run, _inputs(95), _inputs(96), 'jpeg.scan stream=')


@needs_streams
def test_control_a_launch_on_the_null_stream_is_reported(monkeypatch):
    """the same call with a null stream handle inside the side-stream context: it cannot wait for the delay, codes the
    decoy, and the probe must say so (and say nothing when the handle is the caller's stream)"""
    SP.probe(_encode(1 << 16), _inputs(97), _inputs(98), 'control: encode on the current stream')
    monkeypatch.setattr(jpeg, '_stream', lambda device=None: None)
    with pytest.raises(SP.Mismatch) as caught:
        SP.probe(_encode(1 << 16), _inputs(97), _inputs(98), 'control: encode on the null stream')
    print('caught:', caught.value)
    monkeypatch.setattr(jpeg, '_stream', ops._stream)
