"""Do the launches of `deva.hip.png` go to the caller's stream?  The probe of tests/stream_probe.py as
tests/test_gpu_zf_lowres_streams.py uses it: the call runs on a side stream that is still blocked behind a delay kernel
and must be bit-identical to the default-stream run.  The probed buffer is the plane the call reads: it is copied over a
decoy (another valid id map of the same shape) in stream order before the call and the decoy is put back after it, so a
launch that left for the null stream would code the decoy.  `capacity=` keeps the call from waiting; its pinned copies
and the overflow's second placement are part of what is compared.  The control at the end shows that the probe sees a
misrouted launch."""
import os

import numpy as np
import pytest
import torch

import emu_png as EPNG
import png_case as PC
import stream_probe as SP
from deva.hip import ops, png

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DRYRUN = os.environ.get('DEVA_TEST_DRYRUN') == '1'
needs_streams = pytest.mark.skipif(DRYRUN, reason='needs real streams: nothing to observe on the emulated ops')
SIZE = (40, 1100)        # five segments, two steps a row


@pytest.fixture(autouse=True)
def _emulated_when_dry(monkeypatch):
    if DRYRUN:
        EPNG.install(monkeypatch)


def _inputs(seed, rgb=False):
    return dict(plane=torch.from_numpy(PC.blobs(*SIZE, objects=5, seed=seed, rgb=rgb)))


def _as_tensor(data: bytes) -> torch.Tensor:
    return torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy())


def _encode(capacity, palette=None):
    def run(i, mark):
        pending = png.encode(i['plane'], palette=palette, capacity=capacity)
        mark()                                                              # `finish` waits for its copies
        return _as_tensor(pending.finish()), pending.total, pending.overflowed
    return run


@pytest.mark.parametrize('rgb', [False, True])
def test_encode_on_a_blocked_side_stream(rgb):
    want = SP.probe(_encode(1 << 16, None if rgb else bytes(range(256)) * 3), _inputs(91, rgb), _inputs(92, rgb), f'png.encode rgb={rgb}')
    data = dict(want)['out[0]'].numpy().tobytes()
    assert data == png.file_bytes(PC.stream(_inputs(91, rgb)['plane'].numpy())[0], *SIZE, 3 if rgb else 1, None if rgb else bytes(range(256)) * 3)


def test_an_overflowing_encode_on_a_blocked_side_stream():
    """the first copy is cut at 100 bytes; `finish` places the segments again from the scratch the side stream filled"""
    want = SP.probe(_encode(100), _inputs(93), _inputs(94), 'png.encode over capacity')
    assert dict(want)['out[2]'] is True


def test_deflate_with_the_stream_argument_on_a_blocked_side_stream():
    """`stream=`: the launches go to the stream that is passed, here the probe's own (the current one)"""
    def run(i, mark):
        pending = png.deflate(i['plane'], capacity=1 << 16, stream=torch.cuda.current_stream() if not DRYRUN else None)
        mark()
        return _as_tensor(pending.finish()), pending.adler
    SP.probe(run, _inputs(95), _inputs(96), 'png.deflate stream=')


@needs_streams
def test_control_a_launch_on_the_null_stream_is_reported(monkeypatch):
    """the same call with a null stream handle inside the side-stream context: it cannot wait for the delay, codes the
    decoy, and the probe must say so (and say nothing when the handle is the caller's stream)"""
    SP.probe(_encode(1 << 16), _inputs(97), _inputs(98), 'control: encode on the current stream')
    monkeypatch.setattr(png, '_stream', lambda device=None: None)
    with pytest.raises(SP.Mismatch) as caught:
        SP.probe(_encode(1 << 16), _inputs(97), _inputs(98), 'control: encode on the null stream')
    print('caught:', caught.value)
    monkeypatch.setattr(png, '_stream', ops._stream)
