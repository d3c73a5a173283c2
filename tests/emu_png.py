"""TEST-ONLY CPU contract of the two library calls of `deva.hip.png` (`_launch_deflate`, `_launch_place`), in the manner of
tests/emu_lowres.py: the numpy statement of tests/png_case.py behind the binding's own argument checks, minus the refusal
of host tensors.  `install(monkeypatch)` patches it over the ctypes wrappers.  The device must agree byte for byte.

The coded segments live in the library's scratch between the two calls; here the statement's stream is kept per scratch
tensor instead (by its address: the binding holds the tensor for as long as it may place again)."""
import numpy as np
import torch

import png_case as PC
from deva.hip import png as real

_STREAMS = {}


def _place(data, info4, out, capacity, info):
    total = len(data)
    room = min(total, capacity)
    if room:
        out[:room] = torch.from_numpy(np.frombuffer(data[:room], dtype=np.uint8).copy())
    info.copy_(torch.tensor([total, info4[1], int(total > capacity), info4[3]], dtype=torch.int64))


def _launch_deflate(plane, h, w, bpp, scratch, out, capacity, info):
    assert plane.numel() == h * w * bpp and scratch.numel() >= PC.plan(h, w, bpp)['scratch_bytes']
    data, info4 = PC.stream(plane.cpu().numpy().reshape(h, w * bpp))
    if len(_STREAMS) > 64:
        _STREAMS.clear()
    _STREAMS[scratch.data_ptr()] = (data, info4, (h, w, bpp))
    _place(data, info4, out, capacity, info)


def _launch_place(h, w, bpp, scratch, out, capacity, info):
    data, info4, geometry = _STREAMS[scratch.data_ptr()]
    assert geometry == (h, w, bpp)
    _place(data, info4, out, capacity, info)


def install(monkeypatch):
    for name in ('_launch_deflate', '_launch_place'):
        monkeypatch.setattr(real, name, globals()[name])
