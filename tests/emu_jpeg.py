"""TEST-ONLY CPU contract of the two library calls of `deva.hip.jpeg` (`_launch_scan`, `_launch_place`), in the manner of
tests/emu_png.py: the numpy statement of tests/jpeg_case.py behind the binding's own argument checks, minus the refusal of
host tensors.  `install(monkeypatch)` patches it over the ctypes wrappers.  The device must agree byte for byte.

The coded intervals live in the library's scratch between the two calls; here the statement's data is kept per scratch
tensor instead (by its address: the binding holds the tensor for as long as it may place again)."""
import numpy as np
import torch

import jpeg_case as JC
from deva.hip import jpeg as real

_SCANS = {}
_NAMES = {code: name for name, code in real.SUBSAMPLINGS.items()}


def _place(data, info4, out, capacity, info):
    total = len(data)
    room = min(total, capacity)
    if room:
        out[:room] = torch.from_numpy(np.frombuffer(data[:room], dtype=np.uint8).copy())
    info.copy_(torch.tensor([total, info4[1], int(total > capacity), info4[3]], dtype=torch.int64))


def _launch_scan(plane, h, w, quality, sub, restart, scratch, out, capacity, info):
    assert plane.numel() == h * w * 3 and scratch.numel() >= JC.plan(h, w, _NAMES[sub], restart)['scratch_bytes']
    data, info4 = JC.scan(plane.cpu().numpy().reshape(h, w, 3), quality, _NAMES[sub], restart)
    if len(_SCANS) > 64:
        _SCANS.clear()
    _SCANS[scratch.data_ptr()] = (data, info4, (h, w, sub, restart))
    _place(data, info4, out, capacity, info)


def _launch_place(h, w, sub, restart, scratch, out, capacity, info):
    data, info4, geometry = _SCANS[scratch.data_ptr()]
    assert geometry == (h, w, sub, restart)
    _place(data, info4, out, capacity, info)


def install(monkeypatch):
    for name in ('_launch_scan', '_launch_place'):
        monkeypatch.setattr(real, name, globals()[name])
