"""TEST-ONLY CPU contract of the two library calls of `deva.hip.mask_runs` (`_launch_count`, `_launch_write`), in the manner
of tests/emu_rle.py: the numpy statement of tests/runs_case.py behind the binding's own argument checks, chunking, capacity
handling and host arithmetic, minus the refusal of host tensors.  `install(monkeypatch)` patches it over the ctypes
wrappers.  Integers only, so the device must agree exactly.

The scratch of a `count` is opaque to the caller; here it is left as it is and the boundaries wait in `_PENDING` under the
scratch's address until the `write` that follows."""
import numpy as np
import torch

import runs_case as RC
from deva.hip import mask_runs as real

_PENDING = {}


def _launch_count(planes, code, threshold, scratch, n_out, base, total, first, stats):
    host = planes.numpy()
    want = RC.statement(host, threshold if code == real.DTYPES[torch.float32] else None, 0 if first is None else int(first.reshape(-1)[0]))
    n_out.copy_(torch.from_numpy(want['n']))
    base.copy_(torch.from_numpy(want['base']))
    total.fill_(want['total'])
    if stats is not None:
        stats.copy_(torch.from_numpy(want['stats']))
    _PENDING[scratch.data_ptr()] = (want['bounds'], int(want['base'][0]) if len(want['base']) else 0)


def _launch_write(n, h, w, scratch, base, bounds, capacity):
    found, first = _PENDING.pop(scratch.data_ptr())
    room = max(0, min(int(capacity) - first, found.size))       # E5: nothing at or beyond the capacity
    if room:
        bounds[first:first + room] = torch.from_numpy(found[:room])


def install(monkeypatch):
    monkeypatch.setattr(real, '_launch_count', _launch_count)
    monkeypatch.setattr(real, '_launch_write', _launch_write)
