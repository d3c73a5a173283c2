"""TEST-ONLY CPU contract of the one library call of `deva.hip.rle_overlap` (`_launch`), in the manner of
tests/emu_runs.py: the numpy statement of tests/overlap_case.py behind the binding's own parsing, O2 checks, chunking and
host arithmetic, minus the refusal of host tensors.  `install(monkeypatch)` patches it over the ctypes wrapper.  Integers
only, so the device must agree exactly."""
import numpy as np
import torch

import overlap_case as OC
from deva.hip import rle_overlap as real


def counts_of_side(side):
    """the run array of a `_Side` (include/deva_rle.h) back to lists of counts"""
    words = side.host.numpy()[:side.words]
    first, starts = words[:side.n + 1], words[side.n + 1:]
    return [np.diff(starts[first[k]:first[k + 1]]).tolist() for k in range(side.n)]


def _launch(dt, gt, height, width, scratch, inter, area_d, area_g, stream):
    assert scratch.numel() * 4 >= real.overlap_scratch(gt.words, gt.n)
    want = OC.statement(counts_of_side(dt), counts_of_side(gt), height, width)
    inter.copy_(torch.from_numpy(want[0].astype(np.int32)))
    area_d.copy_(torch.from_numpy(want[1].astype(np.int32)))
    area_g.copy_(torch.from_numpy(want[2].astype(np.int32)))


def install(monkeypatch):
    monkeypatch.setattr(real, '_launch', _launch)
