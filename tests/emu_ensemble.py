"""TEST-ONLY CPU contracts of the three test-time-ensemble ops of `deva.hip.ops` (`scores_u8`, `ensemble_index_mask`,
`flip_w`), in the manner of tests/emu_ops.py: plain PyTorch, the executable statement of what each HIP kernel must
compute.  `install(monkeypatch)` patches them over the ctypes wrappers (next to `emu_ops.install`)."""
import torch
import torch.nn.functional as F

import emu_ops
from deva.hip import ops as real

MAX_VARIANTS = 8


def _resized(prob, size, flip):
    """eval_vos.py:170-177: bilinear resize (align_corners=False) when the size differs, then the flip back"""
    if size is not None and tuple(size) != tuple(prob.shape[-2:]):
        prob = F.interpolate(prob.unsqueeze(1), tuple(size), mode='bilinear', align_corners=False)[:, 0]
    return torch.flip(prob, dims=[-1]) if flip else prob


def scores_u8(prob, size=None, flip=False):
    """eval_vos.py:188-189: (prob * 255).astype(np.uint8) -- truncation (probabilities lie in [0, 1])"""
    return (_resized(prob.float(), size, flip) * 255).clamp(0, 255).to(torch.uint8)


def ensemble_index_mask(probs, size, flips, lut=None, quantize=True):
    """merge_multi_scale.py:44-66: sum over the runs (of the uint8 scores, or of the fp32 resized values in variant
    order), first-maximum argmax over channels, id table"""
    probs, flips = list(probs), list(flips)
    if len(probs) != len(flips) or not 1 <= len(probs) <= MAX_VARIANTS:
        raise real.DevaHipError(f'ensemble_index_mask: 1 to {MAX_VARIANTS} variants with one flip flag each')
    if any(p.shape[0] != probs[0].shape[0] for p in probs):
        raise real.DevaHipError('deva_ensemble_index_mask failed: variants differ in their number of channels')
    if quantize:
        total = sum(scores_u8(p, size, f).to(torch.int32) for p, f in zip(probs, flips))
    else:
        total = _resized(probs[0].float(), size, flips[0])
        for p, f in zip(probs[1:], flips[1:]):
            total = total + _resized(p.float(), size, f)
    idx = torch.argmax(total, dim=0)
    return idx if lut is None else emu_ops.lut_remap(idx, lut)


def flip_w(x):
    """torch.flip along W: the last dimension, or dimension 1 of a uint8 [H,W,3] frame"""
    if x.dtype == torch.uint8 and x.dim() == 3 and x.shape[2] == 3:
        return torch.flip(x, dims=[1])
    return torch.flip(x, dims=[-1])


def install(monkeypatch):
    for name in ('scores_u8', 'ensemble_index_mask', 'flip_w'):
        monkeypatch.setattr(real, name, globals()[name])
