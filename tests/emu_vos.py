"""TEST-ONLY CPU contract of the DAVIS counts (`deva.hip.vos_metrics.boundary_counts`), in the manner of
tests/emu_panoptic.py: the numpy statement of tests/vos_case.py behind the binding's own argument checks, minus the refusal
of host tensors.  `install(monkeypatch)` patches it over the ctypes wrapper.  Integers only, so the device must agree bit
for bit."""
import numpy as np
import torch

import vos_case as VC
from deva.hip import vos_metrics as real


def _np(t):
    if t is None:
        return None
    return t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def boundary_counts(gt, pred, ids, *, bound_th=0.008, radius=None, pred_lut=None, binary=False, scratch=None, out=None,
                    validate=True):
    _, size = real._plane(gt, 'gt', real._GT_ENC)
    pred_enc, psize = real._plane(pred, 'pred', real._PRED_ENC)
    if size != psize:
        raise real.DevaHipError(f'boundary_counts: gt is {size} and pred {psize}')
    gt_binary, pred_binary = real._sides(binary)
    if (pred_enc == real.INDEX16) != (pred_lut is not None):
        raise real.DevaHipError('boundary_counts: the int16 channel plane and pred_lut go together')
    table = real.id_list(ids)
    if (gt_binary or pred_binary) and table.size != 1:
        raise real.DevaHipError(f'boundary_counts: binary planes hold one object (got {table.size} ids)')
    if radius is None:
        radius = VC.radius_of(size[0], size[1], bound_th)
    if not 0 <= int(radius) <= real.MAX_RADIUS:
        raise real.DevaHipError(f'boundary_counts: radius 0 to {real.MAX_RADIUS} (got {radius})')
    c = VC.counts(_np(gt), _np(pred), table.astype(np.int64), int(radius), gt_binary=gt_binary, pred_binary=pred_binary,
                  pred_lut=_np(pred_lut))
    res = torch.from_numpy(c.view(np.int32).copy()).view(torch.uint32)
    if out is not None:
        out.copy_(res)
        return out
    return res


def install(monkeypatch):
    monkeypatch.setattr(real, 'boundary_counts', boundary_counts)
