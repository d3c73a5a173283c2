"""TEST-ONLY CPU contract of the pair counts (`deva.hip.pair_metrics.pair_counts`), in the manner of tests/emu_vos.py: the
numpy statement of tests/pair_case.py behind the binding's own argument checks, minus the refusal of host tensors.
`install(monkeypatch)` patches it over the ctypes wrapper.  Integers only, so the device must agree bit for bit."""
import numpy as np
import torch

import pair_case as PC
from deva.hip import pair_metrics as real


def _np(t):
    if t is None:
        return None
    return t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def _u32(a):
    return torch.from_numpy(a.view(np.int32).copy()).view(torch.uint32)


def pair_counts(gt, pred, gt_ids, pred_ids=None, *, bound_th=0.008, radius=None, pred_lut=None, scratch=None, out=None, validate=True):
    _, _, (h, w), fast, radius = real._arguments(gt, pred, gt_ids, pred_ids, radius, bound_th, pred_lut, out)   # (R3: host-only library code)
    table_g = real.id_list(gt_ids, 'gt_ids')
    if fast and isinstance(pred_ids, int):
        n_pred, table_p = pred_ids, pred_ids
        if not 1 <= n_pred <= real.MAX_OBJECTS:
            raise real.DevaHipError(f'pair_counts: at most {real.MAX_OBJECTS} pred_ids, at least one (got {n_pred})')
    else:
        table_p = real.id_list(pred_ids, 'pred_ids')
        n_pred = table_p.size
        table_p = table_p.astype(np.int64)
    real._check_outs(out, table_g.size, n_pred)
    singles, pairs = PC.counts(_np(gt), _np(pred), table_g.astype(np.int64), table_p, radius, pred_lut=_np(pred_lut))
    res = (_u32(singles), _u32(pairs))
    if out is not None:
        out[0].copy_(res[0])
        out[1].copy_(res[1])
        return out[0], out[1]
    return res


def install(monkeypatch):
    monkeypatch.setattr(real, 'pair_counts', pair_counts)
