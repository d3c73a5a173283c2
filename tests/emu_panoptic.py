"""TEST-ONLY CPU contract of the joint count (`deva.hip.metrics.panoptic_counts`), in the manner of tests/emu_text.py:
plain numpy, the executable statement of rules C1-C4 of include/deva_metrics.h, one rule per line.  `install(monkeypatch)`
patches it over the ctypes wrapper.  Integers only, so the device must agree bit for bit."""
import numpy as np
import torch

from deva.hip import metrics as real


def plane_ids(plane):
    """C1: the id of every pixel of an RGB8 / I32 / I64 plane -> int64 [H,W]; ids that no table can list become -1"""
    a = np.asarray(plane)
    if a.dtype == np.uint8 and a.ndim == 3:
        a = a.astype(np.int64)
        return a[:, :, 0] + 256 * a[:, :, 1] + 65536 * a[:, :, 2]
    a = a.astype(np.int64)
    return np.where((a < 0) | (a > 2**31 - 1), -1, a)


def slots(ids, table):
    """C2: 0 for id 0, 2 + i for table[i], 1 for anything else"""
    table = np.asarray(table, dtype=np.int64).reshape(-1)
    out = np.ones(ids.shape, dtype=np.int64)
    out[ids == 0] = 0
    for i, t in enumerate(table.tolist()):
        if t != 0:
            out[ids == t] = 2 + i
    return out


def lut_slots(index, lut, p):
    """C3: lut[channel]; an entry >= P, a negative channel and a channel >= len(lut) give slot 1"""
    index = np.asarray(index).astype(np.int64)
    lut = np.asarray(lut).astype(np.int64).reshape(-1)
    inside = (index >= 0) & (index < lut.size)
    e = np.where(inside, lut[np.clip(index, 0, lut.size - 1)], 1)
    return np.where(e < p, e, 1)


def counts(gt, gt_ids, pred, pred_ids=None, pred_lut=None, n_pred=None):
    """C4 -> uint32 [G,P] as numpy"""
    gt_ids = np.zeros(0, dtype=np.int64) if gt_ids is None else np.asarray(gt_ids, dtype=np.int64).reshape(-1)
    if pred_lut is None:
        pred_ids = np.zeros(0, dtype=np.int64) if pred_ids is None else np.asarray(pred_ids, dtype=np.int64).reshape(-1)
        n_pred = pred_ids.size
    g, p = gt_ids.size + 2, n_pred + 2
    sg = slots(plane_ids(gt), gt_ids)
    sp = lut_slots(pred, pred_lut, p) if pred_lut is not None else slots(plane_ids(pred), pred_ids)
    return np.bincount((sg * p + sp).reshape(-1), minlength=g * p).reshape(g, p).astype(np.uint32)


# ------------------------------------------------------------------------------------------ the wrapper's stand-in
def _np(t):
    if t is None or isinstance(t, int):
        return t
    return t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def panoptic_counts(gt, gt_ids, pred, pred_ids=None, pred_lut=None, *, out=None, validate=True):
    """the same argument checks as the wrapper (its own helpers), minus the refusal of host tensors"""
    gt, gt_enc, size = real._plane(gt, 'gt', (real.RGB8, real.I32))
    pred, pred_enc, psize = real._plane(pred, 'pred', (real.RGB8, real.I32, real.I64, real.INDEX16))
    if size != psize:
        raise real.DevaHipError(f'panoptic_counts: gt is {size} and pred {psize}')
    fast = pred_enc == real.INDEX16
    if fast != (pred_lut is not None):
        raise real.DevaHipError('panoptic_counts: the int16 channel plane and pred_lut go together')
    _, n_gt = real._table(gt_ids, 'cpu', 'gt_ids')
    if fast and isinstance(pred_ids, int):
        n_pred = pred_ids
    else:
        _, n_pred = real._table(pred_ids, 'cpu', 'pred_ids')
    c = counts(_np(gt), _np(gt_ids), _np(pred), None if fast else _np(pred_ids), _np(pred_lut), n_pred)
    res = torch.from_numpy(c.view(np.int32).copy()).view(torch.uint32)
    if out is not None:
        out.copy_(res)
        return out
    return res


def install(monkeypatch):
    monkeypatch.setattr(real, 'panoptic_counts', panoptic_counts)
