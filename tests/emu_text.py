"""TEST-ONLY CPU contract of the box prompts (`deva.hip.ops.box_nms_xyxy`, `ops.box_mask_select`), in the manner of
tests/emu_proposals.py: plain numpy, the executable statement of what the HIP kernels must compute.
`install(monkeypatch)` patches it over the ctypes wrappers (next to `emu_ops.install`).

It is written from the rules of include/deva_hip.h (deva_box_nms_xyxy: N1-N4, deva_box_mask_select: S1-S3), one rule per
line, NOT from torchvision or segment_anything (neither is part of the reference's tree, nor installed).  Every
operation is a single rounded fp32 one on either side and the rest are comparisons, so the device must agree bit for
bit: keep lists in order, choices and planes."""
import numpy as np
import torch

from deva.hip import ops as real
from emu_proposals import nms_order

F = np.float32


def nms_xyxy(boxes, scores, thresh):
    """rules N1-N4 on fp32 boxes as given -> the kept indices in keep order"""
    b = np.asarray(boxes, dtype=F).reshape(-1, 4)
    order = np.array(nms_order(np.asarray(scores, dtype=F)), dtype=np.int64)          # N4
    with np.errstate(invalid='ignore', over='ignore'):
        area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])                              # N1: no +1, negative when inverted
    removed, keep = np.zeros(len(b), dtype=bool), []
    for at, i in enumerate(order):
        if removed[i]:
            continue
        keep.append(int(i))
        j = order[at + 1:]
        with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
            iw = np.maximum(F(0), np.minimum(b[i, 2], b[j, 2]) - np.maximum(b[i, 0], b[j, 0]))
            ih = np.maximum(F(0), np.minimum(b[i, 3], b[j, 3]) - np.maximum(b[i, 1], b[j, 1]))
            inter = iw * ih
            ovr = inter / (area[i] + area[j] - inter)                                 # N2
        assert ovr.dtype == F
        removed[j[ovr.astype(np.float64) > thresh]] = True                            # N3 (NaN: False)
    return keep


def choice(scores):
    """rule S1 for one box: the first NaN, else the first maximum (-0.0 == 0.0); numpy's argmax, spelled out"""
    best, v = 0, F(scores[0])
    for m in range(1, len(scores)):
        c = F(scores[m])
        if not np.isnan(v) and (np.isnan(c) or c > v):
            best, v = m, c
    return best


def mask_select(logits, scores, mask_threshold=0.0):
    """rules S1-S3 -> (uint8 [B,H,W], int32 [B]) as numpy"""
    x, s = np.asarray(logits, dtype=F), np.asarray(scores, dtype=F)
    b, m, h, w = x.shape
    chosen = np.array([choice(s[k]) for k in range(b)], dtype=np.int32)
    planes = np.zeros((b, h, w), dtype=np.uint8)
    with np.errstate(invalid='ignore'):
        for k in range(b):
            planes[k] = x[k, chosen[k]] > F(mask_threshold)                           # S2: strict, NaN -> 0; S3
    return planes, chosen


# ------------------------------------------------------------------------------------------ the wrappers' stand-ins
def box_nms_xyxy(boxes, scores, thresh, *, packed=None):
    if boxes.dim() != 2 or boxes.shape[1] != 4:
        raise real.DevaHipError(f'box_nms_xyxy: fp32 [M,4] boxes expected (got {tuple(boxes.shape)})')
    m = boxes.shape[0]
    if tuple(scores.shape) != (m,):
        raise real.DevaHipError(f'box_nms_xyxy: scores must be fp32 [{m}] (got {tuple(scores.shape)})')
    if m > real.PROPOSAL_MAX_MASKS:
        raise real.DevaHipError(f'box_nms_xyxy: at most {real.PROPOSAL_MAX_MASKS} boxes (got {m})')
    if boxes.dtype != torch.float32 or scores.dtype != torch.float32:
        raise real.DevaHipError('box_nms_xyxy: boxes and scores must be torch.float32')
    keep = nms_xyxy(boxes.cpu().numpy(), scores.cpu().numpy(), float(thresh))
    if packed is None:
        return torch.tensor(keep, dtype=torch.int32)
    assert packed.dtype == torch.int32 and packed.numel() == m + 1
    packed[:len(keep)] = torch.tensor(keep, dtype=torch.int32)
    packed[m] = len(keep)
    return packed


def box_mask_select(logits, scores, mask_threshold=0.0, out=None):
    if logits.dim() != 4:
        raise real.DevaHipError(f'box_mask_select: [B,M,H,W] logits expected (got {tuple(logits.shape)})')
    b, m, h, w = logits.shape
    if not 1 <= m <= real.BOX_MAX_PER_BOX:
        raise real.DevaHipError(f'box_mask_select: 1 to {real.BOX_MAX_PER_BOX} planes per box (got {m})')
    if tuple(scores.shape) != (b, m):
        raise real.DevaHipError(f'box_mask_select: scores must be fp32 [{b},{m}] (got {tuple(scores.shape)})')
    planes, chosen = mask_select(logits.cpu().numpy(), scores.cpu().numpy(), mask_threshold)
    planes = torch.from_numpy(planes)
    if out is not None:
        assert out.dtype == torch.uint8 and tuple(out.shape) == (b, h, w)
        out.copy_(planes)
        planes = out
    return planes, torch.from_numpy(chosen)


def install(monkeypatch):
    for name in ('box_nms_xyxy', 'box_mask_select'):
        monkeypatch.setattr(real, name, globals()[name])
