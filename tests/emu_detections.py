"""TEST-ONLY CPU contract of `deva.hip.ops.detection_assemble`, in the manner of tests/emu_frame_result.py: plain
PyTorch, the executable statement of what the HIP kernels must compute (include/deva_hip.h, deva_detection_assemble).
`install(monkeypatch)` patches it over the ctypes wrapper (next to `emu_ops.install`).

It is written from the contract, one rule per line: resized planes P, an area or a paint position per mask, one
first-maximum decision per pixel, counts per mask, a keep rule, ids by counting.  The float sums are torch's (`.sum()`),
whose order is not the kernel's: for planes that are not dyadic the two may round an area differently, which
tests/test_gpu_p_detections.py accounts for from the inputs alone."""
import numpy as np
import torch
import torch.nn.functional as F

from deva.hip import ops as real

RECORD = real.DETECTION_RECORD


def resized(masks, size):
    """[N,H,W] bool / uint8 / fp32 -> fp32 [N,OH,OW] P (the planes themselves at equal sizes)"""
    p = masks.float()
    if tuple(size) != tuple(p.shape[-2:]):
        p = F.interpolate(p.unsqueeze(0), tuple(size), mode='bilinear', align_corners=False)[0]
    return p


def first_maximum(background, scored):
    """per pixel the index of the first maximum over {background, scored[0], scored[1], ...} -> int64 [OH,OW]"""
    best = torch.full(scored.shape[1:], background, dtype=torch.float32)
    hard = torch.zeros(scored.shape[1:], dtype=torch.int64)
    for k in range(scored.shape[0]):
        wins = scored[k] > best
        best = torch.where(wins, scored[k], best)
        hard[wins] = k + 1
    return hard


def paint_positions(source_area):
    """descending area, among equal areas the higher index first -> position of every mask"""
    n = len(source_area)
    order = sorted(range(n), key=lambda k: (-int(source_area[k]), -k))
    pos = [0] * n
    for at, k in enumerate(order):
        pos[k] = at
    return pos


def detection_assemble(masks, size=None, policy='suppress_small', *, scores=None, overlap_threshold=0.8,
                       consistent_ids=False):
    if policy not in real.DETECTION_POLICIES:
        raise real.DevaHipError(f'detection_assemble: policy must be one of {real.DETECTION_POLICIES}')
    if masks.dim() != 3 or masks.shape[0] > real.DETECTION_MAX_MASKS:
        raise real.DevaHipError('detection_assemble: [N,H,W] masks, at most 4096 of them')
    masks = masks.cpu()
    n, h, w = masks.shape
    oh, ow = (h, w) if size is None else (int(size[0]), int(size[1]))
    out = torch.zeros((oh, ow), dtype=torch.int64)
    rec = torch.zeros((n, len(RECORD)), dtype=torch.int32)
    if n == 0:
        return out, rec
    p = resized(masks, (oh, ow))
    original = (p > 0.5).flatten(1).sum(1)
    source = (masks != 0).flatten(1).sum(1)
    rank = list(range(n))
    if policy == 'text':
        rank = paint_positions(source.tolist())
        position = torch.tensor([r + 1 for r in rank], dtype=torch.float32).view(n, 1, 1)
        hard = first_maximum(0.0, (p > 0.5).float() * position)
        flag = hard > 0
    else:
        area = p.flatten(1).sum(1)
        mult = area if policy == 'suppress_small' else area.max() * 2 - area
        hard = first_maximum(0.1, p * mult.view(n, 1, 1))
        flag = torch.zeros_like(hard, dtype=torch.bool)
        for k in range(n):
            flag |= (hard == k + 1) & (p[k] >= 0.5)
    mask_area = torch.stack([(hard == k + 1).sum() for k in range(n)])
    both = torch.stack([((hard == k + 1) & flag).sum() for k in range(n)])
    if policy == 'text':
        keep = [bool(original[k] > 0) for k in range(n)]
    elif policy == 'prefer_small':
        keep = [bool(mask_area[k] > 0) for k in range(n)]
    else:   # the comparison is torch's own: int64 / int64 against a Python float
        keep = [bool(mask_area[k] > 0 and original[k] > 0 and both[k] > 0
                     and not (mask_area[k] / original[k] < overlap_threshold)) for k in range(n)]
    ids, run = [0] * n, 0
    for k in sorted(range(n), key=lambda k: rank[k]):
        if keep[k]:
            run += 1
            ids[k] = run
    table = torch.tensor([0] + ids, dtype=torch.int64)
    if policy == 'suppress_small':
        out = torch.where(flag, table[hard], torch.zeros_like(hard))
    elif policy == 'prefer_small' and not consistent_ids:
        out = hard.clone()
    else:
        out = table[hard]
    rec[:, 0] = torch.tensor(ids, dtype=torch.int32)
    rec[:, 1], rec[:, 2], rec[:, 3], rec[:, 4] = mask_area.int(), original.int(), both.int(), source.int()
    rec[:, 5] = torch.tensor(rank, dtype=torch.int32)
    if scores is not None:
        rec[:, 6] = scores.detach().cpu().float().view(torch.int32)
    return out, rec


def install(monkeypatch):
    monkeypatch.setattr(real, 'detection_assemble', detection_assemble)
