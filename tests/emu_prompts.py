"""TEST-ONLY CPU contract of the prompt-point choice (`deva.hip.ops.prompt_points`), in the manner of
tests/emu_proposals.py: plain PyTorch on the CPU, the executable statement of what the HIP kernels must compute.
`install(monkeypatch)` patches it over the ctypes wrapper (next to `emu_ops.install`).

It is written from the rules of include/deva_hip.h (deva_prompt_points), one rule per block and every fp32 operation a
separate torch op in the stated order, NOT with F.interpolate / F.grid_sample (tests/test_prompts_cpu.py compares it
with those).  Every operation is a single rounded fp32 one on either side, so the device must agree bit for bit."""
import torch

from deva.hip import ops as real

SCALE, TAPS = 16, 32


def foreground(mask):
    """rule 1: mask > 0 as 1.0f / 0.0f (int64 compared on 64 bits)"""
    return (mask > 0).to(torch.float32)


def axis_weights(n):
    """rule 2 for one axis of n positions -> (pos int64 [n // 16, 32] clamped to the axis, weight fp32 [n // 16, 32]):
    position j of the window of output o is 16 o - 8 + j, its weight (1 - |j - 15.5| / 16) / total, 0 outside"""
    o = torch.arange(n // SCALE).view(-1, 1)
    j = torch.arange(TAPS).view(1, -1)
    pos = SCALE * o - SCALE // 2 + j
    exists = (pos >= 0) & (pos < n)
    raw = (1.0 - (j.to(torch.float32) - 15.5).abs() / 16.0).to(torch.float32).expand(pos.shape)   # multiples of 1/32: exact
    raw = torch.where(exists, raw, torch.zeros(()))
    total = raw.sum(1, keepdim=True)                                                             # exact in any order
    return pos.clamp(0, n - 1), raw / total                                                      # one division per tap


def low_map(fg):
    """rule 2: fp32 [H,W] -> fp32 [H // 16, W // 16]; columns before rows, each sum from 0 in tap order, the product
    and the sum each rounded"""
    h, w = fg.shape
    if h < SCALE or w < SCALE:
        raise real.DevaHipError(f'prompt_points: a mask of at least 16 x 16 (got {h} x {w})')
    pos, wgt = axis_weights(w)
    rows = torch.zeros(h, w // SCALE)
    for j in range(TAPS):
        rows = rows + fg[:, pos[:, j]] * wgt[:, j].view(1, -1)
    pos, wgt = axis_weights(h)
    low = torch.zeros(h // SCALE, w // SCALE)
    for j in range(TAPS):
        low = low + rows[pos[:, j], :] * wgt[:, j].view(-1, 1)
    return low


def unnormalize(c, n):
    g = c * 2 - 1
    return ((g + 1) * float(n) - 1) / 2


def labels_of(low, points_xy):
    """rule 4: the four-tap sample, a tap outside the map is 0"""
    lh, lw = low.shape
    ix, iy = unnormalize(points_xy[:, 0], lw), unnormalize(points_xy[:, 1], lh)
    x0, y0 = torch.floor(ix), torch.floor(iy)
    x1, y1 = x0 + 1, y0 + 1

    def tap(fy, fx, wgt):
        inside = (fy >= 0) & (fy <= lh - 1) & (fx >= 0) & (fx <= lw - 1)
        at = torch.where(inside, fy * lw + fx, torch.zeros(())).to(torch.int64)
        return torch.where(inside, low.reshape(-1)[at] * wgt, torch.zeros(()))

    nw = tap(y0, x0, (x1 - ix) * (y1 - iy))
    ne = tap(y0, x1, (ix - x0) * (y1 - iy))
    sw = tap(y1, x0, (x1 - ix) * (iy - y0))
    se = tap(y1, x1, (ix - x0) * (iy - y0))
    return ((nw + ne) + sw) + se


def prompt_points(mask, points_xy, threshold=0.01, *, scratch=None, packed=None):
    if mask.dim() != 2 or mask.dtype not in (torch.int64, torch.uint8, torch.bool):
        raise real.DevaHipError(f'prompt_points: an [H,W] int64, uint8 or bool mask expected (got {mask.dtype} {tuple(mask.shape)})')
    if points_xy.dim() != 2 or points_xy.shape[1] != 2 or points_xy.dtype != torch.float32:
        raise real.DevaHipError(f'prompt_points: fp32 [P,2] points expected (got {tuple(points_xy.shape)})')
    n = points_xy.shape[0]
    if not 1 <= n <= real.PROMPT_MAX_POINTS:
        raise real.DevaHipError(f'prompt_points: 1 to {real.PROMPT_MAX_POINTS} points (got {n})')
    if threshold != threshold:
        raise real.DevaHipError('prompt_points: the threshold is not a number')
    points_xy = points_xy.cpu()
    labels = labels_of(low_map(foreground(mask.cpu())), points_xy)
    keep = labels < torch.tensor(threshold, dtype=torch.float32)                                  # rule 5: strict, fp32
    kept = points_xy[keep]
    out = torch.full((n, 2), float('nan'))                                                       # beyond the count: not written
    out[:kept.shape[0]] = kept
    return out, labels, torch.tensor([kept.shape[0]], dtype=torch.int32)


def install(monkeypatch):
    monkeypatch.setattr(real, 'prompt_points', prompt_points)
