"""TEST-ONLY CPU contract of the proposal filter (`deva.hip.ops.proposal_*`, `ops.box_nms`), in the manner of
tests/emu_detections.py: plain numpy / PyTorch, the executable statement of what the HIP kernels must compute.
`install(monkeypatch)` patches it over the ctypes wrappers (next to `emu_ops.install`).

It is written from the rules of include/deva_hip.h (deva_proposal_batch), one rule per line, NOT from the helpers the
reference's generator imports (segment_anything.utils.amg, torchvision.ops: neither is part of the reference's tree).
Counts are integers and both divisions are single correctly rounded fp32 divisions on either side, so the device must
agree bit for bit: planes, tables and keep order.

`state.account` counts what happened to the masks of a frame (tests/proposal_case.py asserts on it)."""
import numpy as np
import torch

from deva.hip import ops as real

F = np.float32


class State:
    def __init__(self, height, width, capacity, arena=None):
        self.height, self.width, self.capacity = height, width, capacity
        self.arena = (torch.zeros(capacity, height, width, dtype=torch.uint8) if arena is None else arena).view(capacity, height, width)
        self.rows, self.equal, self.passed, self.account = [], [], 0, {}

    def note(self, what, n=1):
        self.account[what] = self.account.get(what, 0) + n


def proposal_state(height, width, capacity, device, arena=None):
    if not 1 <= capacity <= real.PROPOSAL_MAX_MASKS:
        raise real.DevaHipError(f'proposal_state: a capacity of 1 to {real.PROPOSAL_MAX_MASKS} masks (got {capacity})')
    return State(int(height), int(width), int(capacity), arena)


def proposal_begin(state):
    state.rows, state.equal, state.passed, state.account = [], [], 0, {}


def box_of(mask):
    """rule 4: smallest and largest column and row of the set pixels, inclusive; 0,0,0,0 for an empty mask"""
    ys, xs = np.nonzero(mask)
    return (int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max())) if len(xs) else (0, 0, 0, 0)


def proposal_batch(state, logits, iou_preds, *, pred_iou_thresh, stability_score_thresh, stability_score_offset, mask_threshold):
    x, iou = logits.cpu().numpy(), iou_preds.cpu().numpy()
    t_iou, t_stab, t_mask = F(pred_iou_thresh), F(stability_score_thresh), F(mask_threshold)
    t_hi, t_lo = F(mask_threshold + stability_score_offset), F(mask_threshold - stability_score_offset)   # sums in double
    for k in range(x.shape[0]):
        if pred_iou_thresh > 0.0 and not iou[k] > t_iou:                         # rule 1 (the plane is not touched)
            state.note('dropped_by_iou')
            continue
        hi, lo = int((x[k] > t_hi).sum()), int((x[k] > t_lo).sum())              # rule 2
        with np.errstate(invalid='ignore', divide='ignore'):
            stability = F(hi) / F(lo)
        if stability_score_thresh > 0.0 and not stability >= t_stab:
            state.note('dropped_by_stability')
            continue
        mask = x[k] > t_mask                                                     # rule 3
        if state.passed < state.capacity:
            state.arena[state.passed] = torch.from_numpy(mask.astype(np.uint8))
            state.rows.append((state.passed, F(iou[k]), stability, *box_of(mask)))  # rule 4
            state.equal.append(bool(stability == t_stab))
        state.passed += 1                                                        # beyond capacity: counted, not stored


def nms_order(scores):
    """descending score, a NaN before every number, among equal scores the lower index"""
    return sorted(range(len(scores)), key=lambda i: (not np.isnan(scores[i]), 0.0 if np.isnan(scores[i]) else -float(scores[i]), i))


def nms(boxes, scores, thresh):
    """rule 5 -> the kept indices in keep order"""
    b = np.asarray(boxes, dtype=np.int64).reshape(-1, 4).astype(F)
    order = np.array(nms_order(np.asarray(scores, dtype=F)), dtype=np.int64)
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    removed, keep = np.zeros(len(b), dtype=bool), []
    for at, i in enumerate(order):
        if removed[i]:
            continue
        keep.append(int(i))
        j = order[at + 1:]
        iw = np.maximum(F(0), np.minimum(b[i, 2], b[j, 2]) - np.maximum(b[i, 0], b[j, 0]))
        ih = np.maximum(F(0), np.minimum(b[i, 3], b[j, 3]) - np.maximum(b[i, 1], b[j, 1]))
        inter = iw * ih
        with np.errstate(invalid='ignore', divide='ignore'):
            ovr = inter / (area[i] + area[j] - inter)
        assert ovr.dtype == F
        removed[j[ovr.astype(np.float64) > thresh]] = True                       # NaN: False
    return keep


def proposal_finish(state, box_nms_thresh):
    if state.passed > state.capacity:
        raise real.DevaHipError(f'proposal_finish: {state.passed} masks passed the filter, the arena holds {state.capacity}')
    keep = nms([r[3:7] for r in state.rows], [r[1] for r in state.rows], box_nms_thresh)
    state.note('kept', len(keep))
    state.note('suppressed_by_nms', len(state.rows) - len(keep))
    rows = [state.rows[i] for i in keep]
    state.note('stability_equal_and_kept', sum(state.equal[i] for i in keep))
    masks = state.arena[torch.tensor(keep, dtype=torch.int64)] if keep else torch.zeros(0, state.height, state.width, dtype=torch.uint8)
    return real.ProposalResult(masks.clone(), torch.tensor([r[1] for r in rows], dtype=torch.float32),
                               torch.tensor(np.array([r[2] for r in rows], dtype=F)),
                               torch.tensor([r[3:7] for r in rows], dtype=torch.int32).view(-1, 4),
                               torch.tensor([r[0] for r in rows], dtype=torch.int32))


def box_nms(boxes, scores, box_nms_thresh):
    if boxes.dim() != 2 or boxes.shape[1] != 4 or boxes.shape[0] > real.PROPOSAL_MAX_MASKS:
        raise real.DevaHipError('box_nms: int32 [M,4] boxes, at most 4096 of them')
    return torch.tensor(nms(boxes.cpu().numpy(), scores.cpu().numpy(), box_nms_thresh), dtype=torch.int32)


def install(monkeypatch):
    for name in ('proposal_state', 'proposal_begin', 'proposal_batch', 'proposal_finish', 'box_nms'):
        monkeypatch.setattr(real, name, globals()[name])
