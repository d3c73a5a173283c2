"""The input recipe of the proposal-filter tests, shared by the CPU and the GPU side: mask-logit planes and predicted
IoUs as a point-prompted segmenter gives them, built so that every rule of the contract (include/deva_hip.h,
deva_proposal_batch) decides something.

  * A plane is a centre-distance ramp, slope * (radius - distance), around one of a few shared centres with one of a
    few shared radii: the same disc comes back with another slope or prediction, which is what box NMS is for.
  * Slopes are steep and shallow: (r - 1/slope)^2 / (r + 1/slope)^2 spreads on both sides of the stability threshold.
  * Values are rounded to multiples of 1/4, so logits EQUAL to t_hi = 1, t_lo = -1 and the mask threshold 0 occur (the
    comparisons are strict), and the ramps are clamped at -1 = t_lo: the whole background sits on that threshold.
  * Predictions sit on a coarse grid on both sides of 0.88, so equal predictions occur (the NMS tie rule).
  * Every eleventh plane is a step plane: n_hi pixels at 2, then pixels at exactly 1 (= t_hi) up to n_lo, the rest at
    -1: its stability is n_hi / n_lo, which `EXACT` chooses equal to the stability threshold in fp32 (19 / 20 for 0.95,
    16 / 20 for 0.8).  Every thirteenth is empty above 0 but not above -1 (lo > 0, box 0,0,0,0), every seventeenth is
    nowhere above -1 (lo = 0).

`frame(...)` gives the three batches of a frame: the batch of B planes, a batch without a survivor and one with B = 0,
in an order that depends on B.  `check_case` asserts on the oracle's own account of a geometry's frames that every
outcome occurs at least twice."""
import functools
import math

import numpy as np
import torch

PARAMS = dict(pred_iou_thresh=0.88, stability_score_thresh=0.95, stability_score_offset=1.0, mask_threshold=0.0,
              box_nms_thresh=0.7)
EXACT = {0.95: (19, 20), 0.8: (16, 20)}          # n_hi / n_lo == fp32(threshold) under a correctly rounded division
GRID = (0.80, 0.85, 0.90, 0.90, 0.95, 0.95, 1.0)  # predicted IoUs
SLOPES = (16.0, 8.0, 4.0, 1.0)
BATCHES = (1, 3, 64, 192, 193)
GEOMETRIES = ((29, 53), (30, 45), (64, 64))       # planes 4 bytes off a 16-byte boundary / width % 4 != 0 / all aligned


def params(stability=0.95, **over):
    return dict(PARAMS, stability_score_thresh=stability, **over)


def ramps(h, w, centres, radii, slopes, device='cpu'):
    """fp32 [N,H,W]: round4(slope * (radius - distance to the centre)), clamped below at -1"""
    yy = torch.arange(h, dtype=torch.float32, device=device).view(1, h, 1)
    xx = torch.arange(w, dtype=torch.float32, device=device).view(1, 1, w)
    cy, cx = (torch.tensor([c[i] for c in centres], dtype=torch.float32, device=device).view(-1, 1, 1) for i in (0, 1))
    r = torch.tensor(radii, dtype=torch.float32, device=device).view(-1, 1, 1)
    s = torch.tensor(slopes, dtype=torch.float32, device=device).view(-1, 1, 1)
    dist = ((yy - cy) ** 2 + (xx - cx) ** 2).sqrt()      # (squares of small integers and halves: exact; sqrt is IEEE)
    return (torch.round((r - dist) * s * 4) / 4).clamp_(min=-1.0)


def step_plane(h, w, n_hi, n_lo, at):
    """n_hi pixels at 2 and n_lo - n_hi at exactly 1 in a 5-wide block whose corner is `at`, -1 elsewhere"""
    plane = torch.full((h, w), -1.0)
    y0, x0 = at
    for i in range(n_lo):
        plane[y0 + i // 5, x0 + i % 5] = 2.0 if i < n_hi else 1.0
    return plane


def shared(h, w):
    """the few centres (some on half pixels) and radii every plane of a geometry draws from"""
    centres = [(h * 0.3, w * 0.25), (h * 0.5 + 0.5, w * 0.5), (h * 0.7, w * 0.75 + 0.5), (h * 0.35, w * 0.7)]
    centres = [(math.floor(y * 2) / 2, math.floor(x * 2) / 2) for y, x in centres]
    top = min(h, w) / 2.5
    return centres, [top, top * 0.8, top * 0.5]


def draw(h, w, b, seed):
    """the draws of a batch: (centres, radii, slopes, predicted IoUs), b of each"""
    rng = np.random.default_rng(seed)
    centres, radii = shared(h, w)
    pick = lambda seq: [seq[i] for i in rng.integers(0, len(seq), b)]  # noqa: E731
    return pick(centres), pick(radii), pick(SLOPES), pick(GRID)


def batch(h, w, b, seed, stability=0.95):
    """-> (logits fp32 [b,h,w], iou_preds fp32 [b]) on the host"""
    centres, radii, slopes, grid = draw(h, w, b, seed)
    logits = ramps(h, w, centres, radii, slopes) if b else torch.zeros(0, h, w)
    iou = torch.tensor(grid, dtype=torch.float32)
    n_hi, n_lo = EXACT[stability]
    for k in range(b):
        if b >= 11 and k % 11 == 5:
            logits[k] = step_plane(h, w, n_hi, n_lo, (1 + (k // 11) % 4 * 6, 1 + (k // 44) * 6))
            iou[k] = (0.9, 1.0)[k // 11 % 2]
        elif b >= 13 and k % 13 == 7:
            logits[k] = logits[k].clamp(max=0.0)          # nothing above the mask threshold
        elif b >= 17 and k % 17 == 9:
            logits[k] = -1.0                              # nothing above t_lo either
    return logits, iou


def barren(h, w, seed):
    """a batch without a survivor: predictions at and below the threshold, shallow ramps, an all-negative plane"""
    centres, radii = shared(h, w)
    logits = ramps(h, w, centres[:4], [radii[2]] * 4, [1.0, 0.5, 16.0, 16.0])
    logits[3] = -1.0
    return logits, torch.tensor([0.95, 1.0, 0.85, 1.0], dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def frame(h, w, b, stability=0.95):
    """the three batches of the frame of (geometry, B), read-only: B planes, no survivor, B = 0, rotated by B"""
    seed = h * 1000 + w * 10 + b
    three = [batch(h, w, b, seed, stability), barren(h, w, seed), batch(h, w, 0, seed, stability)]
    return tuple(three[(i + b) % 3] for i in range(3))


@functools.lru_cache(maxsize=None)
def oracle(h, w, b, stability=0.95):
    """(result, account) of the CPU statement on `frame(h, w, b)`, computed once and shared (read-only)"""
    import emu_proposals as EP
    state = EP.proposal_state(h, w, 4096, 'cpu')
    EP.proposal_begin(state)
    p = params(stability)
    nms = p.pop('box_nms_thresh')
    for logits, iou in frame(h, w, b, stability):
        EP.proposal_batch(state, logits, iou, **p)
    return EP.proposal_finish(state, nms), dict(state.account)


@functools.lru_cache(maxsize=None)
def check_case(h, w, stability=0.95):
    """over the frames of a geometry: every outcome at least twice (asserted on the oracle alone)"""
    total = {}
    for b in BATCHES:
        for name, n in oracle(h, w, b, stability)[1].items():
            total[name] = total.get(name, 0) + n
    for name in ('dropped_by_iou', 'dropped_by_stability', 'stability_equal_and_kept', 'suppressed_by_nms', 'kept'):
        assert total.get(name, 0) >= 2, (h, w, stability, name, total)
    return total
