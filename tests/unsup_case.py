"""TEST-ONLY restatement of the unsupervised DAVIS protocol (rules U1-U5 of deva/inference/unsup_quality.py) from scratch,
the toolkit's way: one boolean plane per proposal and per object, J and F of every (proposal, object) pair on every
frame with `vos_case` (boundary map, disk dilation, R6), means over the video, and the assignment by brute force over
every injective map from objects to proposals.  numpy and itertools only; nothing of the product is imported."""
import itertools

import numpy as np

import vos_case as VC


def pair_jf(gt_mask, pred_mask, radius):
    """J and F of one boolean pair, per plane as the toolkits do it"""
    bg, bp = VC.seg2bmap(gt_mask), VC.seg2bmap(pred_mask)
    rec = ((gt_mask & pred_mask).sum(), gt_mask.sum(), pred_mask.sum(), bg.sum(), bp.sum(), (bg & VC.dilate(bp, radius)).sum(),
           (bp & VC.dilate(bg, radius)).sum())
    return VC.jf(rec)


def brute_force(score):
    """score [P, G], P >= G -> (best total, every injective map (p_0 .. p_G-1) within 1e-9 of it)"""
    score = np.asarray(score, dtype=np.float64)
    n_p, n_g = score.shape
    totals = [(sum(score[p, g] for g, p in enumerate(rows)), rows) for rows in itertools.permutations(range(n_p), n_g)]
    best = max(t for t, _ in totals)
    return best, [rows for t, rows in totals if t >= best - 1e-9]


def video(gts, preds, gt_ids, *, bound_th=0.008, max_proposals=20, skip_ends=False):
    """one video -> dict(proposals, score [P,G], total, maps, J, F per object of the FIRST optimal map, as lists per frame)"""
    h, w = gts[0].shape
    radius = VC.radius_of(h, w, bound_th)
    gt_ids = sorted(int(i) for i in gt_ids)
    proposals = sorted({int(v) for p in preds for v in np.unique(p) if v >= 1})
    if len(proposals) > max_proposals:                                   # U1
        raise ValueError('too many proposals')
    rows = proposals + [None] * max(0, len(gt_ids) - len(proposals))     # U2
    frames = list(range(len(gts)))[1:-1] if skip_ends else list(range(len(gts)))     # U3
    j = np.zeros((len(rows), len(gt_ids), len(frames)))
    f = np.zeros_like(j)
    for a, p in enumerate(rows):
        for b, g in enumerate(gt_ids):
            for c, t in enumerate(frames):
                pm = np.zeros((h, w), dtype=bool) if p is None else np.asarray(preds[t]) == p
                j[a, b, c], f[a, b, c] = pair_jf(np.asarray(gts[t]) == g, pm, radius)
    score = (j.mean(axis=2) + f.mean(axis=2)) / 2                        # U4
    total, maps = brute_force(score)
    first = maps[0]
    return dict(proposals=rows, score=score, total=total, maps=maps, J_all=j, F_all=f,
                J=[j[first[b], b].tolist() for b in range(len(gt_ids))], F=[f[first[b], b].tolist() for b in range(len(gt_ids))])


def table(videos):
    """[(name, video(...) dict)] -> the seven global numbers (U5), by `vos_case.table`"""
    per_object = [(name, k + 1, v['J'][k], v['F'][k]) for name, v in videos for k in range(len(v['J']))]
    return VC.table(per_object), per_object
