"""TEST-ONLY numpy statement of the pair counts (rules P1-P5 of include/deva_pair_metrics.h), built on the statement of
the DAVIS counts (tests/vos_case.py: `slots`, `seg2bmap`, `dilate`): one boolean plane, one boundary map and ONE dilation
per object and side -- not per pair -- and then plain ANDs and sums for every (g, p).  numpy only.  Also the
deterministic cases of the tests: `vos_case.case` with the prediction's ids renamed, objects split and merged."""
import numpy as np

import vos_case as VC


def counts(gt, pred, gt_ids, pred_ids, radius, *, pred_lut=None):
    """-> (singles uint32 [G + P, 2], pairs uint32 [G, P, 4]); with `pred_lut` the prediction is a channel plane and
    `pred_ids` only says how many proposals there are (a list or an int)"""
    n_pred = pred_ids if isinstance(pred_ids, int) else len(pred_ids)
    sg = VC.slots(gt, gt_ids)
    sp = VC.slots(pred, list(range(n_pred)), lut=pred_lut) if pred_lut is not None else VC.slots(pred, pred_ids)
    n_gt = len(gt_ids)
    masks_g, masks_p = [sg == g for g in range(n_gt)], [sp == p for p in range(n_pred)]
    bound_g, bound_p = [VC.seg2bmap(m) for m in masks_g], [VC.seg2bmap(m) for m in masks_p]
    near_g, near_p = [VC.dilate(b, radius) for b in bound_g], [VC.dilate(b, radius) for b in bound_p]
    singles = np.zeros((n_gt + n_pred, 2), dtype=np.uint32)
    pairs = np.zeros((n_gt, n_pred, 4), dtype=np.uint32)
    for i, (m, b) in enumerate(zip(masks_g + masks_p, bound_g + bound_p)):
        singles[i] = (m.sum(), b.sum())
    for g in range(n_gt):
        for p in range(n_pred):
            pairs[g, p, :3] = ((masks_g[g] & masks_p[p]).sum(), (bound_g[g] & near_p[p]).sum(), (bound_p[p] & near_g[g]).sum())
    return singles, pairs


def record(singles, pairs, g, p):
    """the record of `vos_case.counts` (R5) of the pair (g, p) -> int64 [8]"""
    n_gt = pairs.shape[0]
    return np.array([pairs[g, p, 0], singles[g, 0], singles[n_gt + p, 0], singles[g, 1], singles[n_gt + p, 1], pairs[g, p, 1],
                     pairs[g, p, 2], 0], dtype=np.int64)


def records(singles, pairs):
    """-> int64 [P, G, 8]: every pair's record, proposals first (the scorer's layout)"""
    n_gt, n_pred = pairs.shape[:2]
    return np.stack([np.stack([record(singles, pairs, g, p) for g in range(n_gt)]) for p in range(n_pred)])


def rename(pred, ids, new_ids):
    """the plane with every id of `ids` replaced by its entry of `new_ids`, other values kept"""
    out = pred.copy()
    for old, new in zip(np.asarray(ids).tolist(), np.asarray(new_ids).tolist()):
        out[pred == old] = new
    return out


def case(height, width, n_gt, n_pred, seed, gt_ids=None, pred_ids=None):
    """-> (gt int64 [H,W], pred int64 [H,W], gt_ids int64 [G], pred_ids int64 [P]): `vos_case.case` with max(G, P)
    objects; the ground truth keeps the first G of them (the rest become background), the prediction the first P under
    ids of its own (by default 100 + 3 k, in another order than the objects).  Unlisted values (255) stay on both sides."""
    rng = np.random.default_rng(seed + 9999)
    n = max(n_gt, n_pred)
    gt, pred, ids = VC.case(height, width, n, seed)
    gt_ids = ids[:n_gt] if gt_ids is None else np.asarray(gt_ids, dtype=np.int64)
    pred_ids = 100 + 3 * np.arange(n_pred, dtype=np.int64) if pred_ids is None else np.asarray(pred_ids, dtype=np.int64)
    gt = rename(np.where(np.isin(gt, ids[n_gt:]), 0, gt), ids[:n_gt], gt_ids)
    assert 255 not in gt_ids.tolist() + pred_ids.tolist()
    pred = rename(np.where(np.isin(pred, ids[n_pred:]), 0, pred), ids[:n_pred], pred_ids[rng.permutation(n_pred)])
    return gt, pred, np.sort(gt_ids), np.sort(pred_ids)
