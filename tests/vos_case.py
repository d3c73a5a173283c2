"""TEST-ONLY numpy statement of the DAVIS counts (rules R1-R6 of include/deva_vos_metrics.h), the per-object way of the
public toolkits: one boolean plane per object, its boundary map with the toolkits' shifted-array lines, dilation by
shifted ORs over the disk, then the arithmetic of J and F.  numpy only.  Also the deterministic cases of the tests:
overlapping ellipses that may leave the image, a shifted and eroded copy as the prediction, a sprinkle of 255."""
import math
import warnings

import numpy as np

U8, I32, I64, INDEX16, BINARY = 0, 1, 2, 3, 256


# ------------------------------------------------------------------------------------------ R1
def slots(plane, ids, binary=False, lut=None):
    """R1 -> int64 [H,W]: the object index of every pixel, -1 for none"""
    a = np.asarray(plane).astype(np.int64)
    if binary:
        return np.where(a != 0, 0, -1)
    n = len(ids)
    if lut is not None:                      # the channel plane: lut[channel]; outside the table or >= n: none
        lut = np.asarray(lut).astype(np.int64).reshape(-1)
        inside = (a >= 0) & (a < lut.size)
        e = np.where(inside, lut[np.clip(a, 0, lut.size - 1)], n)
        return np.where(e < n, e, -1)
    out = np.full(a.shape, -1, dtype=np.int64)
    for i, obj in enumerate(np.asarray(ids, dtype=np.int64).tolist()):
        out[a == obj] = i
    return out


# ------------------------------------------------------------------------------------------ R2
def seg2bmap(seg):
    """the toolkits' boundary map at the mask's own size"""
    seg = np.asarray(seg).astype(bool)
    e, s, se = np.zeros_like(seg), np.zeros_like(seg), np.zeros_like(seg)
    e[:, :-1] = seg[:, 1:]
    s[:-1, :] = seg[1:, :]
    se[:-1, :-1] = seg[1:, 1:]
    b = seg ^ e | seg ^ s | seg ^ se
    b[-1, :] = seg[-1, :] ^ e[-1, :]
    b[:, -1] = seg[:, -1] ^ s[:, -1]
    b[-1, -1] = False
    return b


# ------------------------------------------------------------------------------------------ R3, R4
def radius_of(height, width, bound_th=0.008):
    return int(bound_th) if bound_th >= 1 else int(np.ceil(bound_th * np.linalg.norm((height, width))))


def dilate(b, r):
    """b dilated with the disk x^2 + y^2 <= r^2: the OR of its shifted copies, nothing entering from outside"""
    h, w = b.shape
    out = np.zeros_like(b)
    for dy in range(-r, r + 1):
        half = math.isqrt(r * r - dy * dy)
        for dx in range(-half, half + 1):
            ys, yd = (slice(dy, h), slice(0, h - dy)) if dy >= 0 else (slice(0, h + dy), slice(-dy, h))
            xs, xd = (slice(dx, w), slice(0, w - dx)) if dx >= 0 else (slice(0, w + dx), slice(-dx, w))
            if h - abs(dy) > 0 and w - abs(dx) > 0:
                out[yd, xd] |= b[ys, xs]
    return out


# ------------------------------------------------------------------------------------------ R5
def counts(gt, pred, ids, radius, *, gt_binary=False, pred_binary=False, pred_lut=None):
    """-> uint32 [n,8]"""
    n = len(ids)
    sg = slots(gt, ids, gt_binary)
    sp = slots(pred, ids, pred_binary, None if pred_binary else pred_lut)
    out = np.zeros((n, 8), dtype=np.uint32)
    for i in range(n):
        g, p = sg == i, sp == i
        bg, bp = seg2bmap(g), seg2bmap(p)
        out[i, :7] = ((g & p).sum(), g.sum(), p.sum(), bg.sum(), bp.sum(),
                      (bg & dilate(bp, radius)).sum(), (bp & dilate(bg, radius)).sum())
    return out


# ------------------------------------------------------------------------------------------ R6
def jf(record):
    inter, a_gt, a_pred, n_gt, n_pred, gt_match, pred_match = (int(v) for v in record[:7])
    union = a_gt + a_pred - inter
    j = 1.0 if union == 0 else inter / union
    if n_pred == 0 and n_gt > 0:
        precision, recall = 1.0, 0.0
    elif n_pred > 0 and n_gt == 0:
        precision, recall = 0.0, 1.0
    elif n_pred == 0 and n_gt == 0:
        precision, recall = 1.0, 1.0
    else:
        precision, recall = pred_match / n_pred, gt_match / n_gt
    f = 0.0 if precision + recall == 0 else 2 * precision * recall / (precision + recall)
    return j, f


def statistics(values):
    """(M, O, D) of one object's per-frame values, the toolkits' db_statistics (the uint8 cast of the bin edges wraps
    beyond 255 frames, as theirs does)"""
    v = np.asarray(values, dtype=np.float64)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)      # (the mean of an empty or all-NaN slice is NaN)
        m = np.nanmean(v)
        o = np.nanmean(v > 0.5)
        ids = (np.round(np.linspace(1, len(v), 5) + 1e-10) - 1).astype(np.uint8)
        bins = [v[int(ids[k]):int(ids[k + 1]) + 1] for k in range(4)]
        d = np.nanmean(bins[0]) - np.nanmean(bins[3])
    return float(m), float(o), float(d)


def table(per_object):
    """per_object: [(sequence, k, j values, f values)] -> the seven global numbers in the header's order"""
    sj = np.array([statistics(j) for _, _, j, _ in per_object])
    sf = np.array([statistics(f) for _, _, _, f in per_object])
    jm, jr, jd = sj.mean(axis=0)
    fm, fr, fd = sf.mean(axis=0)
    return [(jm + fm) / 2, jm, jr, jd, fm, fr, fd]


# ------------------------------------------------------------------------------------------ cases
def case(height, width, n_objects, seed, ids=None):
    """-> (gt int64 [H,W], pred int64 [H,W], ids int64 [n]): ellipses painted in order (later ones cover earlier ones),
    centres up to a fifth of the size outside the image; the prediction is each object shifted by up to 2 pixels and
    eroded by one on a random side; about 1 % of both planes is 255 (or an id that no table lists)"""
    rng = np.random.default_rng(seed)
    ids = np.arange(1, n_objects + 1, dtype=np.int64) if ids is None else np.asarray(ids, dtype=np.int64)
    yy, xx = np.mgrid[0:height, 0:width]
    gt = np.zeros((height, width), dtype=np.int64)
    pred = np.zeros((height, width), dtype=np.int64)
    shrink = min(1.0, 2.2 / math.sqrt(n_objects))     # many objects: smaller ones, so that most stay visible
    for i in range(n_objects):
        cy, cx = rng.uniform(-0.2, 1.2) * height, rng.uniform(-0.2, 1.2) * width
        if i < 4:        # the first four are cut by the top-left corner, the bottom-right corner, the left and the top edge
            cy, cx = [(0.0, 0.0), (height - 1.0, width - 1.0), (height / 2, 0.0), (0.0, width / 2)][i]
        ry, rx = rng.uniform(0.08, 0.3) * shrink * height + 1, rng.uniform(0.08, 0.3) * shrink * width + 1
        inside = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0
        gt[inside] = ids[i]
        dy, dx = rng.integers(-2, 3, size=2)
        dy, dx = np.clip(dy, -(height // 4), height // 4), np.clip(dx, -(width // 4), width // 4)   # (a plane one pixel high)
        moved = ((yy - cy - dy) / max(ry - rng.integers(0, 2), 0.5)) ** 2 + ((xx - cx - dx) / max(rx - rng.integers(0, 2), 0.5)) ** 2 <= 1.0
        pred[moved] = ids[i]
    unlisted = 255 if 255 not in ids.tolist() else int(ids.max()) + 7
    gt[rng.random((height, width)) < 0.01] = unlisted
    pred[rng.random((height, width)) < 0.01] = unlisted
    return gt, pred, ids


def channel_form(pred, ids, seed):
    """the tracker's form of `pred`: an int16 channel plane and its lut (uint16, channel -> object index).  Channel 0 is
    the background; the first object has two channels; one more channel holds an id that is not listed (entry 65535) and
    one maps to exactly n (none); unlisted values of `pred` go to the unlisted channel.
    -> (index int16 [H,W], lut uint16 [C], channel_ids int64 [C])"""
    rng = np.random.default_rng(seed)
    n = len(ids)
    channel_ids = np.concatenate([[0], ids, ids[:1], [99999], [88888]]).astype(np.int64)
    lut = np.concatenate([[65535], np.arange(n), [0], [65535], [n]]).astype(np.uint16)
    at = np.searchsorted(ids, pred)
    listed = (at < n) & (ids[np.clip(at, 0, n - 1)] == pred)
    index = np.where(pred == 0, 0, np.where(listed, at + 1, n + 2))
    twin = (index == 1) & (rng.random(pred.shape) < 0.5)
    index[twin] = n + 1
    index[(index == n + 2) & (rng.random(pred.shape) < 0.5)] = n + 3
    return index.astype(np.int16), lut, channel_ids
