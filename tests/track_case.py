"""The statement of the rules T1-T9 of `deva.inference.track_quality` (HOTA and OWTA over alpha = 0.05 .. 0.95), written
from the published definition with plain loops: IoU from boolean planes, the per-frame assignment by brute force over
permutations, no code shared with the scorer.  Also the synthetic clips the CPU and GPU tests run on."""
import itertools
import math

import numpy as np

ALPHAS = [0.05 * k for k in range(1, 20)]
EPS = float(np.finfo(np.float64).eps)
FIELDS = ('HOTA', 'DetA', 'AssA', 'DetRe', 'DetPr', 'AssRe', 'AssPr', 'LocA', 'OWTA')


def plane_iou(a, b):
    inter = int(np.count_nonzero(a & b))
    if inter == 0:
        return 0.0
    return float(inter) / float(int(np.count_nonzero(a)) + int(np.count_nonzero(b)) - inter)


def sims_of(clip):
    """clip: [(gt {id: bool plane}, pred {id: bool plane})] -> [(gt ids, pred ids, sim [G][P] as lists)]"""
    out = []
    for gt, pred in clip:
        g_ids, p_ids = list(gt), list(pred)
        out.append((g_ids, p_ids, [[plane_iou(gt[g], pred[p]) for p in p_ids] for g in g_ids]))
    return out


def best_pairs(score):
    """maximum-weight assignment of an [n][m] table by brute force: every row of the shorter side gets a partner"""
    n, m = len(score), len(score[0]) if score else 0
    if n == 0 or m == 0:
        return []
    best, best_total = None, -math.inf
    if n <= m:
        for cols in itertools.permutations(range(m), n):
            total = math.fsum(score[r][cols[r]] for r in range(n))
            if total > best_total:
                best, best_total = [(r, cols[r]) for r in range(n)], total
    else:
        for rows in itertools.permutations(range(n), m):
            total = math.fsum(score[rows[c]][c] for c in range(m))
            if total > best_total:
                best, best_total = sorted((rows[c], c) for c in range(m)), total
    return best


def sequence(frames):
    """frames: what `sims_of` gives -> the per-sequence record: TP, FN, FP, AssA, AssRe, AssPr, LocA per alpha"""
    gt_count, pr_count, potential = {}, {}, {}
    for g_ids, p_ids, sim in frames:                                     # T2, T3
        for g in g_ids:
            gt_count[g] = gt_count.get(g, 0) + 1
        for p in p_ids:
            pr_count[p] = pr_count.get(p, 0) + 1
        for i, g in enumerate(g_ids):
            for j, p in enumerate(p_ids):
                denom = sum(sim[i]) + sum(row[j] for row in sim) - sim[i][j]
                if denom > 0 + EPS:
                    potential[g, p] = potential.get((g, p), 0.0) + sim[i][j] / denom
    def alignment(g, p):                                                 # T4
        pmc = potential.get((g, p), 0.0)
        return pmc / (gt_count[g] + pr_count[p] - pmc)
    rec = {k: [0] * len(ALPHAS) for k in ('HOTA_TP', 'HOTA_FN', 'HOTA_FP')}
    loc = [0.0] * len(ALPHAS)
    matches = [dict() for _ in ALPHAS]
    for g_ids, p_ids, sim in frames:                                     # T5, T6
        if not g_ids:
            for a in range(len(ALPHAS)):
                rec['HOTA_FP'][a] += len(p_ids)
            continue
        if not p_ids:
            for a in range(len(ALPHAS)):
                rec['HOTA_FN'][a] += len(g_ids)
            continue
        pairs = best_pairs([[alignment(g, p) * sim[i][j] for j, p in enumerate(p_ids)] for i, g in enumerate(g_ids)])
        for a, alpha in enumerate(ALPHAS):
            hits = [(i, j) for i, j in pairs if sim[i][j] >= alpha - EPS]
            rec['HOTA_TP'][a] += len(hits)
            rec['HOTA_FN'][a] += len(g_ids) - len(hits)
            rec['HOTA_FP'][a] += len(p_ids) - len(hits)
            for i, j in hits:
                loc[a] += sim[i][j]
                key = (g_ids[i], p_ids[j])
                matches[a][key] = matches[a].get(key, 0) + 1
    for name in ('AssA', 'AssRe', 'AssPr', 'LocA'):
        rec[name] = [0.0] * len(ALPHAS)
    for a in range(len(ALPHAS)):                                         # T7
        top = max(1, rec['HOTA_TP'][a])
        for (g, p), mc in matches[a].items():
            rec['AssA'][a] += mc * mc / max(1, gt_count[g] + pr_count[p] - mc) / top
            rec['AssRe'][a] += mc * mc / max(1, gt_count[g]) / top
            rec['AssPr'][a] += mc * mc / max(1, pr_count[p]) / top
        rec['LocA'][a] = max(1e-10, loc[a]) / max(1e-10, rec['HOTA_TP'][a])
    return rec


def combined(records):
    """T8, then the rest of T7 -> the record with every field per alpha and 'summary'"""
    n = len(ALPHAS)
    out = {k: [sum(r[k][a] for r in records) for a in range(n)] for k in ('HOTA_TP', 'HOTA_FN', 'HOTA_FP')}
    for name in ('AssA', 'AssRe', 'AssPr'):
        out[name] = [sum(r[name][a] * r['HOTA_TP'][a] for r in records) / max(1, out['HOTA_TP'][a]) for a in range(n)]
    out['LocA'] = [max(1e-10, sum(r['LocA'][a] * r['HOTA_TP'][a] for r in records)) / max(1e-10, out['HOTA_TP'][a]) for a in range(n)]
    tp, fn, fp = out['HOTA_TP'], out['HOTA_FN'], out['HOTA_FP']
    out['DetRe'] = [tp[a] / max(1, tp[a] + fn[a]) for a in range(n)]
    out['DetPr'] = [tp[a] / max(1, tp[a] + fp[a]) for a in range(n)]
    out['DetA'] = [tp[a] / max(1, tp[a] + fn[a] + fp[a]) for a in range(n)]
    out['HOTA'] = [math.sqrt(out['DetA'][a] * out['AssA'][a]) for a in range(n)]
    out['OWTA'] = [math.sqrt(out['DetRe'][a] * out['AssA'][a]) for a in range(n)]
    out['summary'] = {f: sum(out[f]) / n for f in FIELDS}
    return out


def restrict(clip, categories, ids):
    """T9: the ground-truth tracks whose category is in `ids`, every predicted track"""
    return [({g: m for g, m in gt.items() if categories[g] in ids}, pred) for gt, pred in clip]


def score(clips, groups=None, categories=None):
    """clips: {name: clip} -> {group: combined record}, as `TrackQualityScorer.result()`"""
    out = {}
    for group, ids in ([('all', None)] if groups is None else groups.items()):
        records = []
        for name, clip in clips.items():
            kept = clip if ids is None else restrict(clip, categories[name], set(ids))
            records.append(sequence(sims_of(kept)))
        out[group] = combined(records)
    return out


# ------------------------------------------------------------------------------------------ the clips
def _box(h, w, y0, x0, bh, bw):
    p = np.zeros((h, w), dtype=bool)
    p[max(0, y0):max(0, y0 + bh), max(0, x0):max(0, x0 + bw)] = True
    return p


def synthetic_clip(h=96, w=128, frames=6, n_gt=4, n_pred=5, seed=0):
    """moving boxes: ground-truth track g drifts across the frame; predicted track p follows track p % n_gt with an offset
    and a size error that differ per track and frame, some tracks are absent on some frames (one frame has no prediction,
    one ground-truth track starts late), the last predicted track follows nothing.  Track ids are strings."""
    rng = np.random.default_rng(seed)
    clip = []
    gy, gx = rng.integers(5, h // 2, n_gt), rng.integers(5, w // 2, n_gt)
    gh, gw = rng.integers(h // 6, h // 3, n_gt), rng.integers(w // 6, w // 3, n_gt)
    vy, vx = rng.integers(-3, 4, n_gt), rng.integers(-4, 5, n_gt)
    for t in range(frames):
        gt, pred = {}, {}
        for g in range(n_gt):
            if g == n_gt - 1 and t == 0:
                continue                                                   # a track that starts late
            gt[str(100 + g)] = _box(h, w, gy[g] + t * vy[g], gx[g] + t * vx[g], gh[g], gw[g])
        if t != 2:                                                         # a frame with no prediction at all
            for p in range(n_pred):
                if (p + t) % 5 == 4:
                    continue                                               # a track that drops out now and then
                g = p % n_gt
                dy, dx, dh, dw = (int(v) for v in rng.integers(-4, 5, 4))
                if p == n_pred - 1:
                    pred[str(p + 1)] = _box(h, w, h - 12 - t, w - 20 - t, 8, 12)   # follows nothing
                else:
                    pred[str(p + 1)] = _box(h, w, gy[g] + t * vy[g] + dy, gx[g] + t * vx[g] + dx, gh[g] + dh, gw[g] + dw)
        clip.append((gt, pred))
    return clip


def random_clip(rng, h=12, w=16, frames=4, n_gt=3, n_pred=3):
    """small random boxes, tracks present at random: the tables stay small enough for the brute-force assignment"""
    clip = []
    for _ in range(frames):
        gt = {str(g): _box(h, w, *rng.integers(0, h // 2, 1), *rng.integers(0, w // 2, 1), *rng.integers(2, h // 2 + 1, 1), *rng.integers(2, w // 2 + 1, 1))
              for g in range(n_gt) if rng.random() < 0.8}
        pred = {str(10 + p): _box(h, w, *rng.integers(0, h // 2, 1), *rng.integers(0, w // 2, 1), *rng.integers(2, h // 2 + 1, 1), *rng.integers(2, w // 2 + 1, 1))
                for p in range(n_pred) if rng.random() < 0.8}
        clip.append((gt, pred))
    return clip
