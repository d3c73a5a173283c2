"""The numpy statement of the rules O1-O9 of include/deva_rle_overlap.h, and the masks the CPU and GPU tests of the
run-length overlap run on.

`statement(dt, gt, h, w)` derives every mask per pixel from its counts (`rle_case.plane`, rule D1) and takes `inter` and
the areas by boolean AND and sums: no run arithmetic of any kind.  `iou` is pycocotools' arithmetic on those integers,
written as a loop.  `geometry_case(h, w)` is the case table of a geometry; `run_counts(r, h, w)` the column checkerboard of
exactly r runs."""
import functools

import numpy as np

import rle_case as LC

GEOMETRIES = ((1, 1), (1, 9), (9, 1), (2, 2), (63, 65), (480, 854))
DIRECT_LIMIT = 1 << 27      # pixels x pairs up to which `statement` is the literal AND; beyond that a product of 0 / 1 planes


# ------------------------------------------------------------------------------------------ O1, O3
def flat_planes(all_counts, h, w):
    """[n, h * w] bool, every mask derived per pixel from its counts (D1); the order of the pixels is the same for all"""
    out = np.zeros((len(all_counts), h * w), dtype=bool)
    for k, c in enumerate(all_counts):
        out[k] = LC.plane(c, h, w).reshape(-1) != 0
    return out


def statement(dt, gt, h, w, direct=None):
    """-> (inter int64 [D,G], area_d int64 [D], area_g int64 [G]) of two lists of counts"""
    a, b = flat_planes(dt, h, w), flat_planes(gt, h, w)
    inter = np.zeros((len(dt), len(gt)), dtype=np.int64)
    if direct is None:
        direct = len(dt) * len(gt) * h * w <= DIRECT_LIMIT
    if direct:
        for d in range(len(dt)):
            for g in range(len(gt)):
                inter[d, g] = int(np.count_nonzero(a[d] & b[g]))
    else:                                   # the same sums as a product of 0 / 1 values, exact in fp32 below 2^24 a piece
        step = 1 << 18
        for lo in range(0, h * w, step):
            inter += (a[:, lo:lo + step].astype(np.float32) @ b[:, lo:lo + step].astype(np.float32).T).astype(np.int64)
    return inter, a.sum(axis=1).astype(np.int64), b.sum(axis=1).astype(np.int64)


def iou(inter, area_d, area_g, iscrowd=None):
    """pycocotools' rleIou on the integers, pair by pair: u = a_d where crowd, else a_d + a_g - i; i == 0 gives 0"""
    out = np.zeros(inter.shape, dtype=np.float64)
    for d in range(inter.shape[0]):
        for g in range(inter.shape[1]):
            i = int(inter[d, g])
            if i == 0:
                continue
            crowd = iscrowd is not None and bool(iscrowd[g])
            u = int(area_d[d]) if crowd else int(area_d[d]) + int(area_g[g]) - i
            out[d, g] = float(i) / float(u)
    return out


def boxes_of(all_counts, h, w):
    """int64 [n,4] xyxy inclusive, -1 for an empty mask, from the planes (D5)"""
    return LC.records(all_counts, h, w)[2]


# ------------------------------------------------------------------------------------------ the masks
def run_counts(r, h, w):
    """the column checkerboard cut to exactly r runs: r - 1 counts of 1 down the scan, the rest in the last run"""
    assert 1 <= r <= h * w
    return [1] * (r - 1) + [h * w - (r - 1)]


def threshold_frame(lds_runs):
    """the smallest frame that holds lds_runs + 1 runs: one pixel a run"""
    n = lds_runs + 1
    h = max(k for k in range(1, int(n ** 0.5) + 1) if n % k == 0)
    return h, n // h


def small_blobs(h, w, n, seed, radius=None):
    """n masks, each a few discs and holes inside a window of its own (cheap at any frame size) -> list of counts"""
    rng = np.random.default_rng(seed)
    top = max(2, min(h, w) // 6) if radius is None else radius
    out = []
    for _ in range(n):
        p = np.zeros((h, w), dtype=bool)
        cy, cx = int(rng.integers(0, h)), int(rng.integers(0, w))
        y0, y1, x0, x1 = max(0, cy - 2 * top), min(h, cy + 2 * top + 1), max(0, cx - 2 * top), min(w, cx + 2 * top + 1)
        yy, xx = np.mgrid[y0:y1, x0:x1]
        win = np.zeros(yy.shape, dtype=bool)
        for _ in range(3):
            by, bx, r = rng.uniform(cy - top, cy + top), rng.uniform(cx - top, cx + top), rng.uniform(top / 2, top)
            win |= (yy - by) ** 2 + (xx - bx) ** 2 <= r * r
        for _ in range(2):
            by, bx, r = rng.uniform(cy - top, cy + top), rng.uniform(cx - top, cx + top), rng.uniform(0, top / 3)
            win &= ~((yy - by) ** 2 + (xx - bx) ** 2 <= r * r)
        p[y0:y1, x0:x1] = win
        out.append(LC.counts_of(p))
    return out


def touching(h, w):
    """two masks that share exactly one pixel (the middle one), and one that shares none with the first"""
    assert h * w >= 3
    m = h * w // 2
    first, second, third = [0, m + 1, h * w - m - 1], [m, h * w - m], [m + 1, h * w - m - 1]
    return [first], [second, third]


def box_disjoint(h, w):
    """dt in the left half, gt in the right half plus one that crosses: the boxes of the first pairs share no pixel"""
    assert w >= 4 and h >= 2
    left, right, cross = np.zeros((h, w), dtype=np.uint8), np.zeros((h, w), dtype=np.uint8), np.zeros((h, w), dtype=np.uint8)
    left[:, :w // 2 - 1] = 1
    left[0, 0] = 0
    right[1:, w // 2 + 1:] = 1
    cross[h // 2, :] = 1
    return [LC.counts_of(left), LC.counts_of(cross)], [LC.counts_of(right), LC.counts_of(cross), LC.counts_of(left)]


@functools.lru_cache(maxsize=None)
def geometry_case(h, w):
    """-> (dt, gt): the whole row of tests/rle_case.py (empty, full, zero counts first, inside and last, stripes, blobs)
    against itself reversed, so every kind meets every kind and the diagonal-crossing pairs are identical masks"""
    names, all_counts = LC.row(h, w)
    dt = [list(c) for c in all_counts]
    gt = [list(c) for c in all_counts[::-1]] + [[0, 0, 0, h * w, 0, 0]]       # and a full mask written with zero counts
    return dt, gt


def as_rles(all_counts, h, w):
    return LC.as_rles(all_counts, h, w)
