"""The numpy statement of the rules E1-E5 of include/deva_mask_runs.h, and the planes the CPU and GPU tests of the
run-length encoder run on.

`pixels` is E1, `bounds_of` E2 and E3 in three lines of numpy, `stats_of` E4, `statement` all of a call with E5's `base` and
`total`.  The counts that follow from the boundaries are held against `rle_case.counts_of` (the shortest counts of a plane,
what a user without the kernel computes on the host) and the strings against the per-value loop `coco_string` of
tests/emu_frame_result.py.

The planes are those of every case of `rle_case.row(h, w)`; its 'zero-counts' row decodes to a plane whose SHORTEST counts
the encoder must give.  `byte_stack` varies the value a set byte holds (1, 2, 255: E1), `float_stack` turns the planes
into logits around a threshold with NaN, both infinities, -0.0 and values equal to the threshold among them."""
import functools

import numpy as np

import rle_case as LC
from emu_frame_result import coco_string

INT32_MAX = 2**31 - 1
# what tests/test_gpu_zb_mask_runs.py runs every row on (the issue's table); the first eight are rle_case.GEOMETRIES
GEOMETRIES = ((1, 1), (1, 9), (9, 1), (2, 2), (33, 67), (64, 64), (65, 129), (128, 144), (480, 854))
THRESHOLDS = (0.0, -1.25)


# ------------------------------------------------------------------------------------------ E1
def pixels(planes, threshold=None):
    """-> bool, same shape: a byte (or bool) is 1 iff it is not 0; a float iff value > threshold (NaN: 0; -0.0 > 0: 0)"""
    planes = np.asarray(planes)
    if planes.dtype == np.float32:
        assert threshold is not None
        with np.errstate(invalid='ignore'):
            return planes > np.float32(threshold)
    assert planes.dtype in (np.uint8, np.bool_) and threshold is None
    return planes != 0


# ------------------------------------------------------------------------------------------ E2, E3, E4
def bounds_of(mask):
    """bool [h,w] -> the ascending positions p = x * h + y whose pixel differs from the one before (0 before p = 0)"""
    flat = np.asarray(mask, dtype=bool).T.reshape(-1)
    before = np.concatenate([[False], flat[:-1]])
    return np.flatnonzero(flat != before).astype(np.int32)


def counts_from(bounds, h, w):
    return np.diff(np.concatenate([[0], np.asarray(bounds, dtype=np.int64), [h * w]])).tolist()


def stats_of(mask):
    """bool [h,w] -> [area, x_min, y_min, x_max, y_max], inclusive; the empty mask keeps 0, INT32_MAX twice, -1 twice"""
    ys, xs = np.nonzero(mask)
    if len(ys) == 0:
        return [0, INT32_MAX, INT32_MAX, -1, -1]
    return [len(ys), int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max())]


def statement(planes, threshold=None, first=0):
    """-> dict(n int32 [N], bounds int32 [total - first], base int64 [N], total int, stats int32 [N,5]) of a stack"""
    ones = pixels(planes, threshold)
    each = [bounds_of(m) for m in ones]
    n = np.array([b.size for b in each], dtype=np.int32)
    base = first + np.cumsum(n.astype(np.int64)) - n
    return dict(n=n, bounds=np.concatenate(each).astype(np.int32) if each else np.zeros(0, np.int32), base=base.astype(np.int64),
                total=int(first + n.sum()), stats=np.array([stats_of(m) for m in ones], dtype=np.int32).reshape(-1, 5))


def records(planes, threshold=None, form='string', stats=False):
    """what `deva.hip.mask_runs.encode` returns, from the statement and the per-value string loop"""
    ones = pixels(planes, threshold)
    h, w = ones.shape[1:]
    out = []
    for m in ones:
        counts = counts_from(bounds_of(m), h, w)
        body = counts if form == 'counts' else coco_string(counts)
        rec = {'size': [h, w], 'counts': body.encode('ascii') if form == 'bytes' else body}
        if stats:
            s = stats_of(m)
            rec['area'], rec['bbox'] = s[0], (s[1:] if s[0] else None)
        out.append(rec)
    return out


# ------------------------------------------------------------------------------------------ the planes
@functools.lru_cache(maxsize=None)
def row_planes(h, w):
    """-> (names, uint8 [N,h,w] of 0 / 1): every case of rle_case.row(h, w), decoded by its statement"""
    names, all_counts = LC.row(h, w)
    planes = LC.planes(all_counts, h, w)
    planes.setflags(write=False)
    return names, planes


def byte_stack(h, w):
    """the row's planes with the set bytes holding 1, 2 and 255 in turn by mask, and 1 / 2 / 255 mixed inside the last"""
    names, planes = row_planes(h, w)
    out = planes.copy()
    for k in range(len(names)):
        out[k] *= np.uint8((1, 2, 255)[k % 3])
    yy, xx = np.mgrid[:h, :w]
    mixed = np.array([1, 2, 255], dtype=np.uint8)[(yy * 5 + xx * 3) % 3]
    out[-1] = np.where(planes[-1] != 0, mixed, 0)
    return names, out


def float_stack(h, w, threshold):
    """the row's planes as float32 logits around `threshold`.  Zeros: values below it, and by position NaN, -inf, the
    threshold itself and (against a threshold of 0) -0.0.  Ones: values above it, +inf and the next float above it."""
    names, planes = row_planes(h, w)
    t = np.float32(threshold)
    yy, xx = np.mgrid[:h, :w]
    pos = (yy * 7 + xx * 13)[None] + np.arange(len(names))[:, None, None] * 3
    below = np.array([t - np.float32(1.5), np.float32('nan'), np.float32('-inf'), t, np.float32(-0.0) if t == 0 else t,
                      np.nextafter(t, np.float32('-inf'))], dtype=np.float32)
    above = np.array([t + np.float32(1.5), np.float32('inf'), np.nextafter(t, np.float32('inf')), t + np.float32(1e-3)], dtype=np.float32)
    out = np.where(planes != 0, above[pos % above.size], below[pos % below.size]).astype(np.float32)
    assert np.array_equal(pixels(out, threshold), planes != 0)
    return names, out


def checkerboard(h, w):
    """[1,h,w] uint8: the value is the parity of the scan position, so every position is a boundary but p = 0"""
    p = np.arange(h * w) & 1
    return p.reshape(w, h).T.astype(np.uint8)[None].copy()


def many_small(n, h, w, seed=7):
    """n overlapping random planes, every fifth one empty and every seventh one full"""
    rng = np.random.default_rng(seed)
    out = (rng.random((n, h, w)) < 0.4).astype(np.uint8)
    out[::5] = 0
    out[3::7] = 1
    return out


def disjoint(h, w, objects=5, seed=3):
    """-> (int64 [h,w] labels with the ids 0..objects, some absent; the ids listed, one of which no pixel holds)"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:h, :w]
    labels = np.zeros((h, w), dtype=np.int64)
    ids = [3, 10, 4, 700, 9][:objects]
    for k, i in enumerate(ids[:-1]):
        cy, cx, r = rng.uniform(0, h), rng.uniform(0, w), max(1.0, min(h, w) / 3)
        labels[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = i
    return labels, ids


# ------------------------------------------------------------------------------------------ where the scans take a second step
# (tests/test_mask_runs_cpu.py derives both from deva_runs_plan, as tests/full_frame_shapes.py does for the frame kernels)
SCAN_GEOMETRY = (1, 2049)     # the smallest plane whose per-mask scan takes two steps: 2049 segments of one row each
SCAN_MASKS = 257              # the smallest stack whose cross-mask scan takes two steps
SCAN_MASKS_SIZE = (9, 17)
