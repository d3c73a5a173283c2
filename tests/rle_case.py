"""The numpy statement of the rules D1-D5 of include/deva_rle.h, and the masks the CPU and GPU tests of the run-length
decoder run on.

`plane(counts, h, w)` is D1 in two lines of numpy (and what a user without the kernel does on the host: the bench times it);
`coco_decode` of tests/emu_frame_result.py, a per-pixel loop over the COCO API's algorithm, is the independent slow form it
is held against.  `nearest` is D3, `records` D5 from the decoded plane (not from the counts, as the product computes
them).

`row(h, w)` is the case table: per geometry the masks that together reach every outcome the decoder can meet, each as its
counts.  `claims(h, w)` names the outcomes a geometry can hold at all and `outcomes(counts, h, w)` finds them in a mask;
tests/test_rle_cpu.py asserts the one against the other."""
import functools

import numpy as np

from emu_frame_result import coco_decode, coco_parse, coco_string  # noqa: F401  (the slow forms, for the tests)

GEOMETRIES = ((1, 1), (1, 9), (9, 1), (2, 2), (33, 67), (64, 64), (65, 129), (480, 854))
RESIZES = (((33, 67), (66, 134)), ((65, 129), (48, 95)), ((480, 854), (320, 569)))


# ------------------------------------------------------------------------------------------ D1, D2
def valid(counts, h, w):
    """D2 for one mask"""
    c = np.asarray(counts, dtype=np.int64)
    return 1 <= h * w < 2**31 and bool((c >= 0).all()) and int(c.sum()) == h * w


def plane(counts, h, w):
    """D1: counts -> uint8 [h,w] of 0 / 1.  Run k holds the value k & 1; zero counts repeat nothing, so the runs that
    share a start leave the pixel to the last of them."""
    c = np.asarray(counts, dtype=np.int64)
    assert valid(c, h, w), (c[:8], h, w)
    return np.repeat((np.arange(c.size) & 1).astype(np.uint8), c).reshape(w, h).T


def planes(all_counts, h, w):
    return np.stack([plane(c, h, w) for c in all_counts]) if len(all_counts) else np.zeros((0, h, w), dtype=np.uint8)


def counts_of(mask):
    """a plane -> its shortest counts (the first one may be 0, no other is), vectorised"""
    flat = (np.asarray(mask) != 0).T.reshape(-1)
    change = np.flatnonzero(flat[1:] != flat[:-1]) + 1
    counts = np.diff(np.concatenate([[0], change, [flat.size]]))
    return ([0] if flat[0] else []) + counts.tolist()


# ------------------------------------------------------------------------------------------ D3
def nearest_index(out, size):
    """the source index of every output index: ATen's nearest rule with the scale size / out in fp32"""
    scale = np.float32(size) / np.float32(out)
    return np.minimum(np.floor(np.arange(out, dtype=np.float32) * scale).astype(np.int64), size - 1)


def nearest(stack, oh, ow):
    """[..., h, w] -> [..., oh, ow] by D3; equal sizes are the identity"""
    h, w = stack.shape[-2:]
    return np.ascontiguousarray(stack[..., nearest_index(oh, h), :][..., nearest_index(ow, w)])


def decoded(all_counts, h, w, size=None, dtype=np.uint8):
    """D1, D3, D4 in a row: what `deva.hip.rle.decode` returns, as a numpy array"""
    out = planes(all_counts, h, w)
    if size is not None:
        out = nearest(out, int(size[0]), int(size[1]))
    return out.astype(dtype)


# ------------------------------------------------------------------------------------------ D5
def records(all_counts, h, w):
    """-> (runs int64 [n], area int64 [n], bbox int64 [n,4] xyxy inclusive, -1 for an empty mask), from the planes"""
    runs = np.array([len(c) for c in all_counts], dtype=np.int64)
    area, bbox = np.zeros(len(all_counts), dtype=np.int64), np.full((len(all_counts), 4), -1, dtype=np.int64)
    for k, c in enumerate(all_counts):
        ys, xs = np.nonzero(plane(c, h, w))
        area[k] = len(ys)
        if len(ys):
            bbox[k] = (xs.min(), ys.min(), xs.max(), ys.max())
    return runs, area, bbox


# ------------------------------------------------------------------------------------------ the masks
def blobs(h, w, seed, specks=0.02):
    """seeded discs with holes and specks (`specks`: the share of pixels flipped)"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:h, :w]
    p = np.zeros((h, w), dtype=bool)
    top = max(1.5, min(h, w) / 4)
    for _ in range(5):
        cy, cx, r = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(top / 2, top)
        p |= (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
    for _ in range(6):
        cy, cx, r = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(0, top / 3)
        p &= ~((yy - cy) ** 2 + (xx - cx) ** 2 <= r * r)
    return (p ^ (rng.random((h, w)) < specks)).astype(np.uint8)


def corners(h, w):
    p = np.zeros((h, w), dtype=np.uint8)
    p[0, 0] = p[0, -1] = p[-1, 0] = p[-1, -1] = 1
    return p


def mid_column_run(h, w):
    """one run of ones from the middle of column 1 to the middle of column w - 2: it covers the columns between whole"""
    assert h >= 2 and w >= 4
    return [h + h // 2, (w - 3) * h, h * w - (h + h // 2) - (w - 3) * h]


def zero_counts(h, w):
    """zero counts at the front, twice in a row in the middle and at the end: the ones are the first half of the scan"""
    return [0, h * w // 2, 0, 0, h * w - h * w // 2, 0]


@functools.lru_cache(maxsize=None)
def row(h, w):
    """-> (names, counts of every mask): the case table of one geometry"""
    yy, xx = np.mgrid[:h, :w]
    table = [('empty', [h * w]),
             ('full', [0, h * w]),
             ('corners', counts_of(corners(h, w))),
             ('checkerboard', [1] * (h * w)),            # the value is the parity of the scan position: every count is 1
             ('column-stripes', [h] * w),                 # every boundary on a column boundary
             ('row-stripes', counts_of(yy & 1)),
             ('blobs-1', counts_of(blobs(h, w, 1))),
             ('blobs-2', counts_of(blobs(h, w, 2))),
             ('zero-counts', zero_counts(h, w))]
    if 'crosses-columns' in claims(h, w):
        table.insert(6, ('mid-column-run', mid_column_run(h, w)))
    names, all_counts = [n for n, _ in table], [c for _, c in table]
    assert all(valid(c, h, w) for c in all_counts)
    return names, all_counts


OUTCOMES = ('empty', 'full', 'corners', 'every-count-1', 'runs-end-on-columns', 'row-stripes', 'crosses-columns', 'zero-first',
            'zero-twice-inside', 'zero-last')


def claims(h, w):
    """the outcomes a row of this geometry must hold: a run that starts inside a column and covers two whole ones needs
    columns of two pixels and four of them; anything else fits one pixel"""
    out = set(OUTCOMES)
    if h < 2 or w < 4:
        out.discard('crosses-columns')
    return out


def outcomes(counts, h, w):
    """the outcomes of OUTCOMES that this mask shows, read off its counts and its plane"""
    c = np.asarray(counts, dtype=np.int64)
    p = plane(c, h, w)
    yy, _ = np.mgrid[:h, :w]
    found = set()
    if not p.any():
        found.add('empty')
    if p.all():
        found.add('full')
    if p[0, 0] and p[0, -1] and p[-1, 0] and p[-1, -1] and p.sum() == len({(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)}):
        found.add('corners')
    if c.size == h * w and (c == 1).all():
        found.add('every-count-1')
    if c.size == w and (c == h).all():
        found.add('runs-end-on-columns')
    if np.array_equal(p, yy & 1):
        found.add('row-stripes')
    starts = np.cumsum(c) - c
    ones = (np.arange(c.size) & 1 == 1) & (c > 0)
    if (ones & (starts % h != 0) & ((starts + c - 1) // h - starts // h >= 3)).any():
        found.add('crosses-columns')
    if c[0] == 0:
        found.add('zero-first')
    if c.size >= 4 and ((c[1:-2] == 0) & (c[2:-1] == 0)).any():
        found.add('zero-twice-inside')
    if c.size >= 2 and c[-1] == 0:
        found.add('zero-last')
    return found


def check_row(h, w):
    names, all_counts = row(h, w)
    found = set()
    for c in all_counts:
        found |= outcomes(c, h, w)
    return found


@functools.lru_cache(maxsize=None)
def _as_rles(h, w, key):
    out = []
    for k, c in enumerate(key):
        if len(c) > 50000:        # (the string encoder of the tests is a loop over counts)
            out.append({'size': [h, w], 'counts': list(c)})
            continue
        text = coco_string(c)
        out.append({'size': [h, w], 'counts': (text, text.encode('ascii'), list(c))[k % 3]})
    return out


def as_rles(all_counts, h, w):
    """the forms a caller may hand in, taken in turn: a dict with the compressed text, with bytes, with the bare list
    (the list alone for a mask of very many runs)"""
    return list(_as_rles(h, w, tuple(tuple(int(v) for v in c) for c in all_counts)))
