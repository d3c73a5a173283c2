"""TEST-ONLY statement of the region rules (include/deva_regions.h, R1-R7) in numpy and plain Python, and the planes the
region tests run on, shared by the CPU and the GPU side.

`labels(kind)` is a run-based union-find: the runs of every row, united with the runs of the row above that they touch
(8-connectivity: a run [s, e) touches [s', e') when s <= e' and s' <= e), the smaller run index winning, so that a
component's root is the run that holds its first pixel in row-major order.  `clean(plane, min_area)` is R2 then R3 on top
of it, one numpy line per sentence of the rules.  Nothing here comes from OpenCV, scipy or scikit-image (none of which the
GPU box need have); tests/test_regions_cpu.py holds the statement against scipy where that is installed.

The patterns are named for what they do to a tiled labelling: chains that cross every tile edge many times (serpentine,
spiral), merges that arrive late (comb), components that exist only through diagonal steps (checkerboard, diagonals,
`diag_touch`), and the degenerate planes.  `kinds(h, w, min_area)` builds one plane per outcome of the clean-up; thresholded
noise would not: nearly every noisy plane is changed by both passes."""
import functools

import numpy as np

KINDS = ('unchanged', 'only-filled', 'only-removed', 'keep-largest', 'both')


# ------------------------------------------------------------------------------------------ the statement
def labels(kind):
    """bool [H,W] -> int32 [H,W]: 0 where `kind` is False, else 1 + the smallest y * W + x of the pixel's 8-connected component"""
    kind = np.asarray(kind, dtype=bool)
    h, w = kind.shape
    padded = np.zeros((h, w + 2), dtype=np.int8)
    padded[:, 1:-1] = kind
    step = np.diff(padded, axis=1)
    ys, starts = np.nonzero(step == 1)          # runs in row-major order of their first pixel
    ends = np.nonzero(step == -1)[1]            # exclusive
    n = len(ys)
    parent = list(range(n))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    first = np.searchsorted(ys, np.arange(h + 1))       # the runs of row y are first[y] .. first[y + 1]
    s, e = starts.tolist(), ends.tolist()
    for y in range(1, h):
        a, a_end, b, b_end = first[y - 1], first[y], first[y], first[y + 1]
        while a < a_end and b < b_end:
            if s[a] <= e[b] and s[b] <= e[a]:
                ra, rb = find(a), find(b)
                if ra != rb:
                    parent[max(ra, rb)] = min(ra, rb)
            if e[a] < e[b]:        # the run that ends first cannot touch a later run of the other row
                a += 1
            else:
                b += 1
    root = np.array([find(i) for i in range(n)], dtype=np.int64)
    out = np.zeros(h * w, dtype=np.int32)
    if n:
        value = (ys[root] * w + starts[root] + 1).astype(np.int32)
        length = ends - starts
        begin = np.repeat(ys * w + starts, length)
        within = np.arange(length.sum()) - np.repeat(np.cumsum(length) - length, length)
        out[begin + within] = np.repeat(value, length)
    return out.reshape(h, w)


def components(lab):
    """labels -> (roots ascending, areas): a root is the label of a component, 1 + its first pixel"""
    roots, areas = np.unique(lab[lab > 0], return_counts=True)
    return roots, areas


def box_of(mask):
    ys, xs = np.nonzero(mask)
    return (int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max())) if len(xs) else (0, 0, 0, 0)


def clean_steps(plane, min_area):
    """-> (plane uint8 0 / 1, record int32 [8], what happened: dict of holes_small, islands_small, all_small)"""
    assert min_area > 0                                                     # R6
    mask = np.asarray(plane) != 0                                           # R1
    roots, areas = components(labels(~mask))                                # R2: the complement, 8-connected
    small = roots[areas < min_area]
    fill = np.isin(labels(~mask), small) if len(small) else np.zeros_like(mask)
    holes_small = len(small) > 0
    mask = mask | fill
    lab = labels(mask)                                                      # R3: on the result of R2
    roots, areas = components(lab)
    small = areas < min_area
    islands_small, all_small = bool(small.any()), bool(small.any() and small.all())
    if not islands_small:
        remove = np.zeros_like(mask)
    elif all_small:
        remove = (lab > 0) & (lab != roots[np.argmax(areas)])               # the largest; among equals the first in row-major order
    else:
        remove = np.isin(lab, roots[small])
    mask = mask & ~remove
    record = np.array([int(holes_small or islands_small), fill.sum(), remove.sum(), mask.sum(), *box_of(mask)], dtype=np.int32)   # R4, R5
    return mask.astype(np.uint8), record, dict(holes_small=holes_small, islands_small=islands_small, all_small=all_small)


def clean(planes, min_area):
    """uint8 [K,H,W] or [H,W] -> (planes 0 / 1, records int32 [K,8] or [8])"""
    planes = np.asarray(planes)
    if planes.ndim == 2:
        out, record, _ = clean_steps(planes, min_area)
        return out, record
    done = [clean_steps(p, min_area) for p in planes]
    return (np.stack([d[0] for d in done]) if done else np.zeros(planes.shape, np.uint8),
            np.stack([d[1] for d in done]) if done else np.zeros((0, 8), np.int32))


def label_planes(planes, of_zeros=False):
    planes = np.asarray(planes)
    if planes.ndim == 2:
        return labels((planes != 0) != bool(of_zeros))
    return np.stack([labels((p != 0) != bool(of_zeros)) for p in planes]) if len(planes) else np.zeros(planes.shape, np.int32)


def kind_of(plane, min_area):
    """which of KINDS the clean-up of this plane is (asked of the statement alone)"""
    _, _, did = clean_steps(plane, min_area)
    if did['holes_small'] and did['islands_small']:
        return 'both'
    if did['holes_small']:
        return 'only-filled'
    if did['islands_small']:
        return 'keep-largest' if did['all_small'] else 'only-removed'
    return 'unchanged'


# ------------------------------------------------------------------------------------------ the patterns
def serpentine(h, w):
    """one pixel wide: every second row full, joined to the next at alternating ends"""
    p = np.zeros((h, w), dtype=np.uint8)
    p[::2] = 1
    for k, y in enumerate(range(1, h, 2)):
        p[y, -1 if k % 2 == 0 else 0] = 1
    return p


def comb(h, w):
    """teeth in every second column that join only in the last row"""
    p = np.zeros((h, w), dtype=np.uint8)
    p[:, ::2] = 1
    p[-1] = 1
    return p


def spiral(h, w):
    """a square spiral one pixel wide with one pixel between its arms"""
    p = np.zeros((h, w), dtype=np.uint8)
    top, left, bottom, right = 0, 0, h - 1, w - 1
    y, x = 0, 0
    p[0, 0] = 1
    moves = ((0, 1), (1, 0), (0, -1), (-1, 0))
    turn = 0
    while top <= bottom and left <= right:
        dy, dx = moves[turn % 4]
        moved = False
        while top <= y + dy <= bottom and left <= x + dx <= right:
            y, x = y + dy, x + dx
            p[y, x] = 1
            moved = True
        if turn % 4 == 0:
            top += 2
        elif turn % 4 == 1:
            right -= 2
        elif turn % 4 == 2:
            bottom -= 2
        else:
            left += 2
        turn += 1
        if not moved and turn > 4:
            break
    return p


def checkerboard(h, w):
    yy, xx = np.mgrid[:h, :w]
    return ((yy + xx) % 2 == 0).astype(np.uint8)


def diagonals(h, w):
    """diagonal lines with two pixels between them"""
    yy, xx = np.mgrid[:h, :w]
    return ((yy + xx) % 3 == 0).astype(np.uint8)


def diag_touch(h, w, corner, orientation):
    """two blocks (3 x 3 and 2 x 4) whose only contact is the diagonal step across the grid corner `corner` = (y, x): the
    3 x 3 block lies in quadrant `orientation` (0 NW, 1 NE, 2 SW, 3 SE) of it, the other in the opposite one"""
    p = np.zeros((h, w), dtype=np.uint8)
    cy, cx = corner

    def block(quadrant, bh, bw):
        y0, y1 = (cy - bh, cy) if quadrant in (0, 1) else (cy, cy + bh)
        x0, x1 = (cx - bw, cx) if quadrant in (0, 2) else (cx, cx + bw)
        p[max(y0, 0):max(y1, 0), max(x0, 0):max(x1, 0)] = 1
    block(orientation, 3, 3)
    block(3 - orientation, 2, 4)
    return p


def blobs(h, w, seed):
    """discs with holes in them and specks between them"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:h, :w]
    p = np.zeros((h, w), dtype=bool)
    top = max(2.0, min(h, w) / 5)
    for _ in range(6):
        cy, cx, r = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(top / 2, top)
        p |= (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
    for _ in range(10):                                   # holes, from a pixel to a small disc
        cy, cx, r = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(0, top / 3)
        p &= ~((yy - cy) ** 2 + (xx - cx) ** 2 <= r * r)
    specks = rng.random((h, w)) < 0.01
    return (p ^ specks).astype(np.uint8)                  # a speck outside is an island, inside a pinhole


def empty(h, w):
    return np.zeros((h, w), dtype=np.uint8)


def full(h, w):
    return np.ones((h, w), dtype=np.uint8)


def full_minus_corner(h, w):
    p = full(h, w)
    p[-1, -1] = 0
    return p


PATTERNS = {'serpentine': serpentine, 'comb': comb, 'spiral': spiral, 'checkerboard': checkerboard, 'diagonals': diagonals,
            'blobs': lambda h, w: blobs(h, w, 7 * h + w), 'empty': empty, 'full': full, 'full_minus_corner': full_minus_corner}


def kinds(h, w, min_area):
    """name -> plane, one per outcome (KINDS), from solid shapes: a block with a hole of min_area pixels and a far island of
    min_area pixels is unchanged; a pinhole, a speck or both make the other outcomes; specks alone keep the largest.
    Needs h >= 7 and w >= 2 * min_area + 10."""
    m = min_area
    assert h >= 7 and w >= 2 * m + 10 and m >= 3, (h, w, m)
    base = np.zeros((h, w), dtype=np.uint8)
    base[1:h - 1, 1:m + 5] = 1                 # the block: 5 rows or more of m + 4
    base[2, 2:2 + m] = 0                       # a hole of exactly min_area
    base[1, m + 7:2 * m + 7] = 1               # an island of exactly min_area, two columns away
    out = {'unchanged': base}
    pin = base.copy()
    pin[4, 3] = 0                              # a pinhole
    speck = base.copy()
    speck[h - 2, w - 2] = 1                    # a speck far from everything
    both = pin.copy()
    both[h - 2, w - 2] = 1
    alone = np.zeros((h, w), dtype=np.uint8)   # three islands, all small, the two largest equal: the first one stays
    alone[1, 1:3] = 1
    alone[h - 2, 1:3] = 1
    alone[3, w - 2] = 1
    out.update({'only-filled': pin, 'only-removed': speck, 'both': both, 'keep-largest': alone})
    return out


# (H, W, min_area) -> planes by hand where `kinds` does not fit: one row, one column, one 2 x 2 neighbourhood
TINY = {
    (1, 9): (2, {'unchanged': '111100000', 'only-filled': '110111111', 'only-removed': '110000100', 'keep-largest': '100010000',
                 'both': '101100100'}),
    (2, 2): (2, {'unchanged': '11/00', 'only-filled': '11/10', 'keep-largest': '10/00'}),
}


def _parse(text):
    return np.array([[int(c) for c in row] for row in text.split('/')], dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def row(h, w, tile=32):
    """the planes of one geometry row of the GPU test, read-only -> (names, planes uint8 [K,h,w], min_area): every pattern,
    the diagonal pair across every tile corner in all four orientations, one plane per outcome"""
    named = [(name, make(h, w)) for name, make in PATTERNS.items()]
    corners = [(y, x) for y in range(tile, h, tile) for x in range(tile, w, tile)] or [(h // 2, w // 2)]
    if min(h, w) >= 8:
        named += [(f'diag_touch{c}/{o}', diag_touch(h, w, c, o)) for c in corners for o in range(4)]
    if (h, w) in TINY or (w, h) in TINY:
        min_area, by_hand = TINY.get((h, w)) or TINY[(w, h)]
        for kind, text in by_hand.items():
            plane = _parse(text)
            named.append((kind, plane if plane.shape == (h, w) else plane.T.copy()))
    else:
        min_area = 6 if w < 34 else 12
        named += list(kinds(h, w, min_area).items())
    names = tuple(n for n, _ in named)
    planes = np.stack([p for _, p in named])
    planes.setflags(write=False)
    return names, planes, min_area


@functools.lru_cache(maxsize=None)
def expected(h, w, tile=32):
    """(cleaned planes, records, labels of the mask, labels of the complement) of `row(h, w)` by the statement, computed once"""
    _, planes, min_area = row(h, w, tile)
    out = clean(planes, min_area) + (label_planes(planes), label_planes(planes, of_zeros=True))
    for a in out:
        a.setflags(write=False)
    return out


def check_row(h, w, tile=32):
    """the row holds every outcome that its size allows (asserted on the statement alone) -> the outcomes present"""
    names, planes, min_area = row(h, w, tile)
    present = {kind_of(p, min_area) for p in planes}
    want = set(KINDS) - ({'only-removed', 'both'} if (h, w) == (2, 2) else set())
    for name, p in zip(names, planes):
        if name in KINDS:
            assert kind_of(p, min_area) == name, (h, w, name, kind_of(p, min_area))
    assert want <= present, (h, w, want - present)
    return present
