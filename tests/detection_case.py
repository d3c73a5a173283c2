"""The detector output the assembly tests run on (tests/test_detections_cpu.py, tests/test_gpu_p_detections.py) and
that tests/golden/make_detection_golden.py feeds to the reference's own auto_segment / segment_with_text.  Built from
coordinates and seeds: no mask data is committed.

The layout is a 4 x 4 grid of cells, drawn on a 24 x 36 canvas and scaled to the size asked for:
  R0..R7  eight disjoint rectangles of distinct areas; R6 and R7 lie inside
  L       a mask over four cells, which eats R6 and R7 when large masks win and loses them when small ones do
  Z       an all-zero mask in the middle of the list: from here on the uncompacted index and the compacted id differ
  A1, B1  B1 overlaps the larger A1 with a tenth of its pixels: it keeps 0.9 of them, above the threshold of 0.8
  A2, B2  B2 keeps 0.6 of its pixels: below
  T, U    T has exactly 10 pixels at every size and loses exactly 3 to the larger U: 7 / 10 against a threshold of 0.7,
          where an fp32 evaluation (0.7f < 0.7f: false, kept) and an fp64 one (0.699999988 < 0.7: true, dropped) disagree
  P       a single pixel
  D       an exact duplicate of R1, later in the list: the first maximum goes to R1
`extra` random rectangles from the seed follow (many masks, many overlaps)."""
import numpy as np
import torch

NAMES = ('R0', 'R1', 'R2', 'R3', 'R4', 'R5', 'R6', 'R7', 'L', 'Z', 'A1', 'B1', 'A2', 'B2', 'T', 'U', 'P', 'D')
# (y0, y1, x0, x1) on the 24 x 36 canvas, end exclusive
RECTS = {
    'R0': (1, 5, 1, 8), 'R1': (0, 6, 10, 17), 'R2': (1, 6, 19, 26), 'R3': (1, 5, 28, 36),
    'R4': (7, 12, 0, 9), 'R5': (6, 11, 10, 16),
    'R6': (13, 17, 1, 7), 'R7': (13, 16, 10, 16), 'L': (12, 24, 0, 18),
    'A1': (12, 18, 18, 26), 'B1': (13, 17, 25, 35), 'A2': (18, 24, 18, 28), 'B2': (19, 23, 24, 35),
}
SIZES = (((24, 36), (24, 36)), ((24, 36), (48, 72)), ((30, 45), (20, 30)))   # (mask size, output size) of the goldens
POLICIES = (('suppress', 0.8), ('suppress', 0.7), ('prefer', None), ('text', None))


def masks(h, w, extra=0, seed=0):
    """-> bool [18 + extra, h, w]"""
    assert h >= 23 and w >= 36
    out = torch.zeros(len(NAMES) + extra, h, w, dtype=torch.bool)
    for k, name in enumerate(NAMES):
        if name in RECTS:
            y0, y1, x0, x1 = RECTS[name]
            out[k, y0 * h // 24:y1 * h // 24, x0 * w // 36:x1 * w // 36] = True
    ty, tx = 7 * h // 24, 19 * w // 36            # T and U in absolute pixels from a scaled corner
    out[NAMES.index('T'), ty, tx:tx + 10] = True
    out[NAMES.index('U'), ty:ty + 3, tx + 7:tx + 14] = True
    out[NAMES.index('P'), 11 * h // 24, 35 * w // 36] = True
    out[NAMES.index('D')] = out[NAMES.index('R1')]
    rng = np.random.default_rng(seed)
    for k in range(len(NAMES), len(NAMES) + extra):
        y0, x0 = int(rng.integers(0, h - 2)), int(rng.integers(0, w - 2))
        y1, x1 = int(rng.integers(y0 + 1, min(h, y0 + h // 3) + 1)), int(rng.integers(x0 + 1, min(w, x0 + w // 3) + 1))
        out[k, y0:y1, x0:x1] = True
    return out


def scores(n, seed=0):
    """predicted IoUs of the automatic policies -> fp32 [n]"""
    return torch.from_numpy(np.random.default_rng(seed + 100).random(n).astype(np.float32))


def confidences(n):
    """text policy: in descending order, as they leave the (identity) NMS -> fp32 numpy [n]"""
    return np.linspace(0.95, 0.35, n).astype(np.float32) if n else np.zeros(0, dtype=np.float32)


def class_ids(n, seed=0):
    return np.random.default_rng(seed + 200).integers(0, 5, size=n).astype(np.int64)


def golden_key(policy, threshold, size_in, size_out, n):
    t = '' if threshold is None else f'{threshold}'
    return f'{policy}{t}/{size_in[0]}x{size_in[1]}-{size_out[0]}x{size_out[1]}/n{n}'


MORE = (((23, 37), 18), ((270, 480), 40))   # equal sizes: an odd width; several workgroups and chunks, 22 random masks more


def case_masks(size_in, n):
    return masks(*size_in, extra=max(0, n - len(NAMES)))[:n]


def golden_cases():
    """every (policy, threshold, mask size, output size, number of masks) of the golden file: all 18 masks at the three
    size pairs, none / one mask at equal sizes, and the two larger equal-size cases of `MORE`"""
    for policy, threshold in POLICIES:
        for size_in, size_out in SIZES:
            yield policy, threshold, size_in, size_out, len(NAMES)
        for n in (0, 1):
            yield policy, threshold, SIZES[0][0], SIZES[0][1], n
        # (not the text policy: scaled to 23 x 37 some rectangles tie in area, and numpy's default argsort, which the
        # reference calls, is not the stable one on 18 elements there -- the contract fixes the order among equal areas,
        # the reference leaves it open)
        for size, n in MORE if policy != 'text' else ():
            yield policy, threshold, size, size, n
