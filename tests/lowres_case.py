"""TEST-ONLY statement of rules L1-L6 of include/deva_lowres.h in numpy fp32, and the case generator of the low-resolution
tests.  Written from the rules, one line per rule, NOT from segment_anything's or ATen's code: every operation below is a
single rounded fp32 numpy operation in the order the header writes it, so the device must agree bit for bit.  Each
output pixel is evaluated from its own taps (gathers), vectorised over the plane.

`ATEN_BOUND` is the measured distance of this statement from ATen's chain on the CPU; how it was obtained stands beside it."""
import numpy as np
import torch
import torch.nn.functional as TF

F = np.float32

# Worst |statement - F.interpolate(F.interpolate(low, (M, M))[..., :IH, :IW], (OH, OW))| on the CPU over `ATEN_CASES` with
# the generator's finite planes, as printed by
#     python tests/lowres_case.py
# (ATen's vectorised CPU code and the statement round the source index differently: the difference is in the weights'
# last bits, times logits of up to a few tens).  The tests assert 4 x this value -- the factor covers other seeds and the
# device's contracted multiply-adds in ATen, not an error in L2 -- and hold the bytes equal wherever ATen's value is
# further than that from the threshold.
ATEN_BOUND = 3.5e-5      # (measured 3.421e-05, at 256 x 256 -> 1024 -> 1080 x 1920, seed 2)
ATEN_FACTOR = 4.0
ATEN_EXCUSED_MAX = 0.01   # at most this share of the pixels may lie within the bound of the threshold
# (low, model_size, input_size, size)
ATEN_CASES = [((16, 16), 64, (36, 64), (33, 70)), ((16, 16), 64, (36, 64), (65, 129)), ((16, 16), 64, (36, 64), (5, 9)),
              ((64, 64), 256, (144, 256), (270, 480)), ((64, 64), 256, (256, 144), (480, 270)),
              ((256, 256), 1024, (576, 1024), (1080, 1920)), ((256, 256), 1024, (1024, 576), (1920, 1080)),
              ((256, 256), 1024, (576, 1024), (480, 854))]


def axis(n_in, n_out):
    """L1 for every destination index of one axis -> i0, i1 (int64), l0, l1 (fp32)"""
    scale = F(n_in) / F(n_out)
    d = np.arange(n_out, dtype=F)
    s = np.maximum(scale * (d + F(0.5)) - F(0.5), F(0.0))
    i0 = np.minimum(s.astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    l1 = s - i0.astype(F)
    l0 = F(1.0) - l1
    assert s.dtype == F and l1.dtype == F and l0.dtype == F
    return i0, i1, l0, l1


def resize(src, n_in, n_out):
    """L2 for every destination pixel: src [..., >= n_in[0], >= n_in[1]] fp32 -> [..., n_out[0], n_out[1]]; the taps are
    gathered per pixel from src[..., :n_in[0], :n_in[1]]"""
    y0, y1, l0y, l1y = axis(n_in[0], n_out[0])
    x0, x1, l0x, l1x = axis(n_in[1], n_out[1])
    a, b = src[..., y0[:, None], x0[None, :]], src[..., y0[:, None], x1[None, :]]
    c, d = src[..., y1[:, None], x0[None, :]], src[..., y1[:, None], x1[None, :]]
    with np.errstate(invalid='ignore', over='ignore'):                                   # L4: IEEE, 0 * inf is NaN
        v = l0y[:, None] * (l0x[None, :] * a + l1x[None, :] * b) + l1y[:, None] * (l0x[None, :] * c + l1x[None, :] * d)
    assert v.dtype == F
    return v


def upsample(low, model_size, input_size, size):
    """L3: low fp32 [..., LH, LW] -> fp32 [..., OH, OW].  Only mid[:IH, :IW] is ever read, so only that is formed."""
    low = np.ascontiguousarray(low, dtype=F)
    ih, iw = input_size
    y0, y1, l0y, l1y = axis(low.shape[-2], model_size)
    x0, x1, l0x, l1x = axis(low.shape[-1], model_size)
    y0, y1, l0y, l1y = y0[:ih], y1[:ih], l0y[:ih], l1y[:ih]
    x0, x1, l0x, l1x = x0[:iw], x1[:iw], l0x[:iw], l1x[:iw]
    a, b = low[..., y0[:, None], x0[None, :]], low[..., y0[:, None], x1[None, :]]
    c, d = low[..., y1[:, None], x0[None, :]], low[..., y1[:, None], x1[None, :]]
    with np.errstate(invalid='ignore', over='ignore'):
        mid = l0y[:, None] * (l0x[None, :] * a + l1x[None, :] * b) + l1y[:, None] * (l0x[None, :] * c + l1x[None, :] * d)
    assert mid.dtype == F
    return resize(mid, (ih, iw), size)


def choice(scores):
    """S1: numpy's argmax per box (the first NaN, else the first maximum)"""
    return np.argmax(np.asarray(scores, dtype=F), axis=1).astype(np.int32)


def select(low, scores, model_size, input_size, size, threshold=0.0):
    """L6: low [B,M,LH,LW], scores [B,M] or None -> (bytes [B,OH,OW], chosen int32 [B]); only the chosen planes are formed"""
    low = np.asarray(low, dtype=F)
    chosen = np.zeros(low.shape[0], dtype=np.int32) if scores is None else choice(scores)
    planes = upsample(low[np.arange(low.shape[0]), chosen], model_size, input_size, size) if low.shape[0] else \
        np.zeros((0,) + tuple(size), dtype=F)
    return (planes > F(threshold)).astype(np.uint8), chosen


def aten_chain(low, model_size, input_size, size):
    """the segmenter's `postprocess_masks` with ATen on the tensor's device: low torch fp32 [B,LH,LW] -> [B,OH,OW]"""
    x = TF.interpolate(low[:, None], (model_size, model_size), mode='bilinear', align_corners=False)
    x = x[..., :input_size[0], :input_size[1]]
    return TF.interpolate(x, tuple(size), mode='bilinear', align_corners=False)[:, 0]


# ------------------------------------------------------------------------------------------ the case generator
def smooth_logits(seed, planes, low_size, scale=8.0):
    """smooth random low-resolution logits, fp32 [planes, LH, LW]: a coarse N(0, scale^2) field, blurred, plus a per-plane
    offset so that the planes' stability scores spread over both sides of a threshold"""
    rng = np.random.default_rng(seed)
    lh, lw = low_size
    ch, cw = max(2, lh // 4 + 1), max(2, lw // 4 + 1)
    coarse = rng.normal(0.0, scale, size=(planes, ch, cw))
    ys, xs = np.linspace(0, ch - 1, lh), np.linspace(0, cw - 1, lw)
    y0, x0 = np.minimum(ys.astype(int), ch - 2), np.minimum(xs.astype(int), cw - 2)
    fy, fx = (ys - y0)[None, :, None], (xs - x0)[None, None, :]
    field = ((1 - fy) * (1 - fx) * coarse[:, y0][:, :, x0] + (1 - fy) * fx * coarse[:, y0][:, :, x0 + 1] +
             fy * (1 - fx) * coarse[:, y0 + 1][:, :, x0] + fy * fx * coarse[:, y0 + 1][:, :, x0 + 1])
    field += rng.normal(0.0, scale / 4, size=(planes, 1, 1)) + rng.normal(0.0, 0.05, size=field.shape)
    return np.ascontiguousarray(field, dtype=F)


def with_specials(low, seed):
    """planes of NaN and of +-inf mixed in: plane 1 all NaN, plane 2 a patch of +inf, plane 3 a patch of -inf and one NaN
    (where there are that many planes); the patches start in the top left quarter, inside every crop of the tests"""
    low = low.copy()
    rng = np.random.default_rng(seed + 1000)
    n, lh, lw = low.shape
    if n > 1:
        low[1] = np.nan
    if n > 2:
        y, x = rng.integers(0, max(1, lh // 4)), rng.integers(0, max(1, lw // 4))
        low[2, y:y + max(1, lh // 3), x:x + max(1, lw // 3)] = np.inf
    if n > 3:
        y, x = rng.integers(0, max(1, lh // 4)), rng.integers(0, max(1, lw // 4))
        low[3, y:y + max(1, lh // 4), x:x + max(1, lw // 4)] = -np.inf
        low[3, max(0, lh // 2 - 1), max(0, lw // 2 - 1)] = np.nan
    return low


def logits(seed, planes, low_size, specials=True):
    low = smooth_logits(seed, planes, low_size)
    return with_specials(low, seed) if specials else low


def iou_preds(seed, planes):
    """predicted IoUs on both sides of 0.88, with a NaN and ties"""
    rng = np.random.default_rng(seed + 2000)
    iou = rng.uniform(0.80, 1.0, size=planes).astype(F)
    if planes > 4:
        iou[4] = np.nan
    if planes > 6:
        iou[6] = iou[5]
    return iou


def aten_difference(case, seed=0, planes=3):
    """-> (worst |statement - ATen|, share of ATen's values within ATEN_FACTOR * ATEN_BOUND of 0) on finite planes"""
    low_size, m, input_size, size = case
    low = smooth_logits(seed, planes, low_size)
    ours = upsample(low, m, input_size, size)
    aten = aten_chain(torch.from_numpy(low), m, input_size, size).numpy()
    return float(np.abs(ours - aten).max()), float((np.abs(aten) <= ATEN_FACTOR * ATEN_BOUND).mean())


if __name__ == '__main__':
    worst = 0.0
    for case in ATEN_CASES:
        for seed in range(3):
            diff, near = aten_difference(case, seed)
            worst = max(worst, diff)
            print(case, 'seed', seed, f'worst |statement - ATen| = {diff:.3e}, within the bound of 0: {near:.2e} of the pixels')
    print(f'worst = {worst:.3e}')
