"""TEST-ONLY CPU contracts of the per-frame result ops of `deva.hip.ops` (`frame_result`, `mask_rle`), in the manner of
tests/emu_ensemble.py: plain PyTorch / numpy, the executable statement of what each HIP kernel must compute.
`install(monkeypatch)` patches them over the ctypes wrappers (next to `emu_ops.install`).

Also the test side's COCO run-length encoder and decoder, written as straightforward loops over the algorithm of the
COCO API's rleToString / rleFrString (5 bits per character, low bits first, 0x20 marks continuation, sign-aware
termination, 48 added; from the third count on the difference to the count two places back is coded): the executable
specification the product's vectorised encoder is held against."""
import numpy as np
import torch

import emu_ops
from deva.hip import ops as real

INT_MAX = 2**31 - 1


# ------------------------------------------------------------------------------------------ everything after the argmax
def products_from_index(index, channels, lut=None, color_lut=None, image=None, want=real.FRAME_PRODUCTS):
    """the contract downstream of the channel decision: `index` (integer [OH,OW] array / tensor of channel indices) ->
    dict of numpy arrays for the products in `want`"""
    idx = np.asarray(index.cpu() if torch.is_tensor(index) else index).astype(np.int64)
    oh, ow = idx.shape
    if lut is None:
        ids = idx.copy()
    else:
        table = np.asarray(lut.cpu() if torch.is_tensor(lut) else lut).astype(np.int64)
        ids = np.where(idx < len(table), table[np.minimum(idx, len(table) - 1)], 0)
    out = {}
    if 'index' in want:
        out['index'] = idx.astype(np.int16)
    if 'labels' in want:
        out['labels'] = ids
    if 'stats' in want:
        stats = np.zeros((channels, 5), dtype=np.int32)
        stats[:, 1:3], stats[:, 3:5] = INT_MAX, -1
        for c in np.unique(idx).tolist():   # the channels that are present: an absent one keeps the empty pattern
            ys, xs = np.nonzero(idx == c)
            stats[c] = (len(ys), xs.min(), ys.min(), xs.max(), ys.max())
        out['stats'] = stats
    if 'gray' in want:
        out['gray'] = (ids & 0xff).astype(np.uint8)
    if 'color' in want or 'blend' in want:
        colors = np.asarray(color_lut.cpu() if torch.is_tensor(color_lut) else color_lut).astype(np.uint8)
        rgb = colors[idx]
        if 'color' in want:
            out['color'] = rgb
        if 'blend' in want:
            img = np.asarray(image.cpu() if torch.is_tensor(image) else image).astype(np.uint8)
            half = ((img.astype(np.int32) + rgb.astype(np.int32)) >> 1).astype(np.uint8)
            out['blend'] = np.where((ids == 0)[:, :, None], img, half)
    return out


def frame_result(prob, size=None, lut=None, *, color_lut=None, image=None, want=('index', 'labels', 'stats'),
                 out=None):
    want = tuple(want)
    c = prob.shape[0]
    oh, ow = tuple(prob.shape[-2:]) if size is None else (int(size[0]), int(size[1]))
    if 'blend' in want and (image is None or tuple(image.shape) != (oh, ow, 3)):
        raise real.DevaHipError('frame_result: blend needs a uint8 image of the output size')
    if 'index' in want and c > 32767:
        raise real.DevaHipError('frame_result: the int16 index plane holds at most 32767 channels')
    idx = emu_ops.index_mask(prob.float(), size)
    made = products_from_index(idx, c, lut, color_lut, image, want)
    res = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in made.items()}
    if out is not None:
        for k, t in out.items():
            if k in res and t is not None:
                t.copy_(res[k])
                res[k] = t
    return real.FrameProducts(**res)


# ------------------------------------------------------------------------------------------ run boundaries
def rle_bounds(index, channels):
    """-> (n int32 [channels], [bounds_c for c in range(channels)]): per channel c >= 1 the ascending column-major
    positions p with (index[p] == c) != (index[p-1] == c), the label before p = 0 being "no object" """
    idx = np.asarray(index.cpu() if torch.is_tensor(index) else index).astype(np.int64)
    flat = idx.T.reshape(-1)   # p = x * OH + y
    n, bounds = np.zeros(channels, dtype=np.int32), [np.zeros(0, dtype=np.int32)]
    for c in range(1, channels):
        m = (flat == c).astype(np.int8)
        b = np.nonzero(np.diff(np.concatenate([[0], m])))[0].astype(np.int32)
        n[c] = len(b)
        bounds.append(b)
    return n, bounds


def rle_bounds_fast(index, channels):
    """`rle_bounds` without the loop over channels, for tables of thousands of them -> (n int32 [channels], the lists
    back to back, int32): at every position p where the object label of the column-major plane changes (values outside
    1..channels-1 read as 0, and so does the label before p = 0) the run of `prev` ends and the run of `cur` starts, so
    (prev, p) and (cur, p) are emitted for the non-zero ones in position order; a stable sort by channel then leaves
    every channel's positions ascending.  Held equal to `rle_bounds` by tests/test_frame_result_cpu.py."""
    idx = np.asarray(index.cpu() if torch.is_tensor(index) else index).astype(np.int64)
    flat = idx.T.reshape(-1)
    obj = np.where((flat >= 1) & (flat < channels), flat, 0)
    prev = np.concatenate([[0], obj[:-1]])
    at = np.nonzero(obj != prev)[0]
    label = np.stack([prev[at], obj[at]], axis=1).reshape(-1)   # (prev, cur) of each transition, in position order
    where = np.repeat(at, 2)
    keep = label != 0
    label, where = label[keep], where[keep]
    order = np.argsort(label, kind='stable')
    return np.bincount(label, minlength=channels).astype(np.int32), where[order].astype(np.int32)


def mask_rle(index, channels=None):
    c = int(index.max()) + 1 if channels is None else int(channels)
    if c > 2048:   # (the loop over channels takes a quarter of a minute at 4096 of them on half a million positions)
        n, bounds = rle_bounds_fast(index, c)
        return torch.from_numpy(n), torch.from_numpy(bounds)
    n, bounds = rle_bounds(index, c)
    return torch.from_numpy(n), torch.from_numpy(np.concatenate(bounds).astype(np.int32))


# ------------------------------------------------------------------------------------------ COCO strings, by loops
def coco_counts(mask):
    """bool [H,W] -> run lengths of the column-major scan, starting with the run of zeros (possibly empty)"""
    flat = np.asarray(mask).astype(bool).T.reshape(-1)
    counts, last, run = [], False, 0
    for v in flat:
        if v != last:
            counts.append(run)
            run, last = 0, v
        run += 1
    counts.append(run)
    return counts


def coco_string(counts):
    out = []
    for i, cnt in enumerate(counts):
        x = int(cnt)
        if i > 2:
            x -= int(counts[i - 2])
        more = True
        while more:
            c = x & 0x1f
            x >>= 5
            more = (x != -1) if (c & 0x10) else (x != 0)
            if more:
                c |= 0x20
            out.append(chr(c + 48))
    return ''.join(out)


def coco_parse(text):
    counts, p = [], 0
    while p < len(text):
        x, k, more = 0, 0, True
        while more:
            c = ord(text[p]) - 48
            x |= (c & 0x1f) << (5 * k)
            more = bool(c & 0x20)
            p += 1
            k += 1
            if not more and (c & 0x10):
                x |= -1 << (5 * k)
        if len(counts) > 2:
            x += counts[-2]
        counts.append(x)
    return counts


def coco_decode(rle):
    """{'size': [H, W], 'counts': str} -> bool [H,W]"""
    h, w = rle['size']
    flat, p, v = np.zeros(h * w, dtype=bool), 0, False
    for cnt in coco_parse(rle['counts']):
        assert cnt >= 0 and p + cnt <= h * w, (cnt, p)
        flat[p:p + cnt] = v
        p, v = p + cnt, not v
    assert p == h * w, (p, h * w)
    return flat.reshape(w, h).T


def coco_encode(mask):
    h, w = np.asarray(mask).shape
    return {'size': [int(h), int(w)], 'counts': coco_string(coco_counts(mask))}


def install(monkeypatch):
    for name in ('frame_result', 'mask_rle'):
        monkeypatch.setattr(real, name, globals()[name])
