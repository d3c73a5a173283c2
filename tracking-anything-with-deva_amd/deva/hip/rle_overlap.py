"""ctypes binding of libdeva_rle_overlap.so (C ABI declared in include/deva_rle_overlap.h): the overlap of every mask of
one list of COCO run-length masks with every mask of another, taken from the run lengths on the device (rules O1-O9 of the
header), and `pycocotools.mask.iou` on top of it.  No plane is decoded: per side the host parses the text
(`rle.parse_checked`), builds the run array of `deva_rle.h` (`rle.run_array`) and from it the boxes (`boxes_and_areas`)
and sends them up in ONE int32 array; two launches follow.  `pycocotools` is not needed.  With `parse='device'` the
texts go up instead and libdeva_rle_text.so builds the run arrays there (`rle.parse_checked`); the host copy that comes
back is checked as ever and gives the boxes, which follow the run array on the device.

The public names are re-exported by `deva.hip.rle` as `rle.intersections` and `rle.iou`.

An eighth library next to libdeva_hip.so, the three scorers, the regions and the two run-length libraries, loaded lazily
by `lib()`; the conventions are those of `deva.hip.rle`: `check` raises `DevaHipError` with the library's text, there is
no CPU path."""
import contextlib
import ctypes
import os
from ctypes import POINTER, Structure, c_char_p, c_int, c_int32, c_int64, c_uint32, c_void_p
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import DevaHipError, _native
from ._pending import out_tensor, record_event, require_on_device, to_pinned
from .ops import _stream

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libdeva_rle_overlap.so')
ABI_VERSION = 1

MAX_MASKS = 65536
MAX_WORDS = 1 << 26
D_CHUNK = 8          # detections a workgroup of the pair pass owns
LDS_RUNS = 1983      # runs of a ground-truth mask that is held in LDS
SCAN_CHUNK = 1024
DT, GT = 0, 1        # DEVA_OVERLAP_DT, DEVA_OVERLAP_GT


class Limits(Structure):
    """mirror of `struct deva_overlap_limits` (include/deva_rle_overlap.h)"""
    _fields_ = [('max_masks', c_int32), ('max_words', c_int32), ('block', c_int32), ('d_chunk', c_int32), ('lds_runs', c_int32),
                ('scan_chunk', c_int32)]


class Plan(Structure):
    """mirror of `struct deva_overlap_plan`"""
    _fields_ = [('scan_grid', c_uint32), ('pair_grid', c_uint32), ('d_chunks', c_int32), ('lds_bytes', c_int32), ('scratch_bytes', c_int64)]


# name -> (restype, argtypes); must list every symbol of include/deva_rle_overlap.h
SIGNATURES = {
    'deva_overlap_version': (c_int, []),
    'deva_overlap_last_error': (c_char_p, []),
    'deva_overlap_limits': (c_int, [POINTER(Limits)]),
    'deva_overlap_plan': (c_int, [c_int, c_int, c_int64, POINTER(Plan)]),
    'deva_overlap_scratch': (c_int64, [c_int64, c_int]),
    'deva_overlap_check': (c_int, [c_void_p, c_int64, c_int, c_int, c_int, c_int]),
    'deva_overlap_intersections': (c_int, [c_void_p, c_void_p, c_int64, c_int, c_void_p, c_void_p, c_int64, c_int, c_int, c_int, c_void_p,
                                           c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p]),
}

_LIB = None


def lib() -> ctypes.CDLL:
    """Load (once) and return the overlap library; raises if it has not been built."""
    return _LIB or _native.load(globals(), 'deva_overlap_version', 'libdeva_rle_overlap.so', 'the run-length overlap')


def check(code: int, what: str) -> None:
    if code != 0:
        _native.check(globals(), code, what, 'deva_overlap_last_error')


def _rle():
    from . import rle   # (that module re-exports this one's public names, so it is imported when first needed)
    return rle


class LimitInfo(NamedTuple):
    max_masks: int    # masks of one side of one call; `intersections` walks more in chunks
    max_words: int    # int32 words of one side's run array: 2 n + 1 + the runs of its n masks
    block: int
    d_chunk: int      # detections a workgroup of the pair pass owns
    lds_runs: int     # a ground-truth mask of at most this many runs is held in LDS
    scan_chunk: int


class PlanInfo(NamedTuple):
    scan_grid: int
    pair_grid: int
    d_chunks: int
    lds_bytes: int
    scratch_bytes: int


def overlap_limits() -> LimitInfo:
    """what one call of the library takes; host only"""
    limits = Limits()
    check(lib().deva_overlap_limits(ctypes.byref(limits)), 'deva_overlap_limits')
    return LimitInfo(*(int(getattr(limits, f[0])) for f in Limits._fields_))


def overlap_plan(d: int, g: int, words_g: int) -> PlanInfo:
    """the launches of one call for `d` detections against `g` ground-truth masks whose run array has `words_g` words;
    host only: no device is touched"""
    plan = Plan()
    check(lib().deva_overlap_plan(int(d), int(g), int(words_g), ctypes.byref(plan)), 'deva_overlap_plan')
    return PlanInfo(*(int(getattr(plan, f[0])) for f in Plan._fields_))


def overlap_scratch(words_g: int, g: int) -> int:
    """bytes of scratch of one call (O8); -1 beyond the limits"""
    return int(lib().deva_overlap_scratch(int(words_g), int(g)))


# ------------------------------------------------------------------------------------------ arguments
def _limits(max_masks, max_words, fn: str) -> Tuple[int, int]:
    top = overlap_limits()
    max_masks = top.max_masks if max_masks is None else int(max_masks)
    max_words = top.max_words if max_words is None else int(max_words)
    if not (1 <= max_masks <= top.max_masks and 4 <= max_words <= top.max_words):
        raise DevaHipError(f'{fn}: limits of 1 to {top.max_masks} masks and 4 to {top.max_words} words (got {max_masks}, {max_words})')
    return max_masks, max_words


def pair_chunks(per_d: np.ndarray, per_g: np.ndarray, max_masks: int, max_words: int,
                fn: str = 'intersections') -> List[Tuple[Tuple[int, int], Tuple[int, int]]]:
    """((d_lo, d_hi), (g_lo, g_hi)) blocks of the D x G table, each side of each within one call's limits (`rle.chunks`
    per side): D-chunk by G-chunk, every pair in exactly one block"""
    rle = _rle()
    parts_d = rle.chunks(np.asarray(per_d), max_masks, max_words, f'{fn}: dt')
    parts_g = rle.chunks(np.asarray(per_g), max_masks, max_words, f'{fn}: gt')
    return [(pd, pg) for pd in parts_d for pg in parts_g]


def _parse_sides(dt: Sequence, gt: Sequence, source_size, fn: str, parse: str = 'host', device=None, limits=(None, None)):
    """both sides parsed and held to O2, on one common size"""
    rle = _rle()
    sides = []
    for name, masks in (('dt', dt), ('gt', gt)):
        if isinstance(masks, (dict, str, bytes)) or not hasattr(masks, '__len__'):
            raise DevaHipError(f'{fn}: {name}: a list of masks expected (got {type(masks).__name__})')
        sides.append(masks)
    size = None if source_size is None else (int(source_size[0]), int(source_size[1]))
    if size is None:                                   # the size of the first dict of either side serves both
        for masks in sides:
            for m in masks:
                if isinstance(m, dict) and 'size' in m and len(m['size']) == 2:
                    size = (int(m['size'][0]), int(m['size'][1]))
                    break
            if size is not None:
                break
    if size is None and not len(sides[0]) and not len(sides[1]):
        size = (1, 1)                                  # nothing on either side: no size is needed
    if (not len(sides[0]) or not len(sides[1])) and parse in rle.PARSE:
        parse = 'host'                                   # (O7 reads the counts of the side that is not empty)
    names = (f'{fn}: dt', f'{fn}: gt')
    if not rle._parse_mode(parse, fn):
        return (rle.parse_checked(sides[0], size, names[0]), rle.parse_checked(sides[1], size, names[1]))
    # both sides are handed to the device before either is waited for; a side that cannot go there is parsed here
    for side in sides:
        if isinstance(side, (dict, str, bytes)) or not hasattr(side, '__len__'):
            return (rle.parse_checked(sides[0], size, names[0]), rle.parse_checked(sides[1], size, names[1]))   # (raises)
    begun = [rle._begin_device_parse(side, size, name, device, limits[0], limits[1], 4) for side, name in zip(sides, names)]
    parsed = [None, None]
    for k, b in enumerate(begun):                        # dt's errors before gt's, as on the host path
        if b is None:
            parsed[k] = rle.parse_checked(sides[k], size, names[k])
        else:
            b.flags_checked()
    waiting = [b for b in begun if b is not None]
    for b in waiting:
        b.pending.fetch()
    if waiting:
        event = record_event(waiting[0].pending.device)
        if event is not None:
            event.synchronize()
    for k, b in enumerate(begun):
        if b is not None:
            parsed[k] = b.parsed()
    return tuple(parsed)


class _Side(NamedTuple):
    """one chunk of one side as the library takes it: the run array and the boxes, back to back in one pinned array"""
    host: torch.Tensor     # int32, pinned: words, then 4 n box words
    device: torch.Tensor   # the same on the device
    words: int
    n: int


def boxes_and_areas(words: np.ndarray, n: int, height: int) -> Tuple[np.ndarray, np.ndarray]:
    """the run array of n masks (include/deva_rle.h) -> (boxes int64 [n,4]: x0, y0, x1, y1 inclusive, -1 four times for an
    empty mask; areas int64 [n]): rule D5 of deva_rle.h, as `rle.records` gives it, straight from the starts.  A run of
    ones that goes on into another column covers its columns from top to bottom."""
    first = words[:n + 1].astype(np.int64)
    lo = words[n + 1:].astype(np.int64)                      # every start, as the first position of the run it begins
    if n == 0 or lo.size == 0:
        return np.full((n, 4), -1, dtype=np.int64), np.zeros(n, dtype=np.int64)
    hi = np.empty_like(lo)                                   # the run's last position; below `lo` for a count of zero
    hi[:-1] = lo[1:] - 1
    hi[-1] = -1                                              # (and for the last start of a mask: the next mask begins at 0)
    local = np.arange(lo.size) - np.repeat(first[:-1], np.diff(first))
    runs = np.flatnonzero(((local & 1) == 1) & (hi >= lo))   # the runs of ones that hold a pixel, all masks back to back
    empty = (np.full((n, 4), -1, dtype=np.int64), np.zeros(n, dtype=np.int64))
    if runs.size == 0:
        return empty
    lo, hi = lo[runs], hi[runs]
    x_lo, y_lo = np.divmod(lo, height)
    x_hi, y_hi = np.divmod(hi, height)
    whole = x_lo != x_hi
    y_lo[whole], y_hi[whole] = 0, height - 1
    at = np.searchsorted(runs, first[:-1])                   # where every mask's runs begin among them
    none = np.diff(np.append(at, runs.size)) == 0            # (a mask without any: `reduceat` gives it another mask's element, dropped below)

    def per_mask(op, values):                                # (one element more, neutral, so that `at` may point behind the last run)
        return op.reduceat(np.append(values, 0 if op is np.add else values[-1]), at)
    boxes = np.stack([per_mask(np.minimum, x_lo), per_mask(np.minimum, y_lo), per_mask(np.maximum, x_hi), per_mask(np.maximum, y_hi)], axis=1)
    areas = per_mask(np.add, hi - lo + 1)
    boxes[none], areas[none] = -1, 0
    return boxes, areas


def _side(parsed, lo: int, hi: int, side: int, pin: bool) -> _Side:
    """after a parse on the device the run array is in place there, with room for the boxes behind it: `device` is set and
    only the boxes are still to go up"""
    chunk = None if parsed.device is None else next(c for c in parsed.device if (c.lo, c.hi) == (lo, hi))
    words = _rle().run_array(parsed, lo, hi) if chunk is None else chunk.host
    check(lib().deva_overlap_check(words.ctypes.data, words.size, hi - lo, parsed.height, parsed.width, side), 'deva_overlap_check')
    host = torch.empty(words.size + 4 * (hi - lo), dtype=torch.int32, pin_memory=pin)
    host.numpy()[:words.size] = words
    host.numpy()[words.size:] = boxes_and_areas(words, hi - lo, parsed.height)[0].reshape(-1)
    return _Side(host, None if chunk is None else chunk.device[:host.numel()], int(words.size), hi - lo)


def _parts(parsed, max_masks: int, max_words: int, name: str) -> List[Tuple[int, int]]:
    if parsed.device is not None:
        return [(c.lo, c.hi) for c in parsed.device]
    return _rle().chunks(np.asarray(parsed.per_mask), max_masks, max_words, name)


def _launch(dt: _Side, gt: _Side, height: int, width: int, scratch, inter, area_d, area_g, stream) -> None:
    """deva_overlap_intersections on `stream` (the tests' CPU contract replaces this): inter is a [d, g] block of a
    row-major table, its row pitch the table's"""
    fn = 'intersections'
    for name, t in (('dt', dt.device), ('gt', gt.device), ('scratch', scratch), ('inter', inter), ('area_d', area_d), ('area_g', area_g)):
        require_on_device(t, name, fn)
    check(lib().deva_overlap_intersections(
        dt.host.data_ptr(), dt.device.data_ptr(), dt.words, dt.n, gt.host.data_ptr(), gt.device.data_ptr(), gt.words, gt.n, height, width,
        dt.device.data_ptr() + 4 * dt.words, gt.device.data_ptr() + 4 * gt.words, scratch.data_ptr(), scratch.numel() * 4,
        inter.data_ptr(), max(inter.stride(0), inter.shape[1]), area_d.data_ptr(),
        area_g.data_ptr(), stream), 'deva_overlap_intersections')


class PendingOverlap:
    """the tables of one `intersections(..., pending=True)` on their way to the host; `finish()` waits for them"""

    def __init__(self, inter, area_d, area_g, event):
        self._host, self._event, self._result = (inter, area_d, area_g), event, None

    def finish(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """-> (inter int64 [D,G], area_d int64 [D], area_g int64 [G]) on the host"""
        if self._result is None:
            if self._event is not None:
                self._event.synchronize()
            self._result = tuple(t.numpy().astype(np.int64) for t in self._host)
            self._host = None
        return self._result


def intersections(dt: Sequence, gt: Sequence, *, stream=None, source_size: Optional[Tuple[int, int]] = None, device=None,
                  out: Optional[dict] = None, pending: bool = False, max_masks: Optional[int] = None, max_words: Optional[int] = None,
                  parse: str = 'host'):
    """D detections and G ground-truth masks (two lists; each mask in any form `rle.parse_counts` takes, all of one
    size) -> (inter [D,G], area_d [D], area_g [G]) on the device: the pixels every pair shares and every mask's area,
    exact integers (int32 tensors; the library writes uint32 below 2^31, O3).

    Everything is parsed and checked (O2) before anything is launched; an error names the side and the mask.  Per side
    one int32 array (pinned; the run array, then the boxes) goes up on the stream, two launches follow on it and nothing
    synchronises; no result is copied to the host.  `stream`: a `torch.cuda.Stream` (default: the current one).
    `source_size`: for masks that are bare texts or lists.  `out`: preallocated contiguous int32 tensors by name
    ('inter', 'area_d', 'area_g'); they may be uninitialised.  With `pending=True` the three tables are also sent to
    pinned host memory on the same stream and a `PendingOverlap` is returned: still no wait, `finish()` has it.  More
    masks or runs on a side than one call takes (`overlap_limits()`; `max_masks` / `max_words` lower the limits) are
    walked D-chunk by G-chunk, each chunk of a side uploaded once.

    With D == 0 or G == 0 nothing is launched (O7): the areas of the other side are then the host's sums of its counts.

    `parse='device'`: a side whose masks are all texts is parsed on the device, on the same stream (`rle.parse_checked`);
    both sides are handed over before either is waited for, then one wait for their flags and one for the host copies of
    their run arrays; the tables are the same."""
    fn = 'intersections'
    rle = _rle()
    if stream is not None and not isinstance(stream, torch.cuda.Stream):
        raise DevaHipError(f'{fn}: `stream` must be a torch.cuda.Stream (got {type(stream).__name__})')
    if parse == 'device':
        limits = _limits(max_masks, max_words, fn)
        given = [t for t in (out or {}).values() if isinstance(t, torch.Tensor)]
        target = torch.device(device if device is not None else (given[0].device if given else (stream.device if stream is not None else 'cuda')))
        with contextlib.ExitStack() as stack:
            if target.type == 'cuda':
                stack.enter_context(torch.cuda.device(target))
                if stream is not None:
                    stack.enter_context(torch.cuda.stream(stream))
            parsed_d, parsed_g = _parse_sides(dt, gt, source_size, fn, parse, target, limits)
    else:
        parsed_d, parsed_g = _parse_sides(dt, gt, source_size, fn, parse)
    if (parsed_d.height, parsed_d.width) != (parsed_g.height, parsed_g.width):
        raise DevaHipError(f'{fn}: dt is {parsed_d.height} x {parsed_d.width}, gt is {parsed_g.height} x {parsed_g.width} (one size per call)')
    h, w = parsed_d.height, parsed_d.width
    n_d, n_g = int(parsed_d.per_mask.size), int(parsed_g.per_mask.size)
    top = _limits(max_masks, max_words, fn)
    blocks = [(pd, pg) for pd in _parts(parsed_d, *top, f'{fn}: dt') for pg in _parts(parsed_g, *top, f'{fn}: gt')]
    given = [t for t in (out or {}).values() if isinstance(t, torch.Tensor)]
    device = torch.device(device if device is not None else (given[0].device if given else (stream.device if stream is not None else 'cuda')))
    inter = out_tensor(out, 'inter', (n_d, n_g), torch.int32, device, fn)
    area_d, area_g = out_tensor(out, 'area_d', (n_d,), torch.int32, device, fn), out_tensor(out, 'area_g', (n_g,), torch.int32, device, fn)
    on_gpu = device.type == 'cuda'
    sides = {}
    for (lo_d, hi_d), (lo_g, hi_g) in blocks:             # every chunk built and checked before the first launch of the call
        for key, parsed in (((DT, lo_d, hi_d), parsed_d), ((GT, lo_g, hi_g), parsed_g)):
            if key not in sides:
                sides[key] = _side(parsed, key[1], key[2], key[0], on_gpu)
    with contextlib.ExitStack() as stack:
        if on_gpu:
            stack.enter_context(torch.cuda.device(device))
            if stream is not None:
                stack.enter_context(torch.cuda.stream(stream))
        handle = _stream(device) if on_gpu else None
        if not blocks:                                    # O7: an empty side
            for t, parsed in ((area_d, parsed_d), (area_g, parsed_g)):
                if t.numel():
                    areas = np.concatenate([boxes_and_areas(rle.run_array(parsed, lo, hi), hi - lo, h)[1]
                                            for lo, hi in rle.chunks(parsed.per_mask, MAX_MASKS, MAX_WORDS, fn)])
                    t.copy_(torch.from_numpy(areas.astype(np.int32)), non_blocking=True)
        for key, s in list(sides.items()):
            if s.device is None:
                sides[key] = s._replace(device=s.host.to(device, non_blocking=True))
            else:                                         # (parsed on the device: the boxes follow the run array there)
                s.device[s.words:].copy_(s.host[s.words:], non_blocking=True)
        for (lo_d, hi_d), (lo_g, hi_g) in blocks:
            side_d, side_g = sides[(DT, lo_d, hi_d)], sides[(GT, lo_g, hi_g)]
            scratch = torch.empty(max(side_g.words - side_g.n - 1, 1), dtype=torch.int32, device=device)
            _launch(side_d, side_g, h, w, scratch, inter[lo_d:hi_d, lo_g:hi_g], area_d[lo_d:hi_d], area_g[lo_g:hi_g], handle)
        if not pending:
            return inter, area_d, area_g
        host = [to_pinned(t) for t in (inter, area_d, area_g)]
        return PendingOverlap(host[0], host[1], host[2], record_event(device))


def iou_from_counts(inter: np.ndarray, area_d: np.ndarray, area_g: np.ndarray, iscrowd=None) -> np.ndarray:
    """the arithmetic of `pycocotools.mask.iou` for run-length inputs, in fp64 from the integers: inter / (a_d + a_g -
    inter), inter / a_d where iscrowd[g]; 0.0 wherever inter == 0 (the C code sets the union to 1 there, so two empty
    masks give 0, not NaN) -> float64 [D,G]"""
    inter = np.asarray(inter, dtype=np.int64)
    n_d, n_g = inter.shape
    crowd = np.zeros(n_g, dtype=bool) if iscrowd is None else np.asarray(iscrowd).astype(bool).reshape(-1)
    if crowd.size != n_g:
        raise DevaHipError(f'iou: iscrowd has {crowd.size} entries for {n_g} ground-truth masks')
    a_d = np.asarray(area_d, dtype=np.int64).reshape(n_d, 1)
    a_g = np.asarray(area_g, dtype=np.int64).reshape(1, n_g)
    union = np.where(crowd[None, :], np.broadcast_to(a_d, inter.shape), a_d + a_g - inter)
    union = np.where(inter == 0, 1, union)
    return inter.astype(np.float64) / union.astype(np.float64)


def iou(dt: Sequence, gt: Sequence, iscrowd=None, *, source_size: Optional[Tuple[int, int]] = None, device=None,
        parse: str = 'host') -> np.ndarray:
    """`pycocotools.mask.iou(dt, gt, iscrowd)` for run-length masks -> float64 [D,G] on the host: `intersections` on the
    device, one copy of its integers, then `iou_from_counts`.  `parse`: as `intersections` takes it."""
    if iscrowd is not None and len(iscrowd) != len(gt):
        raise DevaHipError(f'iou: iscrowd has {len(iscrowd)} entries for {len(gt)} ground-truth masks')
    inter, area_d, area_g = intersections(dt, gt, source_size=source_size, device=device, pending=True, parse=parse).finish()
    return iou_from_counts(inter, area_d, area_g, iscrowd)
