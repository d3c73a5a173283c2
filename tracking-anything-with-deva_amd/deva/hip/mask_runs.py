"""ctypes binding of libdeva_mask_runs.so (C ABI declared in include/deva_mask_runs.h): a stack of mask planes [N,H,W]
on the device, as `ProposalFilter.finish()` or a segmenter returns them and `assemble_*` takes them (uint8, bool or float
logits against a threshold; the masks may overlap), encoded as COCO run lengths without a copy of the planes to the host
and without `pycocotools` (rules E1-E7 of the header).  The inverse of `deva.hip.rle.decode`.

The device gives the run boundaries of all masks back to back (`count`, then `write`: the contract of `ops.mask_rle`);
the host turns them into counts and compressed strings with the arithmetic `FrameResultSaver` already uses
(`frame_results.rle_counts`, `coco_strings`).  `encode_labels` does the same for an index mask and a list of ids on the
existing `ops.mask_rle`.  With `text='device'` (an opt-in of both) the strings are coded on the device as well
(`deva.hip.rle_text`, libdeva_rle_text.so) and only their bytes come to the host; the results are the same.

A seventh library next to libdeva_hip.so, the three scorers, the regions and the decoder, loaded lazily by `lib()`; the
conventions are those of `deva.hip.rle`: `check` raises `DevaHipError` with the library's text, there is no CPU path."""
import ctypes
import os
from ctypes import POINTER, Structure, c_char_p, c_float, c_int, c_int32, c_int64, c_uint32, c_void_p
from typing import Callable, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import DevaHipError, _native, ops, rle_text
from ._pending import out_tensor, record_event, require_on_device, to_pinned
from .ops import _stream

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libdeva_mask_runs.so')
ABI_VERSION = 1

TILE = 64
MAX_MASKS = 65536
MAX_SCRATCH = 1 << 30
SCAN_CHUNK = 2048
MASK_CHUNK = 256
SEGMENT_BYTES = 12
DTYPES = {torch.uint8: 0, torch.float32: 1}   # DEVA_RUNS_U8, DEVA_RUNS_F32
FORMS = ('string', 'bytes', 'counts')
TEXT = ('host', 'device')   # where the compressed strings are coded
STATS = ('area', 'x_min', 'y_min', 'x_max', 'y_max')


class Limits(Structure):
    """mirror of `struct deva_runs_limits` (include/deva_mask_runs.h)"""
    _fields_ = [('max_masks', c_int32), ('tile', c_int32), ('block', c_int32), ('scan_chunk', c_int32), ('mask_chunk', c_int32),
                ('reserved', c_int32), ('max_scratch', c_int64)]


class Plan(Structure):
    """mirror of `struct deva_runs_plan`"""
    _fields_ = [('tiles_x', c_int32), ('tiles_y', c_int32), ('segments', c_int32), ('scan_chunks', c_int32), ('mask_chunks', c_int32),
                ('count_grid', c_uint32), ('write_grid', c_uint32), ('reserved', c_int32), ('scratch_bytes', c_int64)]


# name -> (restype, argtypes); must list every symbol of include/deva_mask_runs.h
SIGNATURES = {
    'deva_runs_version': (c_int, []),
    'deva_runs_last_error': (c_char_p, []),
    'deva_runs_limits': (c_int, [POINTER(Limits)]),
    'deva_runs_plan': (c_int, [c_int, c_int, c_int, POINTER(Plan)]),
    'deva_runs_scratch': (c_int64, [c_int, c_int, c_int]),
    'deva_runs_count': (c_int, [c_void_p, c_int, c_float, c_int, c_int, c_int, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p,
                                c_void_p, c_void_p]),
    'deva_runs_write': (c_int, [c_int, c_int, c_int, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p]),
}

_LIB = None


def lib() -> ctypes.CDLL:
    """Load (once) and return the run-length encoder's library; raises if it has not been built."""
    return _LIB or _native.load(globals(), 'deva_runs_version', 'libdeva_mask_runs.so', 'the run-length encoder')


def check(code: int, what: str) -> None:
    if code != 0:
        _native.check(globals(), code, what, 'deva_runs_last_error')


class LimitInfo(NamedTuple):
    max_masks: int     # masks of one call of the library; `encode` walks more in chunks
    tile: int          # edge of the tile a workgroup owns; rows of a segment
    block: int
    scan_chunk: int    # segments of one step of the per-mask scan
    mask_chunk: int    # masks of one step of the cross-mask scan
    reserved: int
    max_scratch: int   # bytes of one call's scratch


class PlanInfo(NamedTuple):
    tiles_x: int
    tiles_y: int
    segments: int      # of one mask: W * tiles_y
    scan_chunks: int
    mask_chunks: int
    count_grid: int
    write_grid: int
    reserved: int
    scratch_bytes: int


def runs_limits() -> LimitInfo:
    """what one call of the library takes; host only"""
    limits = Limits()
    check(lib().deva_runs_limits(ctypes.byref(limits)), 'deva_runs_limits')
    return LimitInfo(*(int(getattr(limits, f[0])) for f in Limits._fields_))


def runs_plan(n: int, size: Tuple[int, int]) -> PlanInfo:
    """the launches `count` and `write` make for `n` masks of `size`; host only: no device is touched"""
    plan = Plan()
    check(lib().deva_runs_plan(int(n), int(size[0]), int(size[1]), ctypes.byref(plan)), 'deva_runs_plan')
    return PlanInfo(*(int(getattr(plan, f[0])) for f in Plan._fields_))


def runs_scratch(n: int, size: Tuple[int, int]) -> int:
    """bytes of scratch of one call; -1 beyond the limits (E6)"""
    return int(lib().deva_runs_scratch(int(n), int(size[0]), int(size[1])))


# ------------------------------------------------------------------------------------------ arguments
def _prepare(planes, threshold, fn: str) -> Tuple[torch.Tensor, int, float]:
    """E1 and E6 on the host, before any launch -> (the planes as the library takes them, dtype code, threshold)"""
    if not isinstance(planes, torch.Tensor) or planes.dim() != 3:
        raise DevaHipError(f'{fn}: planes must be an [N,H,W] tensor (got {type(planes).__name__}'
                           f'{tuple(planes.shape) if isinstance(planes, torch.Tensor) else ""})')
    if planes.dtype == torch.bool:
        planes = planes.view(torch.uint8)
    if planes.dtype not in DTYPES:
        raise DevaHipError(f'{fn}: planes must be torch.uint8, torch.bool or torch.float32 (got {planes.dtype})')
    if planes.dtype == torch.float32 and threshold is None:
        raise DevaHipError(f'{fn}: float32 planes need a `threshold` (the pixel is 1 iff value > threshold)')
    if planes.dtype != torch.float32 and threshold is not None:
        raise DevaHipError(f'{fn}: `threshold` is for float32 planes (got {planes.dtype}: the pixel is 1 iff the byte is not 0)')
    _, h, w = planes.shape
    if h < 1 or w < 1 or h * w >= 2**31:
        raise DevaHipError(f'{fn}: bad height x width {h} x {w} (1 <= H * W < 2^31)')
    return planes.contiguous(), DTYPES[planes.dtype], 0.0 if threshold is None else float(threshold)


def _limits(max_masks, max_scratch, fn: str) -> Tuple[int, int]:
    top = runs_limits()
    max_masks = top.max_masks if max_masks is None else int(max_masks)
    max_scratch = top.max_scratch if max_scratch is None else int(max_scratch)
    if not (1 <= max_masks <= top.max_masks and SEGMENT_BYTES <= max_scratch <= top.max_scratch):
        raise DevaHipError(f'{fn}: limits of 1 to {top.max_masks} masks and {SEGMENT_BYTES} to {top.max_scratch} bytes of scratch '
                           f'(got {max_masks}, {max_scratch})')
    return max_masks, max_scratch


def chunks(n: int, size: Tuple[int, int], max_masks: int, max_scratch: int, fn: str = 'encode') -> List[Tuple[int, int]]:
    """[lo, hi) ranges of masks, each within one call's limits: hi - lo <= max_masks and its scratch <= max_scratch"""
    h, w = int(size[0]), int(size[1])
    per_mask = w * ((h + TILE - 1) // TILE) * SEGMENT_BYTES
    if per_mask > max_scratch:
        raise DevaHipError(f'{fn}: one mask of {h} x {w} needs {per_mask} bytes of scratch, above the limit of one call ({max_scratch})')
    step = min(int(max_masks), max_scratch // per_mask)
    return [(lo, min(lo + step, n)) for lo in range(0, n, step)]


# ------------------------------------------------------------------------------------------ the two calls of the library
def _launch_count(planes, code, threshold, scratch, n_out, base, total, first, stats) -> None:
    """deva_runs_count on the current stream of the planes' device (the tests' CPU contract replaces this and `_launch_write`)"""
    fn = 'count'
    for name, t in (('planes', planes), ('scratch', scratch), ('n', n_out), ('base', base), ('total', total), ('first', first),
                    ('stats', stats)):
        if t is not None:
            require_on_device(t, name, fn)
    n, h, w = planes.shape
    with torch.cuda.device(planes.device):
        check(lib().deva_runs_count(planes.data_ptr(), code, threshold, n, h, w, scratch.data_ptr(), scratch.numel() * 4, n_out.data_ptr(),
                                    base.data_ptr(), total.data_ptr(), None if first is None else first.data_ptr(),
                                    None if stats is None else stats.data_ptr(), _stream(planes.device)), 'deva_runs_count')


def _launch_write(n, h, w, scratch, base, bounds, capacity) -> None:
    fn = 'write'
    for name, t in (('scratch', scratch), ('base', base), ('bounds', bounds)):
        require_on_device(t, name, fn)
    with torch.cuda.device(scratch.device):
        check(lib().deva_runs_write(n, h, w, scratch.data_ptr(), scratch.numel() * 4, base.data_ptr(),
                                    bounds.data_ptr() if capacity else None, capacity, _stream(scratch.device)), 'deva_runs_write')


class Counted(NamedTuple):
    """what `count` leaves on the device for `write`"""
    n: torch.Tensor                 # int32 [N]: boundaries of every mask (E3)
    base: torch.Tensor              # int64 [N]: where every mask's boundaries begin in `bounds` (E5)
    total: torch.Tensor             # int64 [1]: first + all boundaries
    stats: Optional[torch.Tensor]   # int32 [N,5] `STATS` (E4)
    scratch: torch.Tensor           # int32: the offsets and words `write` reads
    height: int
    width: int


def count(planes: torch.Tensor, threshold: Optional[float] = None, *, stats: bool = False, first: Optional[torch.Tensor] = None,
          out: Optional[dict] = None) -> Counted:
    """the first half of an encoding, one call of the library (at most `runs_limits()` masks and scratch): the boundary
    bits of every mask go to a scratch, their numbers to `n`, `base` and `total`, and with `stats=True` the areas and
    boxes to `stats`.  `first`: an int64 [1] on the device that `base` starts at (the `total` of the call before, E5).
    `out`: preallocated tensors by name ('n', 'base', 'total', 'stats', 'scratch').  Nothing synchronises."""
    fn = 'count'
    planes, code, threshold = _prepare(planes, threshold, fn)
    n, h, w = planes.shape
    device = planes.device
    if first is not None and (not isinstance(first, torch.Tensor) or first.dtype != torch.int64 or first.numel() != 1):
        raise DevaHipError(f'{fn}: `first` must be an int64 tensor of one element on the device')
    nbytes = runs_scratch(n, (h, w))
    if nbytes < 0:
        raise DevaHipError(f'{fn}: {n} masks of {h} x {w} are above the limits of one call: {lib().deva_runs_last_error().decode()}')
    counted = Counted(out_tensor(out, 'n', (n,), torch.int32, device, fn), out_tensor(out, 'base', (n,), torch.int64, device, fn),
                      out_tensor(out, 'total', (1,), torch.int64, device, fn),
                      out_tensor(out, 'stats', (n, 5), torch.int32, device, fn) if stats else None,
                      out_tensor(out, 'scratch', (nbytes // 4,), torch.int32, device, fn), h, w)
    if n:
        _launch_count(planes, code, threshold, counted.scratch, counted.n, counted.base, counted.total, first, counted.stats)
    elif first is not None:
        counted.total.copy_(first.reshape(1))
    else:
        counted.total.zero_()
    return counted


def write(counted: Counted, bounds: torch.Tensor, capacity: Optional[int] = None) -> torch.Tensor:
    """the second half: the boundaries of `counted` into `bounds` (int32 on the device, contiguous), of which the first
    `capacity` (default: all) may be written (E5).  It must follow its `count` on the same stream.  -> bounds"""
    fn = 'write'
    if not isinstance(bounds, torch.Tensor) or bounds.dtype != torch.int32 or bounds.dim() != 1 or not bounds.is_contiguous():
        raise DevaHipError(f'{fn}: `bounds` must be a contiguous int32 vector on the device')
    capacity = bounds.numel() if capacity is None else int(capacity)
    if not 0 <= capacity <= bounds.numel():
        raise DevaHipError(f'{fn}: capacity {capacity} is outside `bounds` ({bounds.numel()} elements)')
    n = counted.n.numel()
    if n:
        _launch_write(n, counted.height, counted.width, counted.scratch, counted.base, bounds, capacity)
    return bounds


# ------------------------------------------------------------------------------------------ encode
class PendingRuns:
    """an encoding whose results are on their way to the host; `finish()` waits for them"""

    def __init__(self, size, form, n, bounds, total, stats, capacity, event, text=None):
        self.size, self.form, self.capacity = size, form, capacity
        self._n, self._bounds, self._total, self._stats, self._event = n, bounds, total, stats, event
        self._text = text          # a `rle_text.PendingText`: the strings were coded on the device, `bounds` stayed there
        self._result = None

    def finish(self) -> List[dict]:
        """-> the list `encode` returns; raises DevaHipError when the boundaries did not fit the capacity"""
        if self._result is None:
            if self._event is not None:
                self._event.synchronize()
            total = int(self._total[-1]) if self._total is not None else 0
            if total > self.capacity:
                raise DevaHipError(f'encode: the masks have {total} run boundaries, the capacity is {self.capacity}')
            if self._text is not None:
                self._result = _text_records(self._text.finish(), None if self._stats is None else self._stats.numpy(), self.size, self.form)
                return self._result
            self._result = _records(self._n.numpy(), self._bounds.numpy()[:total], None if self._stats is None else self._stats.numpy(),
                                    self.size, self.form)
        return self._result


def _records(n: np.ndarray, bounds: np.ndarray, stats: Optional[np.ndarray], size: Tuple[int, int], form: str) -> List[dict]:
    """E3 on the host: the arithmetic of `FrameResultSaver` (frame_results.rle_counts / coco_strings)"""
    from deva.inference.frame_results import coco_strings, rle_counts   # (that module imports deva.hip.rle, which re-exports this one)
    h, w = size
    counts, lengths = rle_counts(np.concatenate([[0], n]), bounds, h * w)
    if form == 'counts':
        ends = np.cumsum(lengths)
        flat = counts.tolist()
        bodies = [flat[e - m:e] for e, m in zip(ends.tolist(), lengths.tolist())]
    else:
        bodies = coco_strings(counts, lengths)
        if form == 'bytes':
            bodies = [b.encode('ascii') for b in bodies]
    out = [{'size': [h, w], 'counts': b} for b in bodies]
    if stats is not None:
        for rec, row in zip(out, stats.tolist()):
            rec['area'] = row[0]
            rec['bbox'] = row[1:] if row[0] > 0 else None
    return out


def _text_records(bodies: List[bytes], stats: Optional[np.ndarray], size: Tuple[int, int], form: str) -> List[dict]:
    """`_records` for strings that were coded on the device"""
    h, w = size
    out = [{'size': [h, w], 'counts': b if form == 'bytes' else b.decode('ascii')} for b in bodies]
    if stats is not None:
        for rec, row in zip(out, stats.tolist()):
            rec['area'] = row[0]
            rec['bbox'] = row[1:] if row[0] > 0 else None
    return out


def _text_mode(text, form: str, fn: str) -> bool:
    """-> the strings are coded on the device ('counts' has no string: it takes the host path whatever `text` says)"""
    if text not in TEXT:
        raise DevaHipError(f'{fn}: text must be one of {TEXT} (got {text!r})')
    return text == 'device' and form != 'counts'


def encode(planes: torch.Tensor, *, threshold: Optional[float] = None, form: str = 'string', stats: bool = False,
           capacity: Optional[int] = None, max_masks: Optional[int] = None, max_scratch: Optional[int] = None,
           before_wait: Optional[Callable[[], None]] = None, text: str = 'host'):
    """[N,H,W] planes on the device (uint8 or bool: 1 iff not 0; float32 with `threshold`: 1 iff value > threshold, E1)
    -> [{'size': [H, W], 'counts': ...}] in mask order, `counts` as `form` says: 'string' (the ASCII text `pycocotools`
    gives after `.decode('ascii')`), 'bytes', or 'counts' (a list of int).  With `stats=True` every entry also holds
    'area' and 'bbox' (xyxy inclusive, None for an empty mask, as `FrameResult` records it).

    The host waits once, for the 8 bytes of the total, which size `bounds` exactly (`before_wait`, if given, is called
    right before that: nothing has synchronised up to there).  With `capacity=` nothing synchronises: `bounds` holds
    `capacity` boundaries and the call returns a `PendingRuns`, whose `finish()` waits, raises if the masks had more
    boundaries than that and otherwise returns the same list.  More masks than one call of the library takes
    (`runs_limits()`; `max_masks` / `max_scratch` lower the limits) are walked in chunks that fill one `bounds`.

    `text='device'` (forms 'string' and 'bytes'): the strings are coded on the device from `bounds`
    (`rle_text.encode_text`), into a buffer sized from what the call already knows, `max_chars(H * W)` characters for each
    of the `room + N` counts there can be; the characters and their lengths come to the host in place of the boundaries,
    with the same one wait.  The result is identical."""
    fn = 'encode'
    planes, code, threshold_value = _prepare(planes, threshold, fn)
    if form not in FORMS:
        raise DevaHipError(f'{fn}: form must be one of {FORMS} (got {form!r})')
    on_device = _text_mode(text, form, fn)
    if capacity is not None and int(capacity) < 0:
        raise DevaHipError(f'{fn}: capacity must not be negative (got {capacity})')
    n, h, w = planes.shape
    if n == 0:
        none = torch.zeros(0, dtype=torch.int32)
        return [] if capacity is None else PendingRuns((h, w), form, none, none, None, None, int(capacity), None)
    parts = chunks(n, (h, w), *_limits(max_masks, max_scratch, fn), fn)
    device = planes.device
    n_dev = torch.empty(n, dtype=torch.int32, device=device)
    base = torch.empty(n, dtype=torch.int64, device=device)
    totals = torch.zeros(len(parts) + 1, dtype=torch.int64, device=device)
    stats_dev = torch.empty((n, 5), dtype=torch.int32, device=device) if stats else None
    counted = []
    for c, (lo, hi) in enumerate(parts):
        out = {'n': n_dev[lo:hi], 'base': base[lo:hi], 'total': totals[c + 1:c + 2]}
        if stats:
            out['stats'] = stats_dev[lo:hi]
        counted.append(count(planes[lo:hi], threshold, stats=stats, first=totals[c:c + 1], out=out))
    if capacity is None:
        if before_wait is not None:
            before_wait()
        room = int(totals[-1:].cpu())                      # the one synchronisation of the call
    else:
        room = int(capacity)
    bounds = torch.empty(room, dtype=torch.int32, device=device)
    for part in counted:
        write(part, bounds, room)
    coded = rle_text.encode_text(n_dev, base, bounds, (h, w), pending=True, record=False) if on_device else None
    host = [to_pinned(t) if t is not None else None for t in (n_dev, None if on_device else bounds, totals, stats_dev)]
    pending = PendingRuns((h, w), form, host[0], host[1], host[2], host[3], room, record_event(device), coded)
    return pending.finish() if capacity is None else pending


# ------------------------------------------------------------------------------------------ labels
def encode_labels(labels: torch.Tensor, ids: Sequence[int], *, form: str = 'string', text: str = 'host') -> List[dict]:
    """an int64, int32 or int16 [H,W] label plane on the device (a detection's index mask) and a list of ids -> the run
    lengths of `labels == id` per id, in the order of `ids`: [{'size': [H, W], 'counts': ...}].  An id that no pixel
    holds gives [H * W].  The ids are mapped to channels with torch ops and the planes' objects are disjoint, so this is
    the existing `ops.mask_rle`: no new kernel.  `text='device'`: the strings are coded on the device (`encode`)."""
    fn = 'encode_labels'
    if not isinstance(labels, torch.Tensor) or labels.dim() != 2 or labels.dtype not in (torch.int64, torch.int32, torch.int16):
        raise DevaHipError(f'{fn}: labels must be an int64, int32 or int16 [H,W] tensor on the device')
    if form not in FORMS:
        raise DevaHipError(f'{fn}: form must be one of {FORMS} (got {form!r})')
    on_device = _text_mode(text, form, fn)
    ids = [int(i) for i in ids]
    if len(set(ids)) != len(ids):
        raise DevaHipError(f'{fn}: the ids must be distinct (got {ids})')
    if len(ids) + 1 > ops.RLE_MAX_CHANNELS:
        raise DevaHipError(f'{fn}: at most {ops.RLE_MAX_CHANNELS - 1} ids (got {len(ids)})')
    h, w = labels.shape
    if not ids:
        return []
    order = sorted(range(len(ids)), key=ids.__getitem__)
    table = torch.tensor([ids[k] for k in order], dtype=torch.int64, device=labels.device)
    channel_of = torch.tensor([k + 1 for k in order], dtype=torch.int16, device=labels.device)
    wide = labels.to(torch.int64)
    at = torch.searchsorted(table, wide).clamp_(max=len(ids) - 1)  # the one id a pixel can equal
    channel = torch.where(table[at] == wide, channel_of[at], torch.zeros((), dtype=torch.int16, device=labels.device))
    n, bounds = ops.mask_rle(channel.contiguous(), len(ids) + 1)
    if on_device:                                        # (`n` is on the host; the background has no boundaries in `bounds`)
        per = n[1:].to(torch.int32).contiguous()
        base = torch.cumsum(per, 0, dtype=torch.int64) - per
        return _text_records(rle_text.encode_text(per.to(bounds.device), base.to(bounds.device), bounds, (h, w)), None, (h, w), form)
    return _records(n[1:].cpu().numpy(), bounds.cpu().numpy(), None, (h, w), form)
