"""ctypes binding of libdeva_regions.so (C ABI declared in include/deva_regions.h): 8-connected components of byte planes,
and the clean-up a SAM-style mask generator applies with `min_mask_region_area`: fill the small holes of every mask, then
drop its small islands (rules R1-R7 of the header).

A fifth library next to libdeva_hip.so and the three scorers, loaded lazily by `lib()`; the conventions are those of
`deva.hip.pair_metrics`: `check` raises `DevaHipError` with the library's text, host tensors are refused, there is no CPU
path."""
import ctypes
import os
from ctypes import POINTER, Structure, c_char_p, c_int, c_int32, c_int64, c_uint32, c_void_p
from typing import NamedTuple, Optional, Tuple

import torch

from . import DevaHipError, _native, _planes, ops
from .ops import _stream

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libdeva_regions.so')
ABI_VERSION = 1

TILE = 32
FIELDS = 8
MAX_PLANES = 65536
MAX_PIXELS = 1 << 30
DEFAULT_SCRATCH = 256 << 20   # bytes `remove_small_regions` allocates at most when it is handed no scratch (one plane if larger)
# the fields of a record (R5)
CHANGED, FILLED, REMOVED, AREA, X0, Y0, X1, Y1 = range(8)


class Plan(Structure):
    """mirror of `struct deva_regions_plan` (include/deva_regions.h)"""
    _fields_ = [('tile', c_int32), ('block', c_int32), ('tiles_x', c_int32), ('tiles_y', c_int32), ('planes_per_pass', c_int32),
                ('passes', c_int32), ('local_grid', c_uint32), ('border_grid', c_uint32), ('pixel_grid', c_uint32),
                ('reserved', c_uint32), ('plane_bytes', c_int64), ('scratch_bytes', c_int64)]


# name -> (restype, argtypes); must list every symbol of include/deva_regions.h
SIGNATURES = {
    'deva_regions_version': (c_int, []),
    'deva_regions_last_error': (c_char_p, []),
    'deva_regions_scratch_bytes': (c_int, [c_int, c_int, c_int, POINTER(c_int64)]),
    'deva_regions_plan': (c_int, [c_int, c_int, c_int, c_int64, POINTER(Plan)]),
    'deva_regions_label': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_int64, c_void_p]),
    'deva_regions_clean': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_int64, c_void_p]),
}

_LIB = None


def lib() -> ctypes.CDLL:
    """Load (once) and return the region library; raises if it has not been built."""
    return _LIB or _native.load(globals(), 'deva_regions_version', 'libdeva_regions.so', 'the region kernels')


def check(code: int, what: str) -> None:
    if code != 0:
        _native.check(globals(), code, what, 'deva_regions_last_error')


class PlanInfo(NamedTuple):
    tile: int              # edge of a tile of the local stage
    block: int
    tiles_x: int
    tiles_y: int
    planes_per_pass: int   # planes cleaned together: min(n, budget // plane_bytes)
    passes: int
    local_grid: int        # workgroups of the local stage of a full pass
    border_grid: int       # of the border stage (0: a plane is one tile)
    pixel_grid: int        # of flatten, decide and rewrite
    reserved: int
    plane_bytes: int       # scratch of one plane in flight
    scratch_bytes: int     # planes_per_pass * plane_bytes


def region_scratch_bytes(height: int, width: int, n: int = 1) -> int:
    """the scratch that cleans `n` planes of height x width in one pass; `region_scratch_bytes(h, w)` is the least
    `remove_small_regions` takes"""
    nbytes = c_int64()
    check(lib().deva_regions_scratch_bytes(int(height), int(width), int(n), ctypes.byref(nbytes)), 'deva_regions_scratch_bytes')
    return int(nbytes.value)


def region_plan(height: int, width: int, n: int, budget_bytes: Optional[int] = None) -> PlanInfo:
    """the launches `remove_small_regions` makes for `n` planes with `budget_bytes` of scratch (default: one pass);
    host only: no device is touched"""
    if budget_bytes is None:
        budget_bytes = region_scratch_bytes(height, width, n)
    plan = Plan()
    check(lib().deva_regions_plan(int(height), int(width), int(n), int(budget_bytes), ctypes.byref(plan)), 'deva_regions_plan')
    return PlanInfo(*(int(getattr(plan, f[0])) for f in Plan._fields_))


def _arguments(planes, fn: str):
    """the checks that need no device (tests/emu_regions.py, the CPU contract, makes them too) -> (n, h, w, squeeze)"""
    if not isinstance(planes, torch.Tensor):
        raise DevaHipError(f'{fn}: planes must be a tensor (got {type(planes).__name__})')
    if planes.dtype != torch.uint8 or planes.dim() not in (2, 3):
        raise DevaHipError(f'{fn}: planes must be uint8 [K,H,W] or [H,W] (got {planes.dtype} {tuple(planes.shape)})')
    squeeze = planes.dim() == 2
    n = 1 if squeeze else int(planes.shape[0])
    h, w = int(planes.shape[-2]), int(planes.shape[-1])
    if h < 1 or w < 1 or h * w > MAX_PIXELS:
        raise DevaHipError(f'{fn}: bad plane size {h} x {w}')
    if n > MAX_PLANES:
        raise DevaHipError(f'{fn}: 0 to {MAX_PLANES} planes (got {n})')
    return n, h, w, squeeze


def _min_area(min_area) -> int:
    if isinstance(min_area, bool) or int(min_area) != min_area or int(min_area) <= 0 or int(min_area) > 2**31 - 1:
        raise DevaHipError(f'remove_small_regions: min_area must be positive (got {min_area})')
    return int(min_area)


def _check_records(records, n: int, squeeze: bool) -> None:
    shape = (FIELDS,) if squeeze else (n, FIELDS)
    if records is not None and (records.dtype != torch.int32 or tuple(records.shape) != shape):
        raise DevaHipError(f'remove_small_regions: `records` must be int32 {list(shape)}')


def _check_labels(out, planes) -> None:
    if out is not None and (out.dtype != torch.int32 or out.shape != planes.shape):
        raise DevaHipError(f'label_components: `out` must be int32 {list(planes.shape)}')


def _in_place(planes, fn: str) -> None:
    if not planes.is_cuda:
        raise DevaHipError(f'{fn}: planes must live on the HIP device (got {planes.device}); there is no CPU path')
    if not planes.is_contiguous():
        raise DevaHipError(f'{fn}: planes must be contiguous')


def label_components(planes: torch.Tensor, of_zeros: bool = False, out: Optional[torch.Tensor] = None,
                     scratch: Optional[torch.Tensor] = None) -> torch.Tensor:
    """uint8 [K,H,W] or [H,W] on the device -> int32 labels of the same shape on the device: 0 where the pixel is not of the
    labelled kind (the non-zero bytes; with `of_zeros` the zero ones), else 1 + the smallest row-major position
    y * W + x of the pixel's 8-connected component.  Three launches on the current stream, nothing synchronises.
    `out`: the int32 tensor to write into.  `scratch` is accepted for symmetry and not used: `out` is the union-find array."""
    n, h, w, _ = _arguments(planes, 'label_components')
    _check_labels(out, planes)
    _in_place(planes, 'label_components')
    if out is None:
        out = torch.empty(planes.shape, dtype=torch.int32, device=planes.device)
    _planes.check_out_on_device(out, 'label_components')
    check(lib().deva_regions_label(planes.data_ptr() if n else None, n, h, w, int(bool(of_zeros)), out.data_ptr() if n else None,
                                   None, 0, _stream(planes.device)), 'deva_regions_label')
    return out


def remove_small_regions(planes: torch.Tensor, min_area: int, *, scratch: Optional[torch.Tensor] = None,
                         records: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """uint8 [K,H,W] or [H,W], contiguous, on the device, cleaned IN PLACE -> (planes, records int32 [K,8] or [8]) on the
    device: per plane the holes of fewer than `min_area` pixels are filled, then the islands of fewer than `min_area`
    pixels removed (rules R1-R7 of deva_regions.h; 8-connectivity for both; where every island is small the largest
    stays), every byte written back as 0 / 1.  A record is (changed, pixels filled, pixels removed, area, x0, y0, x1, y1)
    with the inclusive box of what is left, 0,0,0,0 for nothing.
    `scratch`: a uint8 device tensor to reuse, of at least `region_scratch_bytes(H, W)` bytes: as many planes as it holds
    are cleaned together, the rest in further passes (default: allocated here, for all planes or `DEFAULT_SCRATCH` bytes
    worth of them, whichever is less).  `records`: the tensor to
    write into.  Launched on the current stream; nothing synchronises."""
    fn = 'remove_small_regions'
    n, h, w, squeeze = _arguments(planes, fn)
    min_area = _min_area(min_area)
    _check_records(records, n, squeeze)
    need = region_scratch_bytes(h, w, 1)
    if scratch is not None and (scratch.dtype != torch.uint8 or scratch.dim() != 1 or scratch.numel() < need):
        raise DevaHipError(f'{fn}: `scratch` must be uint8 [{need}] or longer')
    _in_place(planes, fn)
    _planes.check_out_on_device(records, fn)
    if scratch is not None and not (scratch.is_cuda and scratch.is_contiguous() and scratch.data_ptr() % 16 == 0):
        raise DevaHipError(f'{fn}: `scratch` must be a contiguous 16-byte aligned tensor on the HIP device')
    if records is None:
        records = torch.empty((FIELDS,) if squeeze else (n, FIELDS), dtype=torch.int32, device=planes.device)
    if n:
        if scratch is None:
            together = min(n, max(1, DEFAULT_SCRATCH // need))
            scratch = torch.empty(together * need, dtype=torch.uint8, device=planes.device)
        check(lib().deva_regions_clean(planes.data_ptr(), n, h, w, min_area, records.data_ptr(), scratch.data_ptr(), scratch.numel(),
                                       _stream(planes.device)), 'deva_regions_clean')
    return planes, records


# ------------------------------------------------------------------------------------------ the generator's step
class RegionBuffers(NamedTuple):
    """memory of `clean_and_suppress` for up to `capacity` planes, allocated once and reused"""
    packed: torch.Tensor    # int32 [capacity * 9 + 1], device: K records, then K + 1 words of box NMS (the keep list, its count)
    host: torch.Tensor      # the pinned copy
    scratch: torch.Tensor   # uint8, device: the region kernels'


def region_buffers(height: int, width: int, capacity: int, device) -> RegionBuffers:
    words = int(capacity) * (FIELDS + 1) + 1
    need = region_scratch_bytes(height, width)
    together = min(int(capacity), max(1, DEFAULT_SCRATCH // need))
    return RegionBuffers(torch.empty(words, dtype=torch.int32, device=device), torch.empty(words, dtype=torch.int32, pin_memory=True),
                         torch.empty(together * need, dtype=torch.uint8, device=device))


def clean_and_suppress(masks: torch.Tensor, min_area: int, nms_thresh: float,
                       buffers: RegionBuffers) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """the reference generator's `postprocess_small_regions` on K >= 1 byte planes [K,H,W] on the device:
    `remove_small_regions` in place, boxes from the records, scores `1 - changed`, `ops.box_nms` (so the planes that needed
    no fixing win, and among equals the earlier one), then ONE pinned host copy of the records and the keep list together,
    the only synchronisation -> (records int32 [K,8] on the host, keep int64 [K'] on the host, keep int64 [K'] on the device);
    the caller selects what it keeps in that order"""
    k = int(masks.shape[0])
    packed, host, scratch = buffers
    used = k * (FIELDS + 1) + 1
    if masks.dim() != 3 or k < 1 or used > packed.numel():
        raise DevaHipError(f'clean_and_suppress: 1 to {(packed.numel() - 1) // (FIELDS + 1)} planes [K,H,W] (got {tuple(masks.shape)})')
    records = packed[:k * FIELDS].view(k, FIELDS)
    remove_small_regions(masks, min_area, scratch=scratch, records=records)
    boxes = records[:, X0:Y1 + 1].contiguous()
    scores = (1 - records[:, CHANGED]).to(torch.float32)
    ops._box_nms('box_nms', boxes, torch.int32, scores, nms_thresh, packed[k * FIELDS:used], False)
    host[:used].copy_(packed[:used], non_blocking=True)
    event = torch.cuda.Event()
    event.record()
    event.synchronize()
    kept = int(host[used - 1])
    keep = host[k * FIELDS:k * FIELDS + kept].to(torch.int64)
    return host[:k * FIELDS].view(k, FIELDS).clone(), keep, packed[k * FIELDS:k * FIELDS + kept].to(torch.int64)
