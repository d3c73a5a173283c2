"""ctypes binding of libdeva_vos_metrics.so (C ABI declared in include/deva_vos_metrics.h): the DAVIS measures of a
video-object-segmentation run, region similarity J and boundary accuracy F, from seven counts per object and frame.

A third library next to libdeva_hip.so and libdeva_metrics.so, loaded lazily by `lib()`; the conventions are those of
`deva.hip.metrics`: `check` raises `DevaHipError` with the library's text, host tensors are refused, there is no CPU
path."""
import ctypes
import os
from ctypes import POINTER, Structure, c_char_p, c_double, c_int, c_int32, c_int64, c_uint32, c_void_p
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import DevaHipError, _native, _planes
from .ops import _stream

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libdeva_vos_metrics.so')
ABI_VERSION = 1

U8, I32, I64, INDEX16 = 0, 1, 2, 3
BINARY = 256
MAX_OBJECTS = 64
MAX_RADIUS = 128
MAX_PIXELS = 1 << 30
FIELDS = 8
STRIP = 8
INNER_RADIUS = 3
MIDDLE_RADIUS = 8
# the fields of a record (R5)
INTER, AREA_GT, AREA_PRED, BOUNDARY_GT, BOUNDARY_PRED, MATCHED_GT, MATCHED_PRED = range(7)


class Plan(Structure):
    """mirror of `struct deva_vos_plan` (include/deva_vos_metrics.h)"""
    _fields_ = [('label_grid', c_uint32), ('match_grid', c_uint32), ('block', c_uint32), ('lds_bytes', c_uint32),
                ('inner_radius', c_int32), ('radius', c_int32), ('scratch_bytes', c_int64)]


# name -> (restype, argtypes); must list every symbol of include/deva_vos_metrics.h
SIGNATURES = {
    'deva_vos_version': (c_int, []),
    'deva_vos_last_error': (c_char_p, []),
    'deva_vos_boundary_radius': (c_int, [c_int, c_int, c_double, POINTER(c_int)]),
    'deva_vos_boundary_scratch_bytes': (c_int, [c_int, c_int, POINTER(c_int64)]),
    'deva_vos_boundary_plan': (c_int, [c_int, c_int, c_int, c_int, POINTER(Plan)]),
    'deva_vos_boundary_counts': (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int,
                                         c_void_p, c_int64, c_void_p, c_void_p]),
}

_LIB = None


def lib() -> ctypes.CDLL:
    """Load (once) and return the DAVIS scoring library; raises if it has not been built."""
    return _LIB or _native.load(globals(), 'deva_vos_version', 'libdeva_vos_metrics.so', 'the DAVIS scoring kernels')


def check(code: int, what: str) -> None:
    if code != 0:   # (tested here: the inference wrappers call this after every launch)
        _native.check(globals(), code, what, 'deva_vos_last_error')


class PlanInfo(NamedTuple):
    label_grid: int      # workgroups of the pass over the planes
    match_grid: int      # workgroups of the disk search
    block: int
    lds_bytes: int
    inner_radius: int    # the box that is searched first
    radius: int
    scratch_bytes: int


def boundary_radius(height: int, width: int, bound_th: float = 0.008) -> int:
    """R3: `bound_th` itself when it is 1 or more (an integer), else ceil(bound_th * the image's diagonal)"""
    r = c_int()
    check(lib().deva_vos_boundary_radius(int(height), int(width), float(bound_th), ctypes.byref(r)), 'deva_vos_boundary_radius')
    return int(r.value)


def boundary_scratch_bytes(height: int, width: int) -> int:
    n = c_int64()
    check(lib().deva_vos_boundary_scratch_bytes(int(height), int(width), ctypes.byref(n)), 'deva_vos_boundary_scratch_bytes')
    return int(n.value)


def boundary_plan(height: int, width: int, n_objects: int, radius: int) -> PlanInfo:
    """the two launches `boundary_counts` makes for these sizes (host only: no device is touched)"""
    plan = Plan()
    check(lib().deva_vos_boundary_plan(int(height), int(width), int(n_objects), int(radius), ctypes.byref(plan)),
          'deva_vos_boundary_plan')
    return PlanInfo(int(plan.label_grid), int(plan.match_grid), int(plan.block), int(plan.lds_bytes), int(plan.inner_radius),
                    int(plan.radius), int(plan.scratch_bytes))


# ------------------------------------------------------------------------------------------ the seven counts
_GT_ENC = {torch.uint8: U8, torch.int32: I32}
_PRED_ENC = {torch.uint8: U8, torch.int32: I32, torch.int64: I64, torch.int16: INDEX16}


def id_list(ids) -> np.ndarray:
    """`ids` as the caller gives them -> int32 [n], checked: distinct, ascending, in 1 .. 2^31 - 1, at least one"""
    return _planes.host_ids(ids, 'boundary_counts', 'ids', allow_empty=False)


def _plane(t, name: str, encodings):
    if not isinstance(t, torch.Tensor):
        raise DevaHipError(f'boundary_counts: {name} must be a tensor (got {type(t).__name__})')
    if t.dim() != 2 or t.dtype not in encodings:
        raise DevaHipError(f'boundary_counts: {name} must be an [H,W] plane of {", ".join(str(d) for d in encodings)} '
                           f'(got {t.dtype} {tuple(t.shape)})')
    return encodings[t.dtype], (int(t.shape[0]), int(t.shape[1]))


def _sides(binary):
    if binary is True or binary is False:
        return bool(binary), bool(binary)
    if binary in ('gt', 'pred'):
        return binary == 'gt', binary == 'pred'
    raise DevaHipError(f"boundary_counts: binary is False, True (both planes), 'gt' or 'pred' (got {binary!r})")


def boundary_counts(gt: torch.Tensor, pred: torch.Tensor, ids, *, bound_th: float = 0.008, radius: Optional[int] = None,
                    pred_lut: Optional[torch.Tensor] = None, binary=False, scratch: Optional[torch.Tensor] = None,
                    out: Optional[torch.Tensor] = None, validate: bool = True) -> torch.Tensor:
    """one frame's records -> uint32 [n,8] device tensor, n = len(ids): per object |gt AND pred|, |gt|, |pred|, the
    boundary pixels of gt and of pred, the matched boundary pixels of gt and of pred, 0 (rules R1-R5 of
    deva_vos_metrics.h).

    `gt`: uint8 or int32 [H,W]; `pred`: those, int64, or the int16 channel plane of `frame_result` together with
    `pred_lut`, uint16 [channels] from channel to the index in `ids` (an entry >= n: none).  `ids`: distinct ascending
    ids in 1 .. 2^31 - 1; a device int32 tensor is copied back to be checked unless `validate=False`.  `binary`: True makes
    every non-zero value of both planes the single object (DAVIS 2016, saliency), 'gt' / 'pred' of that plane alone.
    `radius` overrides the rule of `bound_th` (R3).  More than 64 ids are handled in chunks of 64 calls that share the
    scratch.  `scratch`: a uint8 device tensor of at least `boundary_scratch_bytes(H, W)` bytes to reuse.  Launched on
    the current stream; with host ids or validate=False nothing is synchronised."""
    gt_enc, size = _plane(gt, 'gt', _GT_ENC)
    pred_enc, psize = _plane(pred, 'pred', _PRED_ENC)
    if size != psize:
        raise DevaHipError(f'boundary_counts: gt is {size} and pred {psize}')
    h, w = size
    if h < 1 or w < 1 or h * w > MAX_PIXELS:
        raise DevaHipError(f'boundary_counts: bad plane size {h} x {w}')
    gt_binary, pred_binary = _sides(binary)
    fast = pred_enc == INDEX16
    if fast != (pred_lut is not None):
        raise DevaHipError('boundary_counts: the int16 channel plane and pred_lut go together')
    if fast:
        _planes.check_pred_lut(pred_lut, 'boundary_counts')
    device = gt.device
    table, n = _planes.device_ids(ids, device, 'boundary_counts', 'ids', validate=validate, allow_empty=False,
                                  trusted_must_be_contiguous=False)
    if (gt_binary or pred_binary) and n != 1:
        raise DevaHipError(f'boundary_counts: binary planes hold one object (got {n} ids)')
    if radius is None:
        radius = boundary_radius(h, w, bound_th)
    radius = int(radius)
    if not 0 <= radius <= MAX_RADIUS:
        raise DevaHipError(f'boundary_counts: radius 0 to {MAX_RADIUS} (got {radius})')
    _planes.check_out(out, (n, FIELDS), 'boundary_counts')
    need = boundary_scratch_bytes(h, w)
    if scratch is not None and (scratch.dtype != torch.uint8 or scratch.dim() != 1 or scratch.numel() < need):
        raise DevaHipError(f'boundary_counts: `scratch` must be uint8 [{need}] or longer')
    gt, pred = _planes.on_device(gt, 'gt', 'boundary_counts'), _planes.on_device(pred, 'pred', 'boundary_counts')
    table = _planes.on_device(table, 'ids', 'boundary_counts', 4)
    if fast:
        pred_lut = _planes.on_device(pred_lut, 'pred_lut', 'boundary_counts', 2)
    _planes.check_out_on_device(out, 'boundary_counts')
    if scratch is not None and not (scratch.is_cuda and scratch.is_contiguous() and scratch.data_ptr() % 16 == 0):
        raise DevaHipError('boundary_counts: `scratch` must be a contiguous 16-byte aligned tensor on the HIP device')
    if scratch is None:
        scratch = torch.empty(need, dtype=torch.uint8, device=device)
    counts = torch.empty((n, FIELDS), dtype=torch.uint32, device=device) if out is None else out
    stream = _stream(device)
    for first in range(0, n, MAX_OBJECTS):
        m = min(MAX_OBJECTS, n - first)
        lut = pred_lut
        if fast and n > MAX_OBJECTS:     # the chunk's own indices; the other chunks' objects are none here
            rel = pred_lut.to(torch.int32) - first
            lut = torch.where((rel >= 0) & (rel < m), rel, torch.full_like(rel, 65535)).to(torch.uint16)
        check(lib().deva_vos_boundary_counts(
            gt.data_ptr(), gt_enc | (BINARY if gt_binary else 0), pred.data_ptr(), pred_enc | (BINARY if pred_binary else 0),
            table.data_ptr() + 4 * first, m, lut.data_ptr() if fast else None, lut.numel() if fast else 0, h, w, radius,
            scratch.data_ptr(), scratch.numel(), counts.data_ptr() + 4 * FIELDS * first, stream), 'deva_vos_boundary_counts')
    return counts
