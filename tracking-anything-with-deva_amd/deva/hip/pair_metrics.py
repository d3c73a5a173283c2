"""ctypes binding of libdeva_pair_metrics.so (C ABI declared in include/deva_pair_metrics.h): the counts of every
(ground-truth object, proposal) pair of a frame, from which the unsupervised DAVIS protocol takes J and F of each pair
before it assigns proposals to objects.

A fourth library next to libdeva_hip.so, libdeva_metrics.so and libdeva_vos_metrics.so, loaded lazily by `lib()`; the
conventions are those of `deva.hip.vos_metrics`: `check` raises `DevaHipError` with the library's text, host tensors are
refused, there is no CPU path."""
import ctypes
import os
from ctypes import POINTER, Structure, c_char_p, c_int, c_int32, c_int64, c_uint32, c_void_p
from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch

from . import DevaHipError, _native, _planes, vos_metrics
from .ops import _stream

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libdeva_pair_metrics.so')
ABI_VERSION = 1

U8, I32, I64, INDEX16 = 0, 1, 2, 3
MAX_OBJECTS = 64
MAX_RADIUS = 128
MAX_PIXELS = 1 << 30
SINGLE_FIELDS = 2
FIELDS = 4
STRIP = 8
INNER_RADIUS = 3
# the fields of `singles` and of `pairs` (P5)
AREA, BOUNDARY = range(2)
INTER, GT_MATCHED, PRED_MATCHED = range(3)


class Plan(Structure):
    """mirror of `struct deva_pair_plan` (include/deva_pair_metrics.h)"""
    _fields_ = [('label_grid', c_uint32), ('match_grid', c_uint32), ('block', c_uint32), ('label_lds_bytes', c_uint32),
                ('match_lds_bytes', c_uint32), ('inner_radius', c_int32), ('wave_search', c_int32), ('radius', c_int32),
                ('scratch_bytes', c_int64)]


# name -> (restype, argtypes); must list every symbol of include/deva_pair_metrics.h
SIGNATURES = {
    'deva_pair_version': (c_int, []),
    'deva_pair_last_error': (c_char_p, []),
    'deva_pair_scratch_bytes': (c_int, [c_int, c_int, POINTER(c_int64)]),
    'deva_pair_plan': (c_int, [c_int, c_int, c_int, c_int, c_int, POINTER(Plan)]),
    'deva_pair_counts': (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_int,
                                 c_int, c_void_p, c_int64, c_void_p, c_void_p, c_void_p]),
}

_LIB = None


def lib() -> ctypes.CDLL:
    """Load (once) and return the pair scoring library; raises if it has not been built."""
    return _LIB or _native.load(globals(), 'deva_pair_version', 'libdeva_pair_metrics.so', 'the pair scoring kernels')


def check(code: int, what: str) -> None:
    if code != 0:
        _native.check(globals(), code, what, 'deva_pair_last_error')


class PlanInfo(NamedTuple):
    label_grid: int        # workgroups of the pass over the planes
    match_grid: int        # workgroups of the disk search
    block: int
    label_lds_bytes: int
    match_lds_bytes: int
    inner_radius: int
    wave_search: int       # 1: the wave's lanes search a pixel's disk together (radius > INNER_RADIUS)
    radius: int
    scratch_bytes: int


def pair_scratch_bytes(height: int, width: int) -> int:
    n = c_int64()
    check(lib().deva_pair_scratch_bytes(int(height), int(width), ctypes.byref(n)), 'deva_pair_scratch_bytes')
    return int(n.value)


def pair_plan(height: int, width: int, n_gt: int, n_pred: int, radius: int) -> PlanInfo:
    """the two launches `pair_counts` makes for these sizes (host only: no device is touched)"""
    plan = Plan()
    check(lib().deva_pair_plan(int(height), int(width), int(n_gt), int(n_pred), int(radius), ctypes.byref(plan)), 'deva_pair_plan')
    return PlanInfo(*(int(getattr(plan, f[0])) for f in Plan._fields_))


# ------------------------------------------------------------------------------------------ the pair table
_GT_ENC = {torch.uint8: U8, torch.int32: I32}
_PRED_ENC = {torch.uint8: U8, torch.int32: I32, torch.int64: I64, torch.int16: INDEX16}


def id_list(ids, what: str = 'ids') -> np.ndarray:
    """`ids` as the caller gives them -> int32 [n], checked: distinct, ascending, in 1 .. 2^31 - 1, 1 to 64 of them"""
    return _planes.host_ids(ids, 'pair_counts', what, allow_empty=False, max_ids=MAX_OBJECTS)


def _plane(t, name: str, encodings):
    if not isinstance(t, torch.Tensor):
        raise DevaHipError(f'pair_counts: {name} must be a tensor (got {type(t).__name__})')
    if t.dim() != 2 or t.dtype not in encodings:
        raise DevaHipError(f'pair_counts: {name} must be an [H,W] plane of {", ".join(str(d) for d in encodings)} '
                           f'(got {t.dtype} {tuple(t.shape)})')
    return encodings[t.dtype], (int(t.shape[0]), int(t.shape[1]))


def _arguments(gt, pred, gt_ids, pred_ids, radius, bound_th, pred_lut, out):
    """the checks that need no device (tests/emu_pairs.py, the CPU contract, makes them too)
    -> (gt_enc, pred_enc, (h, w), fast, radius)"""
    gt_enc, size = _plane(gt, 'gt', _GT_ENC)
    pred_enc, psize = _plane(pred, 'pred', _PRED_ENC)
    if size != psize:
        raise DevaHipError(f'pair_counts: gt is {size} and pred {psize}')
    h, w = size
    if h < 1 or w < 1 or h * w > MAX_PIXELS:
        raise DevaHipError(f'pair_counts: bad plane size {h} x {w}')
    fast = pred_enc == INDEX16
    if fast != (pred_lut is not None):
        raise DevaHipError('pair_counts: the int16 channel plane and pred_lut go together')
    if fast:
        _planes.check_pred_lut(pred_lut, 'pair_counts')
    if pred_ids is None:
        raise DevaHipError('pair_counts: pred_ids is needed: the ids of the proposals (with the channel plane, what pred_lut indexes)')
    if radius is None:
        radius = vos_metrics.boundary_radius(h, w, bound_th)
    radius = int(radius)
    if not 0 <= radius <= MAX_RADIUS:
        raise DevaHipError(f'pair_counts: radius 0 to {MAX_RADIUS} (got {radius})')
    if out is not None and not (isinstance(out, (tuple, list)) and len(out) == 2):
        raise DevaHipError('pair_counts: `out` is a pair (singles, pairs)')
    return gt_enc, pred_enc, (h, w), fast, radius


def _check_outs(out, n_gt: int, n_pred: int) -> None:
    if out is not None:
        _planes.check_out(out[0], (n_gt + n_pred, SINGLE_FIELDS), 'pair_counts')
        if out[1] is None or out[1].dtype != torch.uint32 or tuple(out[1].shape) != (n_gt, n_pred, FIELDS):
            raise DevaHipError(f'pair_counts: `out[1]` must be uint32 [{n_gt},{n_pred},{FIELDS}]')
        if out[0] is None:
            raise DevaHipError(f'pair_counts: `out[0]` must be uint32 [{n_gt + n_pred},{SINGLE_FIELDS}]')


def pair_counts(gt: torch.Tensor, pred: torch.Tensor, gt_ids, pred_ids=None, *, bound_th: float = 0.008, radius: Optional[int] = None,
                pred_lut: Optional[torch.Tensor] = None, scratch: Optional[torch.Tensor] = None, out=None,
                validate: bool = True) -> Tuple[torch.Tensor, torch.Tensor]:
    """one frame's pair table -> (singles uint32 [n_gt + n_pred, 2], pairs uint32 [n_gt, n_pred, 4]) on the device:
    per object and proposal (ground truth first) the area and the boundary pixels; per pair |gt_g AND pred_p|, the
    boundary pixels of gt_g matched by p, those of pred_p matched by g, 0 (rules P1-P5 of deva_pair_metrics.h).

    `gt`: uint8 or int32 [H,W]; `pred`: those, int64, or the int16 channel plane of `frame_result` together with
    `pred_lut`, uint16 [channels] from channel to the index in `pred_ids` (an entry >= n_pred: none).  `gt_ids`,
    `pred_ids`: each distinct ascending ids in 1 .. 2^31 - 1, 1 to 64 of them, independent of each other (more than 64 on
    either side raises: the protocol allows 20 proposals); a device int32 tensor is copied back to be checked unless
    `validate=False`.  With the channel plane `pred_ids` only says how many proposals there are: an int will do.
    `radius` overrides the rule of `bound_th` (R3 of deva_vos_metrics.h).  `scratch`: a uint8 device tensor of at least
    `pair_scratch_bytes(H, W)` bytes to reuse.  `out`: (singles, pairs) to write into.  Launched on the current stream;
    with host ids or validate=False nothing is synchronised."""
    gt_enc, pred_enc, (h, w), fast, radius = _arguments(gt, pred, gt_ids, pred_ids, radius, bound_th, pred_lut, out)
    device = gt.device
    table_g, n_gt = _planes.device_ids(gt_ids, device, 'pair_counts', 'gt_ids', validate=validate, allow_empty=False,
                                       max_ids=MAX_OBJECTS, trusted_must_be_contiguous=False)
    if fast and isinstance(pred_ids, int):
        table_p, n_pred = None, pred_ids
        if not 1 <= n_pred <= MAX_OBJECTS:
            raise DevaHipError(f'pair_counts: at most {MAX_OBJECTS} pred_ids, at least one (got {n_pred})')
    else:
        table_p, n_pred = _planes.device_ids(pred_ids, device, 'pair_counts', 'pred_ids', validate=validate, allow_empty=False,
                                             max_ids=MAX_OBJECTS, trusted_must_be_contiguous=False)
    _check_outs(out, n_gt, n_pred)
    need = pair_scratch_bytes(h, w)
    if scratch is not None and (scratch.dtype != torch.uint8 or scratch.dim() != 1 or scratch.numel() < need):
        raise DevaHipError(f'pair_counts: `scratch` must be uint8 [{need}] or longer')
    gt, pred = _planes.on_device(gt, 'gt', 'pair_counts'), _planes.on_device(pred, 'pred', 'pair_counts')
    table_g = _planes.on_device(table_g, 'gt_ids', 'pair_counts', 4)
    if fast:
        pred_lut, table_p = _planes.on_device(pred_lut, 'pred_lut', 'pair_counts', 2), None
    else:
        table_p = _planes.on_device(table_p, 'pred_ids', 'pair_counts', 4)
    if out is not None:
        _planes.check_out_on_device(out[0], 'pair_counts')
        _planes.check_out_on_device(out[1], 'pair_counts')
    if scratch is not None and not (scratch.is_cuda and scratch.is_contiguous() and scratch.data_ptr() % 16 == 0):
        raise DevaHipError('pair_counts: `scratch` must be a contiguous 16-byte aligned tensor on the HIP device')
    if scratch is None:
        scratch = torch.empty(need, dtype=torch.uint8, device=device)
    if out is None:
        out = (torch.empty((n_gt + n_pred, SINGLE_FIELDS), dtype=torch.uint32, device=device),
               torch.empty((n_gt, n_pred, FIELDS), dtype=torch.uint32, device=device))
    singles, pairs = out
    check(lib().deva_pair_counts(gt.data_ptr(), gt_enc, table_g.data_ptr(), n_gt, pred.data_ptr(), pred_enc,
                                 None if fast else table_p.data_ptr(), n_pred, pred_lut.data_ptr() if fast else None,
                                 pred_lut.numel() if fast else 0, h, w, radius, scratch.data_ptr(), scratch.numel(),
                                 singles.data_ptr(), pairs.data_ptr(), _stream(device)), 'deva_pair_counts')
    return singles, pairs
