"""ctypes binding of libdeva_metrics.so (C ABI declared in include/deva_metrics.h): the scoring side of a VIPSeg run.

A library of its own next to libdeva_hip.so (scoring is evaluation, not inference), loaded lazily by `lib()`; the
conventions are those of `deva.hip`: `check` raises `DevaHipError` with the library's text, host tensors are refused,
there is no CPU path."""
import ctypes
import os
from ctypes import POINTER, Structure, c_char_p, c_int, c_int32, c_uint32, c_void_p
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import DevaHipError, _native, _planes
from .ops import _stream

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libdeva_metrics.so')
ABI_VERSION = 1

RGB8, I32, I64, INDEX16 = 0, 1, 2, 3
MAX_IDS = 1022
MAX_PIXELS = 1 << 30
STRIP = 16
LDS_LIMIT = 65536
PATHS = ('lds', 'global')


class Plan(Structure):
    """mirror of `struct deva_metrics_plan` (include/deva_metrics.h)"""
    _fields_ = [('path', c_int32), ('grid', c_uint32), ('block', c_uint32), ('lds_bytes', c_uint32)]


# name -> (restype, argtypes); must list every symbol of include/deva_metrics.h
SIGNATURES = {
    'deva_metrics_version': (c_int, []),
    'deva_metrics_last_error': (c_char_p, []),
    'deva_metrics_panoptic_plan': (c_int, [c_int, c_int, c_int, c_int, POINTER(Plan)]),
    'deva_metrics_panoptic_counts': (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int,
                                             c_int, c_int, c_void_p, c_void_p]),
}

_LIB = None


def lib() -> ctypes.CDLL:
    """Load (once) and return the scoring library; raises if it has not been built."""
    return _LIB or _native.load(globals(), 'deva_metrics_version', 'libdeva_metrics.so', 'the scoring kernels')


def check(code: int, what: str) -> None:
    if code != 0:   # (tested here: the inference wrappers call this after every launch)
        _native.check(globals(), code, what, 'deva_metrics_last_error')


class PlanInfo(NamedTuple):
    path: str        # 'lds': runs are added to a per-workgroup table in LDS; 'global': to the result directly
    grid: int
    block: int
    lds_bytes: int


def panoptic_plan(height: int, width: int, n_gt: int, n_pred: int) -> PlanInfo:
    """the launch `panoptic_counts` makes for these sizes (host only: no device is touched)"""
    plan = Plan()
    check(lib().deva_metrics_panoptic_plan(int(height), int(width), int(n_gt), int(n_pred), ctypes.byref(plan)),
          'deva_metrics_panoptic_plan')
    return PlanInfo(PATHS[plan.path], int(plan.grid), int(plan.block), int(plan.lds_bytes))


# ------------------------------------------------------------------------------------------ the joint count
def id_table(ids, what: str = 'ids') -> np.ndarray:
    """the sorted table of distinct ids that `panoptic_counts` wants, from any iterable of ids: 0 is dropped (it has
    slot 0 of its own), duplicates collapse -> int32 [n], ascending.  slot of id = 2 + index in the table."""
    a = np.unique(np.asarray(list(ids) if not isinstance(ids, (np.ndarray, torch.Tensor)) else
                             (ids.cpu().numpy() if isinstance(ids, torch.Tensor) else ids), dtype=np.int64).reshape(-1))
    a = a[a != 0]
    if a.size and (a[0] < 0 or a[-1] > 2**31 - 1):
        raise DevaHipError(f'{what}: ids must lie in 1 .. 2^31 - 1 (got {int(a[0])} .. {int(a[-1])})')
    if a.size > MAX_IDS:
        raise DevaHipError(f'{what}: at most {MAX_IDS} ids (got {a.size})')
    return a.astype(np.int32)


def _table(ids, device, what: str, validate: bool = True):
    """`ids` as given by the caller -> (device int32 tensor or None, n); a tensor or array is taken as the table itself
    and must be strictly ascending and positive"""
    if ids is None:
        return None, 0
    return _planes.device_ids(ids, device, 'panoptic_counts', what, validate=validate, allow_empty=True, max_ids=MAX_IDS,
                              trusted_must_be_contiguous=True)


def _plane(t: torch.Tensor, name: str, allowed):
    """-> (tensor to pass, encoding, (H, W))"""
    if not isinstance(t, torch.Tensor):
        raise DevaHipError(f'panoptic_counts: {name} must be a tensor (got {type(t).__name__})')
    if t.dtype == torch.uint8 and t.dim() == 3 and t.shape[2] == 3:
        enc = RGB8
    elif t.dim() == 2 and t.dtype in (torch.int32, torch.int64, torch.int16):
        enc = {torch.int32: I32, torch.int64: I64, torch.int16: INDEX16}[t.dtype]
    else:
        raise DevaHipError(f'panoptic_counts: {name} must be uint8 [H,W,3] or an integer [H,W] plane '
                           f'(got {t.dtype} {tuple(t.shape)})')
    if enc not in allowed:
        raise DevaHipError(f'panoptic_counts: {name} cannot be {t.dtype}')
    return t, enc, (int(t.shape[0]), int(t.shape[1]))


def panoptic_counts(gt: torch.Tensor, gt_ids, pred: torch.Tensor, pred_ids=None, pred_lut: Optional[torch.Tensor] = None,
                    *, out: Optional[torch.Tensor] = None, validate: bool = True) -> torch.Tensor:
    """one frame's joint count -> uint32 [G,P] device tensor, G = len(gt_ids) + 2, P = len(pred_ids) + 2:
    counts[g][p] = pixels whose ground-truth slot is g and predicted slot is p, where on either side slot 0 is id 0,
    slot 1 any id that the table does not list and slot 2 + i the table's i-th id (rules C1-C4 of deva_metrics.h).

    `gt`: uint8 [H,W,3] (the PNG's bytes) or int32 [H,W].  `pred`: those, int64 [H,W], or the int16 channel plane of
    `frame_result` together with `pred_lut`, uint16 [channels] from channel to slot (then `pred_ids` only gives P: a table
    or its length).  Tables are ascending distinct ids in 1 .. 2^31 - 1 (`id_table` makes one); one given as a device
    tensor is copied back to be checked unless `validate=False` (the caller built it sorted).  Launched on the current
    stream; with host tables or validate=False nothing is synchronised."""
    gt, gt_enc, size = _plane(gt, 'gt', (RGB8, I32))
    pred, pred_enc, psize = _plane(pred, 'pred', (RGB8, I32, I64, INDEX16))
    if size != psize:
        raise DevaHipError(f'panoptic_counts: gt is {size} and pred {psize}')
    if size[0] < 1 or size[1] < 1 or size[0] * size[1] > MAX_PIXELS:
        raise DevaHipError(f'panoptic_counts: bad plane size {size[0]} x {size[1]}')
    fast = pred_enc == INDEX16
    if fast != (pred_lut is not None):
        raise DevaHipError('panoptic_counts: the int16 channel plane and pred_lut go together')
    device = gt.device
    gt_tab, n_gt = _table(gt_ids, device, 'gt_ids', validate)
    if fast and isinstance(pred_ids, int):
        pred_tab, n_pred = None, pred_ids
        if not 0 <= n_pred <= MAX_IDS:
            raise DevaHipError(f'panoptic_counts: at most {MAX_IDS} pred_ids (got {n_pred})')
    else:
        pred_tab, n_pred = _table(pred_ids, device, 'pred_ids', validate)
    if fast:
        _planes.check_pred_lut(pred_lut, 'panoptic_counts')
    g, p = n_gt + 2, n_pred + 2
    _planes.check_out(out, (g, p), 'panoptic_counts')
    gt, pred = _planes.on_device(gt, 'gt', 'panoptic_counts'), _planes.on_device(pred, 'pred', 'panoptic_counts')
    if fast:
        pred_lut = _planes.on_device(pred_lut, 'pred_lut', 'panoptic_counts')
    _planes.check_out_on_device(out, 'panoptic_counts')
    counts = torch.empty((g, p), dtype=torch.uint32, device=device) if out is None else out
    check(lib().deva_metrics_panoptic_counts(
        gt.data_ptr(), gt_enc, None if gt_tab is None else gt_tab.data_ptr(), n_gt,
        pred.data_ptr(), pred_enc, None if pred_tab is None or fast else pred_tab.data_ptr(), n_pred,
        pred_lut.data_ptr() if fast else None, pred_lut.numel() if fast else 0, size[0], size[1], counts.data_ptr(),
        _stream(device)), 'deva_metrics_panoptic_counts')
    return counts
