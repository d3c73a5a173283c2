"""ctypes binding of libdeva_lowres.so (C ABI declared in include/deva_lowres.h): the proposal filter and the best-mask
choice of a promptable segmenter taken straight from its low-resolution mask logits (rules L1-L7 of the header).

A SAM-class mask decoder gives [B,256,256] logits; `postprocess_masks` resizes them twice (to model_size, crop, to the
frame) before anything is thresholded.  `proposal_batch` (what `ProposalFilter.add_lowres` calls) and `select_masks`
form the frame-sized values on the fly and leave what `ops.proposal_batch` and `ops.box_mask_select` leave on the
materialised planes, byte for byte; `upsample_logits` is that materialisation (rule L3) for whoever wants the planes.

A tenth library next to libdeva_hip.so, loaded lazily by `lib()`; the conventions are those of `deva.hip.rle_text`:
`check` raises `DevaHipError` with the library's text, there is no CPU path, every launch goes on torch's current stream."""
import ctypes
import os
from ctypes import POINTER, Structure, c_char_p, c_double, c_int, c_int32, c_int64, c_uint32, c_void_p
from typing import NamedTuple, Optional, Tuple

import torch

from . import DevaHipError, _native
from .ops import _stream

__all__ = ['upsample_logits', 'select_masks', 'proposal_batch', 'sam_input_size', 'plan', 'limits', 'PlanInfo', 'LimitInfo',
           'PATH_TILE', 'PATH_POINT', 'MAX_SIDE', 'MAX_PIXELS', 'MAX_PER_BOX']

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'lowres_lib', 'libdeva_lowres.so')   # (csrc/Makefile says why it has a directory of its own)
ABI_VERSION = 1

MAX_SIDE = 4096
MAX_PIXELS = 1 << 30
MAX_PER_BOX = 16
LDS_BUDGET = 61440
MAX_TILE_ROWS = 16
PATH_TILE, PATH_POINT = 0, 1


class Limits(Structure):
    """mirror of `struct deva_lowres_limits` (include/deva_lowres.h)"""
    _fields_ = [('max_side', c_int32), ('max_pixels', c_int32), ('max_per_box', c_int32), ('block', c_int32), ('lds_budget', c_int32),
                ('max_tile_rows', c_int32)]


class Geometry(Structure):
    """mirror of `struct deva_lowres_geometry`"""
    _fields_ = [('low_h', c_int32), ('low_w', c_int32), ('model_size', c_int32), ('in_h', c_int32), ('in_w', c_int32), ('out_h', c_int32),
                ('out_w', c_int32), ('reserved', c_int32)]


class Plan(Structure):
    """mirror of `struct deva_lowres_plan`"""
    _fields_ = [('path', c_int32), ('tile_rows', c_int32), ('tile_cols', c_int32), ('cover_rows', c_int32), ('mid_rows', c_int32),
                ('low_rows', c_int32), ('lds_bytes', c_int32), ('block', c_int32), ('grid_x', c_uint32), ('grid_y_max', c_uint32),
                ('mid_values', c_int64), ('out_values', c_int64)]


# name -> (restype, argtypes); must list every symbol of include/deva_lowres.h
SIGNATURES = {
    'deva_lowres_version': (c_int, []),
    'deva_lowres_last_error': (c_char_p, []),
    'deva_lowres_limits': (c_int, [POINTER(Limits)]),
    'deva_lowres_plan': (c_int, [POINTER(Geometry), POINTER(Plan)]),
    'deva_lowres_upsample': (c_int, [c_void_p, c_int, POINTER(Geometry), c_void_p, c_void_p]),
    'deva_lowres_select': (c_int, [c_void_p, c_void_p, c_int, c_int, POINTER(Geometry), c_double, c_void_p, c_void_p, c_void_p]),
    'deva_lowres_proposal_batch': (c_int, [c_void_p, c_void_p, c_int, POINTER(Geometry), c_double, c_double, c_double, c_double, c_void_p,
                                           c_int, c_void_p, c_int64, c_void_p]),
}

_LIB = None


def lib() -> ctypes.CDLL:
    """Load (once) and return the library; raises if it has not been built."""
    return _LIB or _native.load(globals(), 'deva_lowres_version', 'libdeva_lowres.so', 'the low-resolution filter kernels')


def check(code: int, what: str) -> None:
    if code != 0:
        _native.check(globals(), code, what, 'deva_lowres_last_error')


class LimitInfo(NamedTuple):
    max_side: int        # LH, LW and model_size at most
    max_pixels: int      # pixels of an output plane at most
    max_per_box: int     # candidates per box of `select_masks` at most
    block: int
    lds_budget: int      # bytes of LDS the patch of a workgroup of the tile path may take
    max_tile_rows: int


class PlanInfo(NamedTuple):
    path: int            # PATH_TILE or PATH_POINT
    tile_rows: int       # whole output rows a workgroup owns
    tile_cols: int
    cover_rows: int
    mid_rows: int
    low_rows: int
    lds_bytes: int
    block: int
    grid_x: int
    grid_y_max: int
    mid_values: int
    out_values: int


def limits() -> LimitInfo:
    """what the library takes; host only"""
    out = Limits()
    check(lib().deva_lowres_limits(ctypes.byref(out)), 'deva_lowres_limits')
    return LimitInfo(*(int(getattr(out, f[0])) for f in Limits._fields_))


def sam_input_size(height: int, width: int, model_size: int = 1024) -> Tuple[int, int]:
    """the frame after the segmenter's longest-side resize (segment_anything's ResizeLongestSide.get_preprocess_shape):
    int(x * scale + 0.5) with scale = model_size / max(height, width) in double"""
    scale = float(model_size) / max(int(height), int(width))
    return int(int(height) * scale + 0.5), int(int(width) * scale + 0.5)


def _geometry(fn: str, low_size, input_size, size, model_size) -> Geometry:
    """rule L7 on the sizes, as the library checks them (raised here with the wrapper's name, before anything is allocated)"""
    try:
        lh, lw = (int(v) for v in low_size)
        ih, iw = (int(v) for v in input_size)
        oh, ow = (int(v) for v in size)
        m = int(model_size)
    except (TypeError, ValueError):
        raise DevaHipError(f'{fn}: sizes are pairs of integers (got low {low_size}, input_size {input_size}, size {size})') from None
    if not (1 <= lh <= MAX_SIDE and 1 <= lw <= MAX_SIDE):
        raise DevaHipError(f'{fn}: low-resolution planes of 1 to {MAX_SIDE} rows and columns (got {(lh, lw)})')
    if not 1 <= m <= MAX_SIDE:
        raise DevaHipError(f'{fn}: a model_size of 1 to {MAX_SIDE} (got {m})')
    if not (1 <= ih <= m and 1 <= iw <= m):
        raise DevaHipError(f'{fn}: an input_size within 1 .. model_size = {m} (got {(ih, iw)})')
    if oh < 1 or ow < 1 or oh * ow > MAX_PIXELS:
        raise DevaHipError(f'{fn}: bad output size {(oh, ow)} (1 <= H * W <= 2^30)')
    return Geometry(lh, lw, m, ih, iw, oh, ow, 0)


def plan(low_size: Tuple[int, int], input_size: Tuple[int, int], size: Tuple[int, int], *, model_size: int = 1024) -> PlanInfo:
    """the launch decision for a geometry (include/deva_lowres.h, deva_lowres_plan): which path, the band, the LDS bytes and
    the grid; host only: no device is touched"""
    geo, out = _geometry('plan', low_size, input_size, size, model_size), Plan()
    check(lib().deva_lowres_plan(ctypes.byref(geo), ctypes.byref(out)), 'deva_lowres_plan')
    return PlanInfo(*(int(getattr(out, f[0])) for f in Plan._fields_))


# ------------------------------------------------------------------------------------------ the three calls of the library
def _dev(t: Optional[torch.Tensor], dtype, name: str, fn: str) -> None:
    if t is None:
        return
    if not t.is_cuda:
        raise DevaHipError(f'{fn}: {name} must live on the HIP device (got {t.device}); there is no CPU path')
    if t.dtype != dtype:
        raise DevaHipError(f'{fn}: {name} must be {dtype} (got {t.dtype})')
    if not t.is_contiguous():
        raise DevaHipError(f'{fn}: {name} must be contiguous')


def _launch_upsample(low, geo, out) -> None:
    """deva_lowres_upsample on torch's current stream (the tests' CPU contract replaces the three `_launch_*`)"""
    fn = 'upsample_logits'
    _dev(low, torch.float32, 'low', fn), _dev(out, torch.float32, 'out', fn)
    b = low.shape[0]
    check(lib().deva_lowres_upsample(low.data_ptr() if b else None, b, ctypes.byref(geo), out.data_ptr() if b else None,
                                     _stream(low.device)), 'deva_lowres_upsample')


def _launch_select(low, scores, geo, threshold, out, chosen) -> None:
    fn = 'select_masks'
    _dev(low, torch.float32, 'low', fn), _dev(scores, torch.float32, 'scores', fn)
    _dev(out, torch.uint8, 'out', fn), _dev(chosen, torch.int32, 'chosen', fn)
    b, m = low.shape[0], low.shape[1]
    check(lib().deva_lowres_select(low.data_ptr() if b else None, scores.data_ptr() if b and scores is not None else None, b, m,
                                   ctypes.byref(geo), threshold, out.data_ptr() if b else None, chosen.data_ptr() if b else None,
                                   _stream(low.device)), 'deva_lowres_select')


def _launch_proposal_batch(state, low, iou_preds, geo, thresholds) -> None:
    fn = 'proposal_batch'
    _dev(low, torch.float32, 'low', fn), _dev(iou_preds, torch.float32, 'iou_preds', fn)
    b = low.shape[0]
    check(lib().deva_lowres_proposal_batch(low.data_ptr() if b else None, iou_preds.data_ptr() if b else None, b, ctypes.byref(geo),
                                           thresholds['pred_iou_thresh'], thresholds['stability_score_thresh'],
                                           thresholds['stability_score_offset'], thresholds['mask_threshold'], state.arena.data_ptr(),
                                           state.capacity, state.scratch.data_ptr(), state.scratch_bytes, _stream(state.arena.device)),
          'deva_lowres_proposal_batch')


# ------------------------------------------------------------------------------------------ public
def upsample_logits(low: torch.Tensor, input_size: Tuple[int, int], size: Tuple[int, int], *, model_size: int = 1024,
                    out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp32 [B,LH,LW] low-resolution logits on the device -> fp32 [B,H,W] at `size`: rule L3 materialised, what
    `postprocess_masks(low, input_size, size)` means (bilinear to model_size, crop to `input_size`, bilinear to `size`),
    every operation a rounded fp32 one.  One launch per 65535 planes, nothing synchronises.  `out`: the caller's contiguous
    fp32 [B,H,W] device tensor."""
    fn = 'upsample_logits'
    if low.dim() != 3:
        raise DevaHipError(f'{fn}: [B,LH,LW] logits expected (got {tuple(low.shape)})')
    geo = _geometry(fn, low.shape[1:], input_size, size, model_size)
    shape = (low.shape[0], geo.out_h, geo.out_w)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=low.device)
    elif out.dtype != torch.float32 or tuple(out.shape) != shape:
        raise DevaHipError(f'{fn}: `out` must be fp32 {list(shape)} (got {out.dtype} {tuple(out.shape)})')
    _launch_upsample(low, geo, out)
    return out


def select_masks(low: torch.Tensor, scores: Optional[torch.Tensor], input_size: Tuple[int, int], size: Tuple[int, int], *,
                 threshold: float = 0.0, model_size: int = 1024, out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """fp32 [B,M,LH,LW] low-resolution candidate logits of B box prompts and their fp32 [B,M] scores on the device ->
    (planes uint8 [B,H,W] 0 / 1 at `size`, chosen int32 [B]) on the device: `ops.box_mask_select` on the planes of rule L3
    (rule L6), without those planes.  Only the chosen candidates are evaluated; one launch, nothing synchronises.
    `scores=None` with M = 1 is a plain threshold.  `out`: the caller's contiguous uint8 [B,H,W] device tensor at any
    alignment, e.g. a slice of an arena."""
    fn = 'select_masks'
    if low.dim() != 4:
        raise DevaHipError(f'{fn}: [B,M,LH,LW] logits expected (got {tuple(low.shape)})')
    b, m = low.shape[0], low.shape[1]
    if not 1 <= m <= MAX_PER_BOX:
        raise DevaHipError(f'{fn}: 1 to {MAX_PER_BOX} planes per box (got {m})')
    if scores is None:
        if m != 1:
            raise DevaHipError(f'{fn}: scores may be None only with one plane per box (got {m})')
    elif tuple(scores.shape) != (b, m):
        raise DevaHipError(f'{fn}: scores must be fp32 [{b},{m}] (got {tuple(scores.shape)})')
    threshold = float(threshold)
    if threshold != threshold:
        raise DevaHipError(f'{fn}: the mask threshold is not a number')
    geo = _geometry(fn, low.shape[2:], input_size, size, model_size)
    shape = (b, geo.out_h, geo.out_w)
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=low.device)
    elif out.dtype != torch.uint8 or tuple(out.shape) != shape:
        raise DevaHipError(f'{fn}: `out` must be uint8 {list(shape)} (got {out.dtype} {tuple(out.shape)})')
    chosen = torch.empty(b, dtype=torch.int32, device=low.device)
    _launch_select(low, scores, geo, threshold, out, chosen)
    return out, chosen


def proposal_batch(state, low: torch.Tensor, iou_preds: torch.Tensor, input_size: Tuple[int, int], *, model_size: int = 1024,
                   pred_iou_thresh: float, stability_score_thresh: float, stability_score_offset: float, mask_threshold: float) -> None:
    """one batch of a segmenter into the frame of `state` (`ops.proposal_state`, begun by `ops.proposal_begin`): `low` fp32
    [B,LH,LW] and `iou_preds` fp32 [B] on the device.  What `ops.proposal_batch` leaves on the planes of rule L3 (rule L5),
    without those planes; a frame may mix both.  Three launches per 1024 planes, nothing synchronises; B = 0 is fine."""
    fn = 'proposal_batch'
    if low.dim() != 3:
        raise DevaHipError(f'{fn}: [B,LH,LW] low-resolution logits expected (got {tuple(low.shape)})')
    b = low.shape[0]
    if tuple(iou_preds.shape) != (b,):
        raise DevaHipError(f'{fn}: iou_preds must be fp32 [{b}] (got {tuple(iou_preds.shape)})')
    geo = _geometry(fn, low.shape[1:], input_size, (state.height, state.width), model_size)
    thresholds = dict(pred_iou_thresh=float(pred_iou_thresh), stability_score_thresh=float(stability_score_thresh),
                      stability_score_offset=float(stability_score_offset), mask_threshold=float(mask_threshold))
    if any(v != v for v in thresholds.values()):
        raise DevaHipError(f'{fn}: a threshold is not a number')
    _launch_proposal_batch(state, low, iou_preds, geo, thresholds)
