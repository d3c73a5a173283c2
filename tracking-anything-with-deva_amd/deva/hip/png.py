"""ctypes binding of libdeva_png.so (C ABI declared in include/deva_png.h): the PNG files of the savers from a zlib stream
that the device codes from a byte plane (rules Z1-Z8 of the header).

`deflate` gives the zlib stream of a plane (`Up` filter on every row, runs of equal bytes as matches at distance 1, the
fixed Huffman code, segments of `plan().rows_per_segment` rows), `encode` a complete PNG file around it.  The file's
frame -- signature, IHDR, PLTE, one IDAT, IEND and the CRC of every chunk (`zlib.crc32` over the copied stream, tens of
KB for an id map) -- is written on the HOST; only the stream comes from the device.

An eleventh library next to libdeva_hip.so, loaded lazily by `lib()`; the conventions are those of `deva.hip.lowres`:
`check` raises `DevaHipError` with the library's text, there is no CPU path, every launch goes on torch's current stream
(or on `stream=`)."""
import contextlib
import ctypes
import os
import struct
import zlib
from ctypes import POINTER, Structure, c_char_p, c_int, c_int32, c_int64, c_void_p
from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch

from . import DevaHipError, _native
from ._pending import record_event, require_on_device, to_pinned
from .ops import _stream

__all__ = ['encode', 'deflate', 'plan', 'limits', 'file_bytes', 'PendingPng', 'PlanInfo', 'LimitInfo', 'MAX_SIDE', 'MAX_BYTES',
           'ROWS_PER_SEGMENT', 'STEP']

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'png_lib', 'libdeva_png.so')   # (csrc/Makefile says why it has a directory of its own)
ABI_VERSION = 1

MAX_SIDE = 16384
MAX_BYTES = 1 << 29
ROWS_PER_SEGMENT = 8
STEP = 1024
SIGNATURE = b'\x89PNG\r\n\x1a\n'


class Limits(Structure):
    """mirror of `struct deva_png_limits` (include/deva_png.h)"""
    _fields_ = [('max_side', c_int32), ('max_bytes', c_int32), ('rows_per_segment', c_int32), ('step', c_int32), ('block', c_int32),
                ('lds_bytes', c_int32)]


class Plan(Structure):
    """mirror of `struct deva_png_plan`"""
    _fields_ = [('rows_per_segment', c_int32), ('segments', c_int32), ('row_bytes', c_int32), ('steps_per_row', c_int32), ('block', c_int32),
                ('reserved', c_int32), ('slot_bytes', c_int64), ('scratch_bytes', c_int64), ('worst_case', c_int64)]


# name -> (restype, argtypes); must list every symbol of include/deva_png.h
SIGNATURES = {
    'deva_png_version': (c_int, []),
    'deva_png_last_error': (c_char_p, []),
    'deva_png_limits': (c_int, [POINTER(Limits)]),
    'deva_png_plan': (c_int, [c_int, c_int, c_int, POINTER(Plan)]),
    'deva_png_deflate': (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p]),
    'deva_png_place': (c_int, [c_int, c_int, c_int, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p]),
}

_LIB = None


def lib() -> ctypes.CDLL:
    """Load (once) and return the library; raises if it has not been built."""
    return _LIB or _native.load(globals(), 'deva_png_version', 'libdeva_png.so', 'the PNG coder kernels')


def check(code: int, what: str) -> None:
    if code != 0:
        _native.check(globals(), code, what, 'deva_png_last_error')


class LimitInfo(NamedTuple):
    max_side: int            # H and W at most
    max_bytes: int           # H * W * bpp at most
    rows_per_segment: int    # R
    step: int                # bytes of a row string a workgroup takes in one step
    block: int
    lds_bytes: int


class PlanInfo(NamedTuple):
    rows_per_segment: int    # R of rule Z5
    segments: int
    row_bytes: int           # W * bpp
    steps_per_row: int
    block: int
    slot_bytes: int          # a segment's slot in the scratch
    scratch_bytes: int       # the scratch of one call
    worst_case: int          # a capacity no plane of this size exceeds (Z7)


def limits() -> LimitInfo:
    """what the library takes; host only"""
    out = Limits()
    check(lib().deva_png_limits(ctypes.byref(out)), 'deva_png_limits')
    return LimitInfo(*(int(getattr(out, f[0])) for f in Limits._fields_))


def _sizes(fn: str, height, width, bpp) -> Tuple[int, int, int]:
    """rule Z1 on the sizes, as the library checks them (raised here with the wrapper's name, before anything is allocated)"""
    try:
        h, w, b = int(height), int(width), int(bpp)
    except (TypeError, ValueError):
        raise DevaHipError(f'{fn}: height, width and bpp are integers (got {height!r}, {width!r}, {bpp!r})') from None
    if b not in (1, 3):
        raise DevaHipError(f'{fn}: bpp: 1 ([H,W]) or 3 ([H,W,3]) bytes a pixel (got {b})')
    if not (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE):
        raise DevaHipError(f'{fn}: bad height x width {h} x {w} (1 to {MAX_SIDE} each)')
    if h * w * b > MAX_BYTES:
        raise DevaHipError(f'{fn}: a plane of {h} x {w} x {b} bytes, a call takes {MAX_BYTES}')
    return h, w, b


def plan(height: int, width: int, bpp: int = 1) -> PlanInfo:
    """R, the segment count, the scratch bytes and the worst-case capacity for a plane; host only: no device is touched"""
    h, w, b = _sizes('plan', height, width, bpp)
    out = Plan()
    check(lib().deva_png_plan(h, w, b, ctypes.byref(out)), 'deva_png_plan')
    return PlanInfo(*(int(getattr(out, f[0])) for f in Plan._fields_ if f[0] != 'reserved'))


# ------------------------------------------------------------------------------------------ the two calls of the library
def _launch_deflate(plane, h, w, bpp, scratch, out, capacity, info) -> None:
    """deva_png_deflate on the current stream of the plane's device (the tests' CPU contract replaces the two `_launch_*`)"""
    fn = 'deflate'
    for name, t in (('plane', plane), ('scratch', scratch), ('out', out), ('info', info)):
        require_on_device(t, name, fn)
    with torch.cuda.device(plane.device):
        check(lib().deva_png_deflate(plane.data_ptr(), h, w, bpp, scratch.data_ptr(), scratch.numel(), out.data_ptr() if capacity else None,
                                     capacity, info.data_ptr(), _stream(plane.device)), 'deva_png_deflate')


def _launch_place(h, w, bpp, scratch, out, capacity, info) -> None:
    fn = 'deflate'
    for name, t in (('scratch', scratch), ('out', out), ('info', info)):
        require_on_device(t, name, fn)
    with torch.cuda.device(scratch.device):
        check(lib().deva_png_place(h, w, bpp, scratch.data_ptr(), scratch.numel(), out.data_ptr() if capacity else None, capacity,
                                   info.data_ptr(), _stream(scratch.device)), 'deva_png_place')


# ------------------------------------------------------------------------------------------ the file around the stream (host)
def _chunk(kind: bytes, data: bytes) -> bytes:
    return struct.pack('>I', len(data)) + kind + data + struct.pack('>I', zlib.crc32(kind + data) & 0xffffffff)


def file_bytes(stream: bytes, height: int, width: int, bpp: int = 1, palette: Optional[bytes] = None) -> bytes:
    """a zlib stream of the `Up`-filtered rows -> the PNG file: colour type 0 for [H,W], 3 for [H,W] with a palette, 2 for
    [H,W,3]; 8 bits a sample, no interlace, one IDAT.  Host only."""
    color = 2 if bpp == 3 else (0 if palette is None else 3)
    parts = [SIGNATURE, _chunk(b'IHDR', struct.pack('>IIBBBBB', int(width), int(height), 8, color, 0, 0, 0))]
    if palette is not None:
        parts.append(_chunk(b'PLTE', palette))
    parts += [_chunk(b'IDAT', stream), _chunk(b'IEND', b'')]
    return b''.join(parts)


def _plane(fn: str, plane) -> Tuple[int, int, int]:
    if not isinstance(plane, torch.Tensor):
        raise DevaHipError(f'{fn}: the plane is a uint8 tensor [H,W] or [H,W,3] on the HIP device (got {type(plane).__name__})')
    if plane.dtype != torch.uint8:
        raise DevaHipError(f'{fn}: plane must be {torch.uint8} (got {plane.dtype})')
    if not (plane.dim() == 2 or (plane.dim() == 3 and plane.shape[2] == 3)):
        raise DevaHipError(f'{fn}: [H,W] or [H,W,3] expected (got {tuple(plane.shape)})')
    if not plane.is_contiguous():
        raise DevaHipError(f'{fn}: plane must be contiguous')
    return _sizes(fn, plane.shape[0], plane.shape[1], 3 if plane.dim() == 3 else 1)


def _palette(fn: str, palette, bpp: int) -> Optional[bytes]:
    """a palette as PIL's putpalette takes it (bytes, or a flat sequence of 0 .. 255) -> bytes: whole triples, 768 at most"""
    if palette is None:
        return None
    if bpp != 1:
        raise DevaHipError(f'{fn}: a palette belongs to an [H,W] plane')
    try:
        data = bytes(palette) if isinstance(palette, (bytes, bytearray, memoryview)) else np.asarray(palette).astype(np.uint8, casting='unsafe').tobytes()
    except (TypeError, ValueError):
        raise DevaHipError(f'{fn}: palette: bytes or a flat sequence of 0 .. 255 (got {type(palette).__name__})') from None
    if len(data) == 0 or len(data) > 768 or len(data) % 3:
        raise DevaHipError(f'{fn}: palette: 1 to 256 RGB triples, 768 bytes at most (got {len(data)} bytes)')
    return data


class PendingPng:
    """one `encode` / `deflate` with `capacity=`: the kernels and the copies of `info` and of the first `capacity` bytes of
    the stream are in flight on the caller's stream; `finish()` waits for them.  The coded segments stay in the scratch
    on the device until then, so a stream above `capacity` is placed again at its exact size and copied: never truncated."""

    def __init__(self, geometry, palette, as_file, scratch, out, info, capacity, host_out, host_info, event):
        self.geometry, self.capacity = geometry, capacity
        self._palette, self._as_file = palette, as_file
        self._scratch, self._out, self._info, self._host_out, self._host_info, self._event = scratch, out, info, host_out, host_info, event
        self._result = None
        self.total = self.adler = self.segments = None
        self.overflowed = None

    def finish(self) -> bytes:
        if self._result is None:
            if self._event is not None:
                self._event.synchronize()
            total, adler, over, segments = (int(v) for v in self._host_info.tolist())
            self.total, self.adler, self.overflowed, self.segments = total, adler, bool(over), segments
            if over:   # (rare: the saver's capacity is twice the largest stream seen so far)
                h, w, bpp = self.geometry
                device = self._scratch.device
                with torch.cuda.device(device) if device.type == 'cuda' else contextlib.nullcontext():
                    out = torch.empty(total, dtype=torch.uint8, device=device)
                    _launch_place(h, w, bpp, self._scratch, out, total, self._info)
                    stream = out.cpu().numpy().tobytes()
            else:
                stream = self._host_out.numpy()[:total].tobytes()
            self._result = file_bytes(stream, *self.geometry, self._palette) if self._as_file else stream
            self._scratch = self._out = self._info = self._host_out = None
        return self._result


def _run(fn: str, plane, palette, capacity, stream, as_file: bool):
    h, w, bpp = _plane(fn, plane)
    palette = _palette(fn, palette, bpp)
    if capacity is not None:
        capacity = int(capacity)
        if capacity < 0:
            raise DevaHipError(f'{fn}: capacity must not be negative (got {capacity})')
    p = plan(h, w, bpp)
    device = plane.device
    with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
        scratch = torch.empty(p.scratch_bytes, dtype=torch.uint8, device=device)
        info = torch.empty(4, dtype=torch.int64, device=device)
        room = p.worst_case if capacity is None else capacity
        out = torch.empty(max(room, 1), dtype=torch.uint8, device=device)
        _launch_deflate(plane, h, w, bpp, scratch, out, room, info)
        if capacity is None:   # one wait, for info; then exactly the stream
            total = int(info.cpu()[0])
            data = out[:total].cpu().numpy().tobytes()
            return file_bytes(data, h, w, bpp, palette) if as_file else data
        host_out, host_info = to_pinned(out[:room]), to_pinned(info)
        event = record_event(device)
    return PendingPng((h, w, bpp), palette, as_file, scratch, out, info, room, host_out, host_info, event)


def deflate(plane: torch.Tensor, *, capacity: Optional[int] = None, stream=None):
    """uint8 [H,W] or [H,W,3] on the device, contiguous, at any alignment -> the zlib stream of its `Up`-filtered rows
    (rules Z1-Z8) as bytes; `zlib.decompress` gives the row strings back.  `capacity`, `stream`: as `encode`."""
    return _run('deflate', plane, None, capacity, stream, False)


def encode(plane: torch.Tensor, *, palette=None, capacity: Optional[int] = None, stream=None):
    """uint8 [H,W] (gray, or indices into `palette`: bytes or a flat sequence, whole RGB triples, 768 bytes at most) or
    uint8 [H,W,3] on the device -> the bytes of a complete PNG file.  Three launches on the current stream (or on
    `stream`, a torch.cuda.Stream); the chunks and their CRCs are made on the host from the copied stream.

    `capacity=None`: the stream is coded into a buffer of the plan's worst case on the device, ONE wait for `info`, then
    a copy of exactly the stream.  `capacity=` bytes: nothing synchronises; `info` and the first `capacity` bytes are on
    their way to pinned memory and a `PendingPng` is returned, whose `finish()` waits and, should the stream be longer,
    places it again at its exact size and copies that."""
    return _run('encode', plane, palette, capacity, stream, True)
