"""ctypes binding of libdeva_jpeg.so (C ABI declared in include/deva_jpeg.h): the overlay JPEG of the `demo` saver from
entropy-coded data that the device codes from an RGB plane (rules J1-J10 of the header).

`scan` gives the entropy-coded data of a plane with its restart markers (colour conversion, 4:2:0 or 4:4:4, integer DCT,
libjpeg's quality scaling of the Annex K tables, the Annex K Huffman tables, one restart interval per MCU row unless
`restart` says otherwise), `encode` a complete baseline JFIF file around it.  The file's markers -- SOI, APP0, DQT, SOF0,
DHT, DRI, SOS, EOI -- are written on the HOST (`file_bytes`); only the data comes from the device.

A twelfth library next to libdeva_hip.so, loaded lazily by `lib()`; the conventions are those of `deva.hip.png`: `check`
raises `DevaHipError` with the library's text, there is no CPU path, every launch goes on torch's current stream (or on
`stream=`)."""
import contextlib
import ctypes
import os
from ctypes import POINTER, Structure, c_char_p, c_int, c_int32, c_int64, c_void_p
from typing import NamedTuple, Optional, Tuple

import torch

from . import DevaHipError, _native
from ._pending import record_event, require_on_device, to_pinned
from .ops import _stream

__all__ = ['encode', 'scan', 'plan', 'limits', 'quant_tables', 'file_bytes', 'PendingJpeg', 'PlanInfo', 'LimitInfo', 'MAX_SIDE', 'MAX_BYTES',
           'MAX_RESTART', 'SUBSAMPLINGS']

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'jpeg_lib', 'libdeva_jpeg.so')   # (csrc/Makefile says why it has a directory of its own)
ABI_VERSION = 1

MAX_SIDE = 16384
MAX_BYTES = 1 << 29
MAX_RESTART = 65535
SUBSAMPLINGS = {'4:2:0': 420, '4:4:4': 444}

# ITU-T T.81, Annex K.3: the "typical" Huffman tables as a DHT holds them (the counts of the code lengths 1 .. 16, the symbols)
_DC = (bytes([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]), bytes([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0]))
_AC_COUNTS = (bytes([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d]), bytes([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77]))
_AC_SYMBOLS = (bytes.fromhex(
    '01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a'
    '434445464748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9'
    'aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa'), bytes.fromhex(
    '000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a3536373839'
    '3a434445464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7'
    'a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa'))


class Limits(Structure):
    """mirror of `struct deva_jpeg_limits` (include/deva_jpeg.h)"""
    _fields_ = [('max_side', c_int32), ('max_bytes', c_int32), ('max_restart', c_int32), ('block_bits', c_int32), ('block', c_int32),
                ('lds_bytes', c_int32)]


class Plan(Structure):
    """mirror of `struct deva_jpeg_plan`"""
    _fields_ = [('mcu', c_int32), ('mcus_x', c_int32), ('mcus_y', c_int32), ('blocks_per_mcu', c_int32), ('restart', c_int32),
                ('intervals', c_int32), ('blocks', c_int32), ('block', c_int32), ('coef_bytes', c_int64), ('slot_bytes', c_int64),
                ('scratch_bytes', c_int64), ('worst_case', c_int64)]


# name -> (restype, argtypes); must list every symbol of include/deva_jpeg.h
SIGNATURES = {
    'deva_jpeg_version': (c_int, []),
    'deva_jpeg_last_error': (c_char_p, []),
    'deva_jpeg_limits': (c_int, [POINTER(Limits)]),
    'deva_jpeg_plan': (c_int, [c_int, c_int, c_int, c_int, POINTER(Plan)]),
    'deva_jpeg_quant': (c_int, [c_int, c_void_p]),
    'deva_jpeg_scan': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p]),
    'deva_jpeg_place': (c_int, [c_int, c_int, c_int, c_int, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p]),
}

_LIB = None


def lib() -> ctypes.CDLL:
    """Load (once) and return the library; raises if it has not been built."""
    return _LIB or _native.load(globals(), 'deva_jpeg_version', 'libdeva_jpeg.so', 'the JPEG coder kernels')


def check(code: int, what: str) -> None:
    if code != 0:
        _native.check(globals(), code, what, 'deva_jpeg_last_error')


class LimitInfo(NamedTuple):
    max_side: int            # H and W at most
    max_bytes: int           # H * W * 3 at most
    max_restart: int         # MCUs of an interval at most
    block_bits: int          # the longest coded block
    block: int               # lanes of a workgroup = blocks of a step
    lds_bytes: int


class PlanInfo(NamedTuple):
    mcu: int                 # 16 ('4:2:0') or 8 ('4:4:4')
    mcus_x: int
    mcus_y: int
    blocks_per_mcu: int      # 6 or 3
    restart: int             # MCUs of an interval, as DRI holds it
    intervals: int
    blocks: int
    block: int
    coef_bytes: int          # the int16 coefficients in the scratch
    slot_bytes: int          # an interval's slot in the scratch
    scratch_bytes: int       # the scratch of one call
    worst_case: int          # a capacity no plane of this size exceeds


def limits() -> LimitInfo:
    """what the library takes; host only"""
    out = Limits()
    check(lib().deva_jpeg_limits(ctypes.byref(out)), 'deva_jpeg_limits')
    return LimitInfo(*(int(getattr(out, f[0])) for f in Limits._fields_))


def _parameters(fn: str, height, width, quality, subsampling, restart) -> Tuple[int, int, int, int, int]:
    """rules J1, J5 and J8 on the sizes and the three parameters, as the library checks them (raised here with the wrapper's
    name, before anything is allocated) -> (h, w, quality, the library's subsampling code, restart)"""
    try:
        h, w, q, r = int(height), int(width), int(quality), int(restart)
    except (TypeError, ValueError):
        raise DevaHipError(f'{fn}: height, width, quality and restart are integers (got {height!r}, {width!r}, {quality!r}, {restart!r})') from None
    if not isinstance(subsampling, str) or subsampling not in SUBSAMPLINGS:
        raise DevaHipError(f"{fn}: subsampling: '4:2:0' or '4:4:4' (got {subsampling!r})")
    if not (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE):
        raise DevaHipError(f'{fn}: bad height x width {h} x {w} (1 to {MAX_SIDE} each)')
    if h * w * 3 > MAX_BYTES:
        raise DevaHipError(f'{fn}: a plane of {h} x {w} x 3 bytes, a call takes {MAX_BYTES}')
    if not 1 <= q <= 100:
        raise DevaHipError(f'{fn}: quality: 1 to 100 (got {q})')
    if not 0 <= r <= MAX_RESTART:
        raise DevaHipError(f'{fn}: restart: 0 (one MCU row) to {MAX_RESTART} MCUs (got {r})')
    return h, w, q, SUBSAMPLINGS[subsampling], r


def plan(height: int, width: int, subsampling: str = '4:2:0', restart: int = 0) -> PlanInfo:
    """the MCU and interval geometry, the scratch bytes and the worst-case capacity for a plane; host only: no device is touched"""
    h, w, _, sub, r = _parameters('plan', height, width, 75, subsampling, restart)
    out = Plan()
    check(lib().deva_jpeg_plan(h, w, sub, r, ctypes.byref(out)), 'deva_jpeg_plan')
    return PlanInfo(*(int(getattr(out, f[0])) for f in Plan._fields_))


def quant_tables(quality: int = 75) -> Tuple[bytes, bytes]:
    """J5: (luminance, chrominance), 64 bytes each in zigzag order, as the DQT of the file holds them; host only"""
    q = _parameters('quant_tables', 1, 1, quality, '4:2:0', 0)[2]
    out = (ctypes.c_uint8 * 128)()
    check(lib().deva_jpeg_quant(q, out), 'deva_jpeg_quant')
    return bytes(out[:64]), bytes(out[64:])


# ------------------------------------------------------------------------------------------ the two calls of the library
def _launch_scan(plane, h, w, quality, sub, restart, scratch, out, capacity, info) -> None:
    """deva_jpeg_scan on the current stream of the plane's device (the tests' CPU contract replaces the two `_launch_*`)"""
    fn = 'scan'
    for name, t in (('plane', plane), ('scratch', scratch), ('out', out), ('info', info)):
        require_on_device(t, name, fn)
    with torch.cuda.device(plane.device):
        check(lib().deva_jpeg_scan(plane.data_ptr(), h, w, quality, sub, restart, scratch.data_ptr(), scratch.numel(),
                                   out.data_ptr() if capacity else None, capacity, info.data_ptr(), _stream(plane.device)), 'deva_jpeg_scan')


def _launch_place(h, w, sub, restart, scratch, out, capacity, info) -> None:
    fn = 'scan'
    for name, t in (('scratch', scratch), ('out', out), ('info', info)):
        require_on_device(t, name, fn)
    with torch.cuda.device(scratch.device):
        check(lib().deva_jpeg_place(h, w, sub, restart, scratch.data_ptr(), scratch.numel(), out.data_ptr() if capacity else None, capacity,
                                    info.data_ptr(), _stream(scratch.device)), 'deva_jpeg_place')


# ------------------------------------------------------------------------------------------ the file around the data (host)
def _segment(marker: int, payload: bytes) -> bytes:
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, 'big') + payload


def file_bytes(scan: bytes, height: int, width: int, *, quality: int = 75, subsampling: str = '4:2:0', restart: int = 0) -> bytes:
    """entropy-coded data (rules J1-J9) -> the baseline JFIF file (J10): SOI, APP0 (JFIF 1.01, no density), the two DQT,
    SOF0 (three components, Y sampled 2 x 2 or 1 x 1), the four DHT, DRI, SOS, the data, EOI.  Host only."""
    h, w, q, sub, r = _parameters('file_bytes', height, width, quality, subsampling, restart)
    every = r if r else -(-w // (16 if sub == 420 else 8))
    lum, chrom = quant_tables(q)
    parts = [b'\xff\xd8', _segment(0xE0, b'JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00'),
             _segment(0xDB, b'\x00' + lum), _segment(0xDB, b'\x01' + chrom),
             _segment(0xC0, bytes([8]) + h.to_bytes(2, 'big') + w.to_bytes(2, 'big')
                      + bytes([3, 1, 0x22 if sub == 420 else 0x11, 0, 2, 0x11, 1, 3, 0x11, 1])),
             _segment(0xC4, b'\x00' + _DC[0] + bytes(range(12))), _segment(0xC4, b'\x10' + _AC_COUNTS[0] + _AC_SYMBOLS[0]),
             _segment(0xC4, b'\x01' + _DC[1] + bytes(range(12))), _segment(0xC4, b'\x11' + _AC_COUNTS[1] + _AC_SYMBOLS[1]),
             _segment(0xDD, every.to_bytes(2, 'big')),
             _segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])),
             bytes(scan), b'\xff\xd9']
    return b''.join(parts)


def _plane(fn: str, plane, quality, subsampling, restart) -> Tuple[int, int, int, int, int]:
    if not isinstance(plane, torch.Tensor):
        raise DevaHipError(f'{fn}: the plane is a uint8 tensor [H,W,3] on the HIP device (got {type(plane).__name__})')
    if plane.dtype != torch.uint8:
        raise DevaHipError(f'{fn}: plane must be {torch.uint8} (got {plane.dtype})')
    if not (plane.dim() == 3 and plane.shape[2] == 3):
        raise DevaHipError(f'{fn}: [H,W,3] expected (got {tuple(plane.shape)})')
    if not plane.is_contiguous():
        raise DevaHipError(f'{fn}: plane must be contiguous')
    return _parameters(fn, plane.shape[0], plane.shape[1], quality, subsampling, restart)


class PendingJpeg:
    """one `encode` / `scan` with `capacity=`: the kernels and the copies of `info` and of the first `capacity` bytes of
    the data are in flight on the caller's stream; `finish()` waits for them.  The coded intervals stay in the scratch on
    the device until then, so data above `capacity` is placed again at its exact size and copied: never truncated."""

    def __init__(self, geometry, parameters, as_file, scratch, out, info, capacity, host_out, host_info, event):
        self.geometry, self.parameters, self.capacity = geometry, parameters, capacity
        self._as_file = as_file
        self._scratch, self._out, self._info, self._host_out, self._host_info, self._event = scratch, out, info, host_out, host_info, event
        self._result = None
        self.total = self.blocks = self.intervals = None
        self.overflowed = None

    def finish(self) -> bytes:
        if self._result is None:
            if self._event is not None:
                self._event.synchronize()
            total, blocks, over, intervals = (int(v) for v in self._host_info.tolist())
            self.total, self.blocks, self.overflowed, self.intervals = total, blocks, bool(over), intervals
            (h, w), (quality, subsampling, restart) = self.geometry, self.parameters
            if over:   # (rare: the saver's capacity is twice the largest data seen so far)
                device = self._scratch.device
                with torch.cuda.device(device) if device.type == 'cuda' else contextlib.nullcontext():
                    out = torch.empty(total, dtype=torch.uint8, device=device)
                    _launch_place(h, w, SUBSAMPLINGS[subsampling], restart, self._scratch, out, total, self._info)
                    data = out.cpu().numpy().tobytes()
            else:
                data = self._host_out.numpy()[:total].tobytes()
            self._result = file_bytes(data, h, w, quality=quality, subsampling=subsampling, restart=restart) if self._as_file else data
            self._scratch = self._out = self._info = self._host_out = None
        return self._result


def _run(fn: str, plane, quality, subsampling, restart, capacity, stream, as_file: bool):
    h, w, q, sub, r = _plane(fn, plane, quality, subsampling, restart)
    if capacity is not None:
        capacity = int(capacity)
        if capacity < 0:
            raise DevaHipError(f'{fn}: capacity must not be negative (got {capacity})')
    p = plan(h, w, subsampling, r)
    device = plane.device
    with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
        scratch = torch.empty(p.scratch_bytes, dtype=torch.uint8, device=device)
        info = torch.empty(4, dtype=torch.int64, device=device)
        room = p.worst_case if capacity is None else capacity
        out = torch.empty(max(room, 1), dtype=torch.uint8, device=device)
        _launch_scan(plane, h, w, q, sub, r, scratch, out, room, info)
        if capacity is None:   # one wait, for info; then exactly the data
            total = int(info.cpu()[0])
            data = out[:total].cpu().numpy().tobytes()
            return file_bytes(data, h, w, quality=q, subsampling=subsampling, restart=r) if as_file else data
        host_out, host_info = to_pinned(out[:room]), to_pinned(info)
        event = record_event(device)
    return PendingJpeg((h, w), (q, subsampling, r), as_file, scratch, out, info, room, host_out, host_info, event)


def scan(plane: torch.Tensor, *, quality: int = 75, subsampling: str = '4:2:0', restart: int = 0, capacity: Optional[int] = None, stream=None):
    """uint8 [H,W,3] RGB on the device, contiguous, at any alignment -> the entropy-coded data of its baseline JPEG with
    the restart markers (rules J1-J9) as bytes.  `capacity`, `stream`: as `encode`."""
    return _run('scan', plane, quality, subsampling, restart, capacity, stream, False)


def encode(plane: torch.Tensor, *, quality: int = 75, subsampling: str = '4:2:0', restart: int = 0, capacity: Optional[int] = None, stream=None):
    """uint8 [H,W,3] RGB on the device -> the bytes of a complete baseline JFIF file.  `quality` 1 .. 100 scales the Annex K
    tables as libjpeg does, `subsampling` is '4:2:0' or '4:4:4', `restart` the MCUs of a restart interval (0: one MCU
    row).  Four launches on the current stream (or on `stream`, a torch.cuda.Stream); the markers are made on the host.

    `capacity=None`: the data is coded into a buffer of the plan's worst case on the device, ONE wait for `info`, then a
    copy of exactly the data.  `capacity=` bytes: nothing synchronises; `info` and the first `capacity` bytes are on their
    way to pinned memory and a `PendingJpeg` is returned, whose `finish()` waits and, should the data be longer, places
    it again at its exact size and copies that."""
    return _run('encode', plane, quality, subsampling, restart, capacity, stream, True)
