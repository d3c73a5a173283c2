"""ctypes binding of libdeva_rle_text.so (C ABI declared in include/deva_rle_text.h): the text of COCO run-length masks
(the COCO API's rleToString / rleFrString) coded and parsed on the device (rules C1-C8 of the header).

`encode_text` turns what the run-length encoder leaves on the device (`n`, `base`, `bounds`: `mask_runs.count` / `write` or
`ops.mask_rle`) into the masks' compressed strings, byte for byte what `frame_results.coco_strings` gives on the host;
`parse_text` turns compressed strings into the run array of `deva_rle.h` on the device, word for word what
`rle.run_array(rle.parse_checked(...))` gives.  Both stand behind opt-in parameters of the public functions:
`rle.encode(..., text='device')`, `rle.decode(..., parse='device')`, `rle.intersections`, `rle.iou`, `rle.records`.

A ninth library next to libdeva_hip.so, the three scorers, the regions and the three run-length libraries, loaded lazily
by `lib()`; the conventions are those of `deva.hip.mask_runs`: `check` raises `DevaHipError` with the library's text, there
is no CPU path."""
import ctypes
import os
from ctypes import POINTER, Structure, c_char_p, c_int, c_int32, c_int64, c_uint32, c_void_p
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import DevaHipError, _native
from ._pending import record_event, require_on_device, to_pinned
from .ops import _stream

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'rle_text_lib', 'libdeva_rle_text.so')   # (csrc/Makefile says why it has a directory of its own)
ABI_VERSION = 1

MAX_MASKS = 65536
MAX_WORDS = 1 << 26
MAX_CHARS = 12
SCAN_CHUNK = 1024
MASK_CHUNK = 256
MASK_SCRATCH_BYTES = 8
FLAG_CHAR, FLAG_OPEN, FLAG_LONG, FLAG_COUNT, FLAG_SUM = 1, 2, 4, 8, 16
FLAGS = {FLAG_CHAR: "a character outside '0'..'o'", FLAG_OPEN: 'a text that ends inside a value',
         FLAG_LONG: f'a value of more than {MAX_CHARS} characters', FLAG_COUNT: 'a count below 0 or above H * W',
         FLAG_SUM: 'counts that do not sum to H * W'}


class Limits(Structure):
    """mirror of `struct deva_text_limits` (include/deva_rle_text.h)"""
    _fields_ = [('max_masks', c_int32), ('max_words', c_int32), ('max_chars', c_int32), ('block', c_int32), ('scan_chunk', c_int32),
                ('mask_chunk', c_int32)]


class Plan(Structure):
    """mirror of `struct deva_text_plan`"""
    _fields_ = [('mask_grid', c_uint32), ('scan_grid', c_uint32), ('mask_chunks', c_int32), ('items', c_int32), ('value_chars', c_int32),
                ('reserved', c_int32), ('min_words', c_int64), ('parse_scratch_bytes', c_int64)]


# name -> (restype, argtypes); must list every symbol of include/deva_rle_text.h
SIGNATURES = {
    'deva_text_version': (c_int, []),
    'deva_text_last_error': (c_char_p, []),
    'deva_text_limits': (c_int, [POINTER(Limits)]),
    'deva_text_plan': (c_int, [c_int, c_int, c_int, c_int64, POINTER(Plan)]),
    'deva_text_max_chars': (c_int, [c_int64]),
    'deva_text_parse_scratch': (c_int64, [c_int]),
    'deva_text_encode_count': (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                       c_void_p]),
    'deva_text_encode_write': (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_int, c_void_p, c_void_p, c_int64, c_void_p]),
    'deva_text_parse': (c_int, [c_void_p, c_int64, c_void_p, c_int, c_int, c_int, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p]),
}

_LIB = None


def lib() -> ctypes.CDLL:
    """Load (once) and return the text codec's library; raises if it has not been built."""
    return _LIB or _native.load(globals(), 'deva_text_version', 'libdeva_rle_text.so', 'the run-length text codec')


def check(code: int, what: str) -> None:
    if code != 0:
        _native.check(globals(), code, what, 'deva_text_last_error')


class LimitInfo(NamedTuple):
    max_masks: int    # masks of one call of the library; `encode_text` and `parse_text` walk more in chunks
    max_words: int    # words of the run array of one parse: at least 2 n + 1 + characters
    max_chars: int    # characters of one coded value
    block: int
    scan_chunk: int   # counts or characters of one step of the per-mask walk
    mask_chunk: int   # masks of one step of the cross-mask scan


class PlanInfo(NamedTuple):
    mask_grid: int
    scan_grid: int
    mask_chunks: int
    items: int
    value_chars: int
    reserved: int
    min_words: int
    parse_scratch_bytes: int


def text_limits() -> LimitInfo:
    """what one call of the library takes; host only"""
    limits = Limits()
    check(lib().deva_text_limits(ctypes.byref(limits)), 'deva_text_limits')
    return LimitInfo(*(int(getattr(limits, f[0])) for f in Limits._fields_))


def text_plan(n: int, size: Tuple[int, int], chars: int = 0) -> PlanInfo:
    """the launches of both directions for `n` masks of `size` and `chars` characters of text; host only: no device is touched"""
    plan = Plan()
    check(lib().deva_text_plan(int(n), int(size[0]), int(size[1]), int(chars), ctypes.byref(plan)), 'deva_text_plan')
    return PlanInfo(*(int(getattr(plan, f[0])) for f in Plan._fields_))


def max_chars(total: int) -> int:
    """the widest a coded value can be when every count is within [0, total] (C4): 5 at 1080p, 7 at most; -1 outside 1 .. 2^31 - 1"""
    return int(lib().deva_text_max_chars(int(total)))


def parse_scratch(n: int) -> int:
    """bytes of scratch of one parse of n masks; -1 beyond the limits"""
    return int(lib().deva_text_parse_scratch(int(n)))


# ------------------------------------------------------------------------------------------ the three calls of the library
def _launch_encode_count(n, base, bounds, bounds_len, h, w, text_len, text_base, text_total, first) -> None:
    """deva_text_encode_count on the current stream of the inputs' device (the tests' CPU contract replaces the three `_launch_*`)"""
    fn = 'encode_count'
    for name, t in (('n', n), ('base', base), ('bounds', bounds), ('text_len', text_len), ('text_base', text_base), ('text_total', text_total),
                    ('first', first)):
        if t is not None:
            require_on_device(t, name, fn)
    with torch.cuda.device(n.device):
        check(lib().deva_text_encode_count(n.data_ptr(), base.data_ptr(), bounds.data_ptr() if bounds_len else None, bounds_len, n.numel(), h, w,
                                           text_len.data_ptr(), text_base.data_ptr(), text_total.data_ptr(),
                                           None if first is None else first.data_ptr(), _stream(n.device)), 'deva_text_encode_count')


def _launch_encode_write(n, base, bounds, bounds_len, h, w, text_base, chars, capacity) -> None:
    fn = 'encode_write'
    for name, t in (('n', n), ('base', base), ('bounds', bounds), ('text_base', text_base), ('chars', chars)):
        require_on_device(t, name, fn)
    with torch.cuda.device(n.device):
        check(lib().deva_text_encode_write(n.data_ptr(), base.data_ptr(), bounds.data_ptr() if bounds_len else None, bounds_len, n.numel(), h, w,
                                           text_base.data_ptr(), chars.data_ptr() if capacity else None, capacity, _stream(n.device)),
              'deva_text_encode_write')


def _launch_parse(chars, chars_len, text_first, n, h, w, scratch, runs, words_cap, info) -> None:
    fn = 'parse'
    for name, t in (('chars', chars), ('text_first', text_first), ('scratch', scratch), ('runs', runs), ('info', info)):
        require_on_device(t, name, fn)
    with torch.cuda.device(runs.device):
        check(lib().deva_text_parse(chars.data_ptr() if chars_len else None, chars_len, text_first.data_ptr(), n, h, w,
                                    scratch.data_ptr() if n else None, scratch.numel() * 4, runs.data_ptr(), words_cap, info.data_ptr(),
                                    _stream(runs.device)), 'deva_text_parse')


def _size(size, fn: str) -> Tuple[int, int]:
    h, w = int(size[0]), int(size[1])
    if h < 1 or w < 1 or h * w >= 2**31:
        raise DevaHipError(f'{fn}: bad height x width {h} x {w} (1 <= H * W < 2^31)')
    return h, w


# ------------------------------------------------------------------------------------------ encode
def _encoder_inputs(n, base, bounds, fn: str) -> int:
    for name, t, dtype in (('n', n, torch.int32), ('base', base, torch.int64), ('bounds', bounds, torch.int32)):
        if not isinstance(t, torch.Tensor) or t.dtype != dtype or t.dim() != 1 or not t.is_contiguous():
            raise DevaHipError(f'{fn}: `{name}` must be a contiguous {dtype} vector on the device')
    if base.numel() != n.numel():
        raise DevaHipError(f'{fn}: `base` has {base.numel()} entries for {n.numel()} masks')
    return int(n.numel())


class PendingText:
    """the texts of one `encode_text(..., pending=True)` on their way to the host; `finish()` waits for them"""

    def __init__(self, chars, text_len, text_total, capacity, event):
        self.capacity = capacity
        self._chars, self._len, self._total, self._event, self._result = chars, text_len, text_total, event, None

    def finish(self) -> List[bytes]:
        """-> the compressed string of every mask as bytes, in mask order"""
        if self._result is None:
            if self._event is not None:
                self._event.synchronize()
            total = int(self._total[-1]) if self._total is not None else 0
            if total > self.capacity:
                raise DevaHipError(f'encode_text: the texts have {total} characters, the capacity is {self.capacity}')
            lengths = self._len.numpy().astype(np.int64)
            ends = np.cumsum(lengths)
            text = self._chars.numpy()[:total].tobytes()
            self._result = [text[e - m:e] for e, m in zip(ends.tolist(), lengths.tolist())]
            self._chars = None
        return self._result


def encode_text(n: torch.Tensor, base: torch.Tensor, bounds: torch.Tensor, size: Tuple[int, int], *, capacity: Optional[int] = None,
                pending: bool = False, record: bool = True, max_masks: Optional[int] = None):
    """the run boundaries of N masks of `size` on the device (C3: `n` int32 [N], `base` int64 [N], `bounds` int32, as
    `mask_runs.count` / `write` or `ops.mask_rle` leave them) -> the compressed string of every mask as `bytes`, equal to
    `frame_results.coco_strings` of their counts.

    `capacity`: the characters `chars` holds; the default, `max_chars(H * W) * (bounds.numel() + N)`, is enough for any
    boundaries (a mask has n[k] + 1 counts), so nothing is waited for to size it.  The two launches per call of the
    library, then ONE copy of `chars`, `text_len` and `text_total` to pinned host memory; with `pending=True` a
    `PendingText` is returned and nothing synchronises (`record=False`: no event of its own either, the caller's covers
    the copies).  More masks than one call takes (`text_limits()`; `max_masks` lowers it) are walked in chunks that fill
    one `chars`."""
    fn = 'encode_text'
    count = _encoder_inputs(n, base, bounds, fn)
    h, w = _size(size, fn)
    top = text_limits().max_masks
    step = top if max_masks is None else int(max_masks)
    if not 1 <= step <= top:
        raise DevaHipError(f'{fn}: limit of 1 to {top} masks (got {step})')
    widest = max_chars(h * w)
    room = widest * (bounds.numel() + count) if capacity is None else int(capacity)
    if room < 0:
        raise DevaHipError(f'{fn}: capacity must not be negative (got {capacity})')
    device = n.device
    if count == 0:
        none = torch.zeros(0, dtype=torch.int32)
        result = PendingText(torch.zeros(0, dtype=torch.uint8), none, None, room, None)
        return result if pending else result.finish()
    parts = [(lo, min(lo + step, count)) for lo in range(0, count, step)]
    text_len = torch.empty(count, dtype=torch.int32, device=device)
    text_base = torch.empty(count, dtype=torch.int64, device=device)
    totals = torch.zeros(len(parts) + 1, dtype=torch.int64, device=device)
    chars = torch.empty(room, dtype=torch.uint8, device=device)
    for c, (lo, hi) in enumerate(parts):
        _launch_encode_count(n[lo:hi], base[lo:hi], bounds, bounds.numel(), h, w, text_len[lo:hi], text_base[lo:hi], totals[c + 1:c + 2],
                             totals[c:c + 1])
    for lo, hi in parts:
        _launch_encode_write(n[lo:hi], base[lo:hi], bounds, bounds.numel(), h, w, text_base[lo:hi], chars, room)
    host = [to_pinned(t) for t in (chars, text_len, totals)]
    result = PendingText(host[0], host[1], host[2], room, record_event(device) if record else None)
    return result if pending else result.finish()


# ------------------------------------------------------------------------------------------ parse
class RunChunk(NamedTuple):
    """the run array (include/deva_rle.h) of the masks lo .. hi - 1 of a call"""
    lo: int
    hi: int
    device: torch.Tensor    # int32 on the device: the words of the run array come first, room behind them (`spare` words at least)
    host: np.ndarray        # int32 [words]: the run array on the host
    words: int


def text_chunks(lengths: Sequence[int], max_masks: int, max_words: int) -> Optional[List[Tuple[int, int]]]:
    """[lo, hi) ranges of masks, each within one parse's limits: hi - lo <= max_masks and 2 n + 1 + characters <=
    max_words.  None when one mask's text alone is above them."""
    out, lo, words = [], 0, 1
    for k, m in enumerate(lengths):
        if 3 + m > max_words:
            return None
        if k > lo and (k - lo >= max_masks or words + m + 2 > max_words):
            out.append((lo, k))
            lo, words = k, 1
        words += m + 2
    if len(lengths) > lo:
        out.append((lo, len(lengths)))
    return out


class PendingParse:
    """the parses of one `parse_text(..., pending=True)`: launched, `info` on its way to the host"""

    def __init__(self, texts, size, device, parts, spare):
        self.texts, self.size, self.device = texts, size, torch.device(device)
        h, w = size
        pin = self.device.type == 'cuda'
        self._chunks = []
        for lo, hi in parts:
            n = hi - lo
            lengths = np.fromiter((len(t) for t in texts[lo:hi]), dtype=np.int64, count=n)
            total = int(lengths.sum())
            # one upload: text_first as int64 [n + 1], then the characters
            up = torch.empty(8 * (n + 1) + total, dtype=torch.uint8, pin_memory=pin)
            first = up[:8 * (n + 1)].view(torch.int64).numpy()
            first[0] = 0
            np.cumsum(lengths, out=first[1:])
            up.numpy()[8 * (n + 1):] = np.frombuffer(b''.join(texts[lo:hi]), dtype=np.uint8)
            up_d = up.to(self.device, non_blocking=True)
            words_cap = 2 * n + 1 + total
            runs = torch.empty(words_cap + spare * n, dtype=torch.int32, device=self.device)
            scratch = torch.empty(max(2 * n, 1), dtype=torch.int32, device=self.device)
            info = torch.empty(2, dtype=torch.int64, device=self.device)
            _launch_parse(up_d[8 * (n + 1):], total, up_d[:8 * (n + 1)].view(torch.int64), n, h, w, scratch, runs, words_cap, info)
            self._chunks.append((lo, hi, runs, to_pinned(info), up))
        self._event = record_event(self.device)
        self._result = None

    def flags(self) -> int:
        """the first wait: the flag bits of C7 of all chunks, or-ed"""
        if self._event is not None:
            self._event.synchronize()
            self._event = None
        out = 0
        for _, _, _, info, _ in self._chunks:
            out |= int(info[0])
        return out

    def fetch(self) -> None:
        """after `flags()` gave 0: start the copies of the words that `info` counts (the caller waits for them: `complete`)"""
        self._hosts = [to_pinned(runs[:int(info[1])]) for _, _, runs, info, _ in self._chunks]

    def complete(self) -> List[RunChunk]:
        """after `fetch()` and a wait for its copies"""
        if self._result is not None:
            return self._result
        self._result = [RunChunk(lo, hi, runs, host.numpy(), int(info[1])) for (lo, hi, runs, info, _), host in zip(self._chunks, self._hosts)]
        self._chunks = self._hosts = None
        return self._result

    def finish(self, on_flags=None) -> List[RunChunk]:
        """-> the chunks' run arrays, on the device and on the host: two waits, for `info` and for the words it counts.
        A flag of C7 raises `DevaHipError` (after `on_flags(flags)`, if given, had its chance to raise a better one)."""
        if self._result is None:
            flags = self.flags()
            if flags:
                if on_flags is not None:
                    on_flags(flags)
                raise DevaHipError('parse_text: ' + '; '.join(text for bit, text in FLAGS.items() if flags & bit))
            self.fetch()
            event = record_event(self.device)
            if event is not None:
                event.synchronize()
            self.complete()
        return self._result


def parse_text(texts: Sequence[bytes], size: Tuple[int, int], *, device=None, pending: bool = False, spare: int = 0,
               max_masks: Optional[int] = None, max_words: Optional[int] = None):
    """the compressed strings of N masks of `size` (`bytes` each) -> [RunChunk]: their run array (include/deva_rle.h) built
    on the device, and its host copy; word for word `rle.run_array(rle.parse_checked(texts, size), lo, hi)`.

    The joined bytes of a chunk go up once, three launches follow, and `info` and the words it counts come back in two
    waits (`pending=True`: a `PendingParse`, nothing has synchronised; `finish()` has both).  A text that breaks C7 raises
    `DevaHipError`.  `spare`: int32 words per mask kept free behind every chunk's run array on the device (the overlap
    keeps its boxes there).  More masks or characters than one parse takes (`text_limits()`; `max_masks` / `max_words`
    lower the limits) are walked in chunks; a single text above them is an error."""
    fn = 'parse_text'
    h, w = _size(size, fn)
    if isinstance(texts, (bytes, str)) or not all(isinstance(t, (bytes, bytearray)) for t in texts):
        raise DevaHipError(f'{fn}: a list of bytes expected')
    top = text_limits()
    max_masks = top.max_masks if max_masks is None else int(max_masks)
    max_words = top.max_words if max_words is None else int(max_words)
    if not (1 <= max_masks <= top.max_masks and 4 <= max_words <= top.max_words):
        raise DevaHipError(f'{fn}: limits of 1 to {top.max_masks} masks and 4 to {top.max_words} words (got {max_masks}, {max_words})')
    parts = text_chunks([len(t) for t in texts], max_masks, max_words)
    if parts is None:
        raise DevaHipError(f'{fn}: one text alone is above the limit of one call ({max_words} words)')
    result = PendingParse(list(texts), (h, w), 'cuda' if device is None else device, parts, int(spare))
    return result if pending else result.finish()
