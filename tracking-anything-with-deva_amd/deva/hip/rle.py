"""ctypes binding of libdeva_rle.so (C ABI declared in include/deva_rle.h): COCO run-length masks, as a detector's
"COCO results" file, a referring pipeline's proposals or this project's own BURST output carry them, decoded on the
device into the byte planes that `assemble_*` and `ProposalFilter` take or the float planes of the consensus vote, with
the frame reader's nearest resize fused in (rules D1-D6 of the header).

The host parses the text (`parse_counts`: the inverse of `frame_results.coco_strings`, vectorised over all characters
of all masks of a call), checks the counts (D2), turns them into run starts by one cumulative sum and sends ONE int32
array per call to the device; the kernel does the rest.  `pycocotools` is not needed.  With `parse='device'` (an opt-in
of `decode`, `records`, `intersections` and `iou`) the texts go up as they are and libdeva_rle_text.so builds the run
array there (`deva.hip.rle_text`); the results are the same.

A sixth library next to libdeva_hip.so, the three scorers and the regions, loaded lazily by `lib()`; the conventions are
those of `deva.hip.regions`: `check` raises `DevaHipError` with the library's text, there is no CPU path."""
import ctypes
import os
from ctypes import POINTER, Structure, c_char_p, c_float, c_int, c_int32, c_int64, c_uint32, c_void_p
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import DevaHipError, _native, _planes, rle_text
from .mask_runs import encode, encode_labels  # noqa: F401  (the other direction: planes -> run lengths, libdeva_mask_runs.so)
from .rle_overlap import intersections, iou  # noqa: F401  (mask overlaps from the run lengths, libdeva_rle_overlap.so)
from .ops import _stream

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libdeva_rle.so')
ABI_VERSION = 1

TILE = 64
MAX_MASKS = 65536
MAX_WORDS = 1 << 26
DTYPES = {torch.uint8: 0, torch.float32: 1}   # DEVA_RLE_U8, DEVA_RLE_F32
MAX_CHARS = 12                                 # characters of one coded value: 60 bits
PARSE = ('host', 'device')                     # where the text of a mask is parsed


class Limits(Structure):
    """mirror of `struct deva_rle_limits` (include/deva_rle.h)"""
    _fields_ = [('max_masks', c_int32), ('max_words', c_int32), ('tile', c_int32), ('block', c_int32)]


class Plan(Structure):
    """mirror of `struct deva_rle_plan`"""
    _fields_ = [('tiles_x', c_int32), ('tiles_y', c_int32), ('grid', c_uint32), ('lds_bytes', c_int32), ('scale_y', c_float),
                ('scale_x', c_float), ('out_bytes', c_int64)]


# name -> (restype, argtypes); must list every symbol of include/deva_rle.h
SIGNATURES = {
    'deva_rle_version': (c_int, []),
    'deva_rle_last_error': (c_char_p, []),
    'deva_rle_limits': (c_int, [POINTER(Limits)]),
    'deva_rle_plan': (c_int, [c_int, c_int, c_int, c_int, c_int, c_int, POINTER(Plan)]),
    'deva_rle_check': (c_int, [c_void_p, c_int64, c_int, c_int, c_int]),
    'deva_rle_decode': (c_int, [c_void_p, c_void_p, c_int64, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
}

_LIB = None


def lib() -> ctypes.CDLL:
    """Load (once) and return the run-length library; raises if it has not been built."""
    return _LIB or _native.load(globals(), 'deva_rle_version', 'libdeva_rle.so', 'the run-length decoder')


def check(code: int, what: str) -> None:
    if code != 0:
        _native.check(globals(), code, what, 'deva_rle_last_error')


class LimitInfo(NamedTuple):
    max_masks: int   # masks of one call of the library; `decode` walks more in chunks
    max_words: int   # int32 words of one call's run array: 2 n + 1 + the runs of its n masks
    tile: int        # edge of the output tile a workgroup owns
    block: int


class PlanInfo(NamedTuple):
    tiles_x: int
    tiles_y: int
    grid: int
    lds_bytes: int
    scale_y: float   # D3: H / OH in fp32
    scale_x: float
    out_bytes: int


def rle_limits() -> LimitInfo:
    """what one call of the library takes; host only"""
    limits = Limits()
    check(lib().deva_rle_limits(ctypes.byref(limits)), 'deva_rle_limits')
    return LimitInfo(*(int(getattr(limits, f[0])) for f in Limits._fields_))


def rle_plan(n: int, source_size: Tuple[int, int], size: Optional[Tuple[int, int]] = None, dtype=torch.uint8) -> PlanInfo:
    """the launch `decode` makes for `n` masks of `source_size` decoded at `size`; host only: no device is touched"""
    size = source_size if size is None else size
    plan = Plan()
    check(lib().deva_rle_plan(int(n), int(source_size[0]), int(source_size[1]), int(size[0]), int(size[1]), _dtype_code(dtype, 'rle_plan'),
                              ctypes.byref(plan)), 'deva_rle_plan')
    return PlanInfo(*(getattr(plan, f[0]) for f in Plan._fields_))


def _dtype_code(dtype, fn: str) -> int:
    if dtype not in DTYPES:
        raise DevaHipError(f'{fn}: dtype must be torch.uint8 or torch.float32 (got {dtype})')
    return DTYPES[dtype]


# ------------------------------------------------------------------------------------------ the text
def _segment_cumsum(values: np.ndarray, segment: np.ndarray) -> np.ndarray:
    """cumulative sums that start anew wherever `segment` (ascending ids) changes"""
    if values.size == 0:
        return values
    total = np.cumsum(values)
    new = np.ones(values.size, dtype=bool)
    new[1:] = segment[1:] != segment[:-1]
    return total - (total - values)[new][np.cumsum(new) - 1]


def _restarted_cumsum(values: np.ndarray, restarts: np.ndarray) -> np.ndarray:
    """cumulative sums that start anew at every position of `restarts` (ascending, the first one 0)"""
    total = np.cumsum(values)
    base = total[restarts] - values[restarts]
    return total - np.repeat(base, np.diff(np.append(restarts, values.size)))


def _decode_texts(chars: np.ndarray, lengths: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """the characters of several masks' compressed strings back to back (uint8, `lengths[k]` of them for mask k) ->
    (their counts back to back, int64; how many per mask): the COCO API's rleFrString for all of them at once.  One numpy
    step per character position of a value (as `frame_results.coco_strings` encodes), none per run or character."""
    lengths = np.asarray(lengths, dtype=np.int64)
    if chars.size == 0:
        return np.zeros(0, dtype=np.int64), np.zeros(lengths.size, dtype=np.int64)
    text_ends = np.cumsum(lengths)                       # one past the last character of every text

    def mask_at(k):
        return int(np.searchsorted(text_ends, k, side='right'))
    v = chars - np.uint8(48)                             # (uint8: what lies below '0' wraps to above 63)
    bad = v > 63
    if bad.any():
        k = int(np.argmax(bad))
        raise DevaHipError(f"parse_counts: mask {mask_at(k)}: character {bytes(chars[k:k + 1])!r} is outside '0'..'o'")
    some = np.flatnonzero(lengths > 0)
    open_ = (v[text_ends[some] - 1] & 0x20) != 0         # the last character of a text announces another one
    if open_.any():
        raise DevaHipError(f'parse_counts: mask {int(some[np.argmax(open_)])}: the text ends inside a value')
    finals = np.flatnonzero((v & 0x20) == 0)             # the character that ends a value: one per value, in order
    per_mask = np.diff(np.concatenate([[0], np.searchsorted(finals, text_ends - 1, side='right')])).astype(np.int64)
    begins = np.empty_like(finals)                       # the character that begins a value
    begins[0], begins[1:] = 0, finals[:-1] + 1
    width = finals - begins + 1                          # characters of every value: 5 bits each, low bits first
    if int(width.max()) > MAX_CHARS:
        raise DevaHipError(f'parse_counts: mask {mask_at(int(begins[np.argmax(width > MAX_CHARS)]))}: a value of more than {MAX_CHARS} characters')
    x = (v[begins] & 0x1f).astype(np.int64)
    longer = np.flatnonzero(width > 1)
    for place in range(1, int(width.max())):             # (at most MAX_CHARS - 1 steps, over the values that are this long)
        x[longer] |= (v[begins[longer] + place] & 0x1f).astype(np.int64) << (5 * place)
        longer = longer[width[longer] > place + 1]
    negative = np.flatnonzero((v[finals] & 0x10) != 0)
    x[negative] |= np.int64(-1) << (5 * width[negative])
    # from a mask's fourth count on the value is the difference to the count two places back: count 0 stands alone, the
    # counts 1, 3, 5, ... are the running sums of their values, and so are the counts 2, 4, 6, ...  Values two apart lie
    # two apart in the whole array as well, so each chain is a strided half of it, restarted at a mask's counts 0, 1, 2.
    first = (np.cumsum(per_mask) - per_mask)[:, None] + np.arange(3)[None, :]
    first = first[np.arange(3)[None, :] < per_mask[:, None]]
    counts = np.empty_like(x)
    for parity in (0, 1):
        if x.size > parity:
            counts[parity::2] = _restarted_cumsum(x[parity::2], first[(first & 1) == parity] >> 1)
    return counts, per_mask


def _text(counts, k: int) -> bytes:
    if isinstance(counts, str):
        try:
            return counts.encode('latin-1')
        except UnicodeEncodeError:
            raise DevaHipError(f"parse_counts: mask {k}: a character is outside '0'..'o'") from None
    return bytes(counts)


def _is_text(counts) -> bool:
    return isinstance(counts, (str, bytes, bytearray))


def parse_many(rles: Sequence) -> Tuple[np.ndarray, np.ndarray, List[Optional[Tuple[int, int]]]]:
    """masks in any of the forms `parse_counts` takes -> (their counts back to back, int64; how many per mask; per mask
    the (H, W) of its dict, None for a bare text or list).  One vectorised pass over all characters of all texts."""
    sizes, bodies = [], []
    for k, obj in enumerate(rles):
        if isinstance(obj, dict):
            if 'counts' not in obj or 'size' not in obj or len(obj['size']) != 2:
                raise DevaHipError(f"parse_counts: mask {k}: a dict must hold 'size': [H, W] and 'counts'")
            sizes.append((int(obj['size'][0]), int(obj['size'][1])))
            obj = obj['counts']
        else:
            sizes.append(None)
        bodies.append(obj)
    texts = [(k, _text(b, k)) for k, b in enumerate(bodies) if _is_text(b)]
    per_mask = np.zeros(len(bodies), dtype=np.int64)
    pieces = [None] * len(bodies)
    if texts:
        lengths = np.array([len(t) for _, t in texts], dtype=np.int64)
        chars = np.frombuffer(b''.join(t for _, t in texts), dtype=np.uint8)
        try:
            counts, n = _decode_texts(chars, lengths)
        except DevaHipError as e:                        # (the message counts the texts: name the mask of the call)
            raise DevaHipError(_renumber(str(e), [k for k, _ in texts])) from None
        ends = np.cumsum(n)
        for (k, _), e, m in zip(texts, ends.tolist(), n.tolist()):
            pieces[k], per_mask[k] = counts[e - m:e], m
    for k, b in enumerate(bodies):
        if pieces[k] is None:
            try:
                a = np.asarray(b.cpu() if isinstance(b, torch.Tensor) else b)
                if a.dtype.kind not in 'iu' and not (a.size == 0 or (a.dtype.kind == 'f' and np.array_equal(a, np.floor(a)))):
                    raise ValueError
                pieces[k] = a.astype(np.int64).reshape(-1)
            except (ValueError, TypeError):
                raise DevaHipError(f'parse_counts: mask {k}: counts must be a str, bytes or a list of integers') from None
            per_mask[k] = pieces[k].size
    flat = np.concatenate(pieces) if pieces else np.zeros(0, dtype=np.int64)
    return flat, per_mask, sizes


def _renumber(message: str, order: List[int]) -> str:
    import re
    return re.sub(r'mask (\d+)', lambda m: f'mask {order[int(m.group(1))]}', message, count=1)


def parse_counts(obj) -> np.ndarray:
    """one mask's run lengths as int64 counts, from a compressed `str` / `bytes` (the COCO API's string: 5 bits per
    character, low bits first, 0x20 marks a continuation, sign extension when the last character of a value has 0x10,
    48 added; from the fourth count on the coded value is the difference to the count two places back), an
    uncompressed list of counts, or a dict {'size': [H, W], 'counts': either}.  The inverse of
    `frame_results.coco_strings`.  A character outside '0'..'o' or a text that ends inside a value is an error.  The
    counts are not judged here (D2 is `decode`'s and `records`')."""
    return parse_many([obj])[0]


# ------------------------------------------------------------------------------------------ D2 and the run array
class Parsed(NamedTuple):
    counts: Optional[np.ndarray]   # int64, all masks back to back (None after a parse on the device: `counts_of` has them)
    per_mask: np.ndarray    # int64 [N]: runs of every mask
    height: int
    width: int
    device: Optional[list] = None  # after a parse on the device: its [rle_text.RunChunk], the run arrays there and here


def _parse_mode(parse, fn: str) -> bool:
    if parse not in PARSE:
        raise DevaHipError(f'{fn}: parse must be one of {PARSE} (got {parse!r})')
    return parse == 'device'


def _texts_and_size(rles: Sequence, source_size) -> Optional[Tuple[List[bytes], Tuple[int, int]]]:
    """every mask's text as bytes and the one size of the call, when every mask is a text (a dict's `counts` included) and
    the sizes raise no question; None otherwise: the host path then parses, or says what is wrong"""
    bodies, size = [], None if source_size is None else (int(source_size[0]), int(source_size[1]))
    try:
        for obj in rles:
            if isinstance(obj, dict):
                if 'counts' not in obj or 'size' not in obj or len(obj['size']) != 2:
                    return None
                s = (int(obj['size'][0]), int(obj['size'][1]))
                if size is not None and s != size:
                    return None
                size, obj = s, obj['counts']
            if not _is_text(obj):
                return None
            bodies.append(obj.encode('latin-1') if isinstance(obj, str) else bytes(obj))
    except (TypeError, ValueError, UnicodeEncodeError):
        return None
    if size is None or not bodies or size[0] < 1 or size[1] < 1 or size[0] * size[1] >= 2**31:
        return None
    return bodies, size


class _DeviceParse:
    """a parse that libdeva_rle_text.so has been handed (`_begin_device_parse`): `finish()` -> Parsed.  Several of them
    (the two sides of an overlap) share their second wait: `flags_checked()` on each in turn, `fetch()` on each, one wait,
    `parsed()` on each."""

    def __init__(self, pending, size, verdict):
        self.pending, self.size, self.verdict = pending, size, verdict

    def flags_checked(self) -> None:
        flags = self.pending.flags()
        if flags:
            self.verdict(flags)

    def parsed(self) -> 'Parsed':
        chunks = self.pending.complete()
        per_mask = np.concatenate([np.diff(c.host[:c.hi - c.lo + 1].astype(np.int64)) - 1 for c in chunks])
        return Parsed(None, per_mask, self.size[0], self.size[1], chunks)

    def finish(self) -> 'Parsed':
        self.pending.finish(self.verdict)
        return self.parsed()


def _begin_device_parse(rles: Sequence, source_size, fn: str, device, max_masks, max_words, spare: int) -> Optional[_DeviceParse]:
    """`parse_checked` with the run arrays built by libdeva_rle_text.so, launched and not waited for; None when the call
    takes the host path (a mask that is no text, a size that is missing or differs, a text above one call's limits, no
    mask at all)"""
    found = _texts_and_size(rles, source_size)
    if found is None:
        return None
    bodies, size = found
    top = rle_text.text_limits()
    parts = rle_text.text_chunks([len(b) for b in bodies], min(top.max_masks, max_masks or top.max_masks),
                                 min(top.max_words, max_words or top.max_words))
    if parts is None:
        return None

    def host_verdict(flags):
        parse_checked(rles, source_size, fn)             # raises the message that names the mask
        raise DevaHipError(f'{fn}: the device parser flags the texts ({flags:#x}: ' +
                           '; '.join(t for b, t in rle_text.FLAGS.items() if flags & b) + ') and the host parser accepts them')
    return _DeviceParse(rle_text.PendingParse(bodies, size, 'cuda' if device is None else device, parts, spare), size, host_verdict)


def counts_of(parsed: Parsed) -> np.ndarray:
    """the counts of all masks back to back, int64: `parsed.counts`, or after a parse on the device the differences of
    the starts of its run arrays"""
    if parsed.counts is not None:
        return parsed.counts
    pieces = []
    for c in parsed.device:
        n = c.hi - c.lo
        first, starts = c.host[:n + 1].astype(np.int64), c.host[n + 1:].astype(np.int64)
        pieces.append(np.delete(np.diff(starts), first[1:n] - 1))        # (without the differences across two masks)
    return np.concatenate(pieces) if pieces else np.zeros(0, dtype=np.int64)


def parse_checked(rles: Sequence, source_size: Optional[Tuple[int, int]] = None, fn: str = 'decode', *, parse: str = 'host', device=None,
                  max_masks: Optional[int] = None, max_words: Optional[int] = None, spare: int = 0) -> Parsed:
    """parse and hold to D2: one size (the dicts', else `source_size`), 1 <= H * W < 2^31, no negative count, every mask's
    counts sum to H * W.  An error names the mask.

    `parse='device'`: when every mask is a `str` / `bytes` (a dict's `counts` included) the joined bytes go up once and
    `deva.hip.rle_text` builds the run arrays on `device`, in chunks within `max_masks` / `max_words`; they come back in
    `Parsed.device` after two waits.  What the device flags is parsed again here, so the error is the host path's.  A
    call with any other mask takes the host path whole."""
    if isinstance(rles, (dict, str, bytes)) or not hasattr(rles, '__len__'):
        raise DevaHipError(f'{fn}: a list of masks expected (got {type(rles).__name__})')
    if _parse_mode(parse, fn):
        begun = _begin_device_parse(rles, source_size, fn, device, max_masks, max_words, spare)
        if begun is not None:
            return begun.finish()
    counts, per_mask, sizes = parse_many(rles)
    size = None if source_size is None else (int(source_size[0]), int(source_size[1]))
    for k, s in enumerate(sizes):
        if s is not None and size is not None and s != size:
            raise DevaHipError(f'{fn}: mask {k}: size {s[0]} x {s[1]}, the call\'s is {size[0]} x {size[1]} (one source size per call)')
        size = size or s
    if size is None:
        raise DevaHipError(f'{fn}: no mask carries its size: give `source_size`')
    h, w = size
    if h < 1 or w < 1 or h * w >= 2**31:
        raise DevaHipError(f'{fn}: bad source size {h} x {w} (1 <= H * W < 2^31)')
    first = np.cumsum(per_mask) - per_mask
    if counts.size and (int(counts.min()) < 0 or int(counts.max()) > h * w):
        k = int(np.argmax((counts < 0) | (counts > h * w)))
        mask = int(np.searchsorted(first, k, side='right')) - 1
        if counts[k] < 0:
            raise DevaHipError(f'{fn}: mask {mask}: a count is negative ({int(counts[k])})')
        raise DevaHipError(f'{fn}: mask {mask}: a count of {int(counts[k])}: the counts sum to more than H * W = {h * w}')
    sums = np.zeros(per_mask.size, dtype=np.int64)
    if counts.size:
        sums = np.add.reduceat(counts, np.minimum(first, counts.size - 1))
        sums[per_mask == 0] = 0
    wrong = np.nonzero(sums != h * w)[0]
    if wrong.size:
        raise DevaHipError(f'{fn}: mask {int(wrong[0])}: the counts sum to {int(sums[wrong[0]])}, H * W is {h * w}')
    return Parsed(counts, per_mask, h, w)


def run_array(parsed: Parsed, lo: int, hi: int) -> np.ndarray:
    """the int32 run array of the masks lo .. hi - 1 (include/deva_rle.h): first[0 .. n], then per mask its starts
    s_0 = 0, ..., s_r = H * W: one cumulative sum"""
    per = parsed.per_mask[lo:hi]
    n = hi - lo
    begin = int(parsed.per_mask[:lo].sum())
    counts = counts_of(parsed)[begin:begin + int(per.sum())]
    first = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(per + 1, out=first[1:])
    mask_of = np.repeat(np.arange(n), per)
    ends = _segment_cumsum(counts, mask_of)              # s_1 .. s_r of every mask
    words = np.zeros(n + 1 + int(first[n]), dtype=np.int32)
    words[:n + 1] = first
    words[n + 1 + np.arange(counts.size) + mask_of + 1] = ends   # (s_0 = 0 stays in front of every mask)
    return words


def chunks(per_mask: np.ndarray, max_masks: int, max_words: int, fn: str = 'decode') -> List[Tuple[int, int]]:
    """[lo, hi) ranges of masks, each within one call's limits: hi - lo <= max_masks and 2 n + 1 + runs <= max_words"""
    out, lo, words = [], 0, 1
    for k, r in enumerate(per_mask.tolist()):
        if 3 + r > max_words:
            raise DevaHipError(f'{fn}: mask {k}: {r} runs are above the limit of one call ({max_words} words)')
        if k > lo and (k - lo >= max_masks or words + r + 2 > max_words):
            out.append((lo, k))
            lo, words = k, 1
        words += r + 2
    if per_mask.size > lo:
        out.append((lo, int(per_mask.size)))
    return out


# ------------------------------------------------------------------------------------------ decode
def _sizes(parsed: Parsed, size, fn: str) -> Tuple[int, int]:
    oh, ow = (parsed.height, parsed.width) if size is None else (int(size[0]), int(size[1]))
    if oh < 1 or ow < 1 or oh * ow >= 2**31:
        raise DevaHipError(f'{fn}: bad output size {oh} x {ow} (1 <= OH * OW < 2^31)')
    return oh, ow


def _limits(max_masks, max_words, fn: str) -> Tuple[int, int]:
    top = rle_limits()
    max_masks = top.max_masks if max_masks is None else int(max_masks)
    max_words = top.max_words if max_words is None else int(max_words)
    if not (1 <= max_masks <= top.max_masks and 4 <= max_words <= top.max_words):
        raise DevaHipError(f'{fn}: limits of 1 to {top.max_masks} masks and 4 to {top.max_words} words (got {max_masks}, {max_words})')
    return max_masks, max_words


def _check_out(out, n: int, oh: int, ow: int, dtype, fn: str) -> None:
    if out is not None and (not isinstance(out, torch.Tensor) or out.dtype != dtype or tuple(out.shape) != (n, oh, ow)):
        raise DevaHipError(f'{fn}: `out` must be {dtype} [{n}, {oh}, {ow}]')


def decode(rles: Sequence, size: Optional[Tuple[int, int]] = None, *, dtype=torch.uint8, out: Optional[torch.Tensor] = None,
           source_size: Optional[Tuple[int, int]] = None, device=None, max_masks: Optional[int] = None,
           max_words: Optional[int] = None, parse: str = 'host') -> torch.Tensor:
    """N run-length masks (each in any form `parse_counts` takes) -> planes [N, OH, OW] on the device, uint8 0 / 1 or
    float32 0.0 / 1.0 (D4).  `size`: the output size; the masks' own (one per call, D2) when None; otherwise the nearest
    resize of `F.interpolate(mode='nearest')` is fused in (D3) and no source-size plane exists.  `source_size`: for masks
    that are bare texts or lists.  `out`: the contiguous device tensor to write into (it may be uninitialised).

    Everything is parsed and checked (D2) before anything is launched; an error names the mask and leaves `out` as it
    was.  Per call of the library one int32 array (pinned) goes up on the current stream, and one launch follows on it;
    nothing synchronises.  More masks or runs than one call takes (`rle_limits()`; `max_masks` / `max_words` lower the
    limits) are walked in chunks.

    `parse='device'`: the texts are parsed on the device (`parse_checked`): per chunk the joined bytes go up instead, the
    run array is built there and its host copy, which the library checks as ever, comes back in two waits."""
    fn = 'decode'
    code = _dtype_code(dtype, fn)
    target = out.device if isinstance(out, torch.Tensor) else torch.device('cuda' if device is None else device)
    if _parse_mode(parse, fn) and target.type == 'cuda':
        limits = _limits(max_masks, max_words, fn)
        with torch.cuda.device(target):
            parsed = parse_checked(rles, source_size, fn, parse=parse, device=target, max_masks=limits[0], max_words=limits[1])
    else:
        parsed = parse_checked(rles, source_size, fn)
    oh, ow = _sizes(parsed, size, fn)
    n = int(parsed.per_mask.size)
    _check_out(out, n, oh, ow, dtype, fn)
    if parsed.device is None:
        parts = chunks(parsed.per_mask, *_limits(max_masks, max_words, fn), fn)
    else:
        parts = [(c.lo, c.hi) for c in parsed.device]
    if out is None:
        device = torch.device('cuda' if device is None else device)
        if device.type != 'cuda':
            raise DevaHipError(f'{fn}: the planes live on the HIP device (got {device}); there is no CPU path')
        out = torch.empty((n, oh, ow), dtype=dtype, device=device)
    elif not out.is_cuda:
        raise DevaHipError(f'{fn}: `out` must live on the HIP device (got {out.device}); there is no CPU path')
    _planes.check_out_on_device(out, fn)
    arrays = [run_array(parsed, lo, hi) for lo, hi in parts] if parsed.device is None else [c.host for c in parsed.device]
    for (lo, hi), words in zip(parts, arrays):           # the library's own D2 on every chunk, before the first launch of the call
        check(lib().deva_rle_check(words.ctypes.data, words.size, hi - lo, parsed.height, parsed.width), 'deva_rle_check')
    with torch.cuda.device(out.device):
        stream = _stream(out.device)
        for c, ((lo, hi), words) in enumerate(zip(parts, arrays)):
            if parsed.device is None:
                host = torch.empty(words.size, dtype=torch.int32, pin_memory=True)
                host.numpy()[:] = words
                host_ptr, runs = host.data_ptr(), host.to(out.device, non_blocking=True)
            else:                                        # the run array is in place on the device; `words` is its host copy
                host_ptr, runs = words.ctypes.data, parsed.device[c].device
            part = out[lo:hi]
            check(lib().deva_rle_decode(host_ptr, runs.data_ptr(), words.size, hi - lo, parsed.height, parsed.width, oh, ow, code,
                                        part.data_ptr(), stream), 'deva_rle_decode')
    return out


# ------------------------------------------------------------------------------------------ D5
class Records(NamedTuple):
    runs: np.ndarray    # int64 [N]
    area: np.ndarray    # int64 [N]
    bbox: np.ndarray    # int64 [N,4]: x0, y0, x1, y1 inclusive at source size; -1 four times for an empty mask


def records(rles: Sequence, source_size: Optional[Tuple[int, int]] = None, *, parse: str = 'host', device=None) -> Records:
    """D5, on the host from the counts alone (`pycocotools`' area / toBbox in the convention of `FrameResult.segments`).
    `parse='device'`: the texts are parsed on `device` (`parse_checked`) and the counts come from its run arrays."""
    parsed = parse_checked(rles, source_size, 'records', parse=parse, device=device)
    h, n = parsed.height, int(parsed.per_mask.size)
    per, counts = parsed.per_mask, counts_of(parsed)
    mask_of = np.repeat(np.arange(n), per)
    local = np.arange(counts.size) - np.repeat(np.cumsum(per) - per, per)
    ends = _segment_cumsum(counts, mask_of)
    ones = np.nonzero(((local & 1) == 1) & (counts > 0))[0]
    area = np.bincount(mask_of[ones], weights=counts[ones].astype(np.float64), minlength=n).astype(np.int64)
    bbox = np.empty((n, 4), dtype=np.int64)
    bbox[:, :2], bbox[:, 2:] = np.iinfo(np.int64).max, -1
    if ones.size:
        lo, hi, m = ends[ones] - counts[ones], ends[ones] - 1, mask_of[ones]       # a run of ones: positions lo .. hi
        x_lo, x_hi = lo // h, hi // h
        whole = x_lo != x_hi                                                       # it runs on into the next column
        np.minimum.at(bbox[:, 0], m, x_lo)
        np.minimum.at(bbox[:, 1], m, np.where(whole, 0, lo % h))
        np.maximum.at(bbox[:, 2], m, x_hi)
        np.maximum.at(bbox[:, 3], m, np.where(whole, h - 1, hi % h))
    bbox[area == 0] = -1
    return Records(per.copy(), area, bbox)
