"""The statement of rules C1-C7 of include/deva_rle_text.h, written from the COCO API's published loops (rleToString /
rleFrString) as plain per-value Python loops, independent of `frame_results.coco_strings` and `rle._decode_texts`, and
the case generators of the text codec's tests.  Integers and bytes only: every comparison is exact."""
import functools

import numpy as np

import rle_case as LC

MAX_CHARS = 12
SCAN_CHUNK = 1024      # DEVA_TEXT_SCAN_CHUNK
MASK_CHUNK = 256       # DEVA_TEXT_MASK_CHUNK
FLAG_CHAR, FLAG_OPEN, FLAG_LONG, FLAG_COUNT, FLAG_SUM = 1, 2, 4, 8, 16
TOP = 2**31 - 1        # the largest H * W


# ------------------------------------------------------------------------------------------ C1, C2
def value_chars(x, width=None):
    """C1: the characters of x, canonical, or padded to `width` characters (which x must fit)"""
    out = []
    while True:
        c = x & 0x1f
        x >>= 5
        done = (x == -1) if (c & 0x10) else (x == 0)
        more = not done if width is None else len(out) + 1 < width
        assert more or done, 'the value does not fit the width'
        out.append((c | (0x20 if more else 0)) + 48)
        if not more:
            return bytes(out)


def text_of(counts, widths=None):
    """C2 over C1: one mask's counts -> its text; `widths`: per value None (canonical) or the padded width"""
    out = b''
    for j, c in enumerate(counts):
        x = int(c) - (int(counts[j - 2]) if j > 2 else 0)
        out += value_chars(x, None if widths is None else widths[j])
    return out


def max_chars(total):
    return max(len(value_chars(total)), len(value_chars(-total)))


def read_text(text, total=None):
    """rleFrString with C7 -> (counts, flags); the counts are what the loop gives where it can go on"""
    flags, counts, p = 0, [], 0
    if any(not 48 <= ch <= 111 for ch in text):
        return [], FLAG_CHAR
    while p < len(text):
        x, k, more = 0, 0, True
        while more:
            if p >= len(text):
                return counts, flags | FLAG_OPEN
            c = text[p] - 48
            if k == MAX_CHARS:
                flags |= FLAG_LONG                      # (read on: where the value ends does not depend on its width)
            x |= (c & 0x1f) << (5 * k)
            more = bool(c & 0x20)
            p += 1
            k += 1
            if not more and (c & 0x10):
                x |= -1 << (5 * k)
        if len(counts) > 2:
            x += counts[-2]
        counts.append(x)
    if total is not None:
        if any(c < 0 or c > total for c in counts):
            flags |= FLAG_COUNT
        if sum(counts) != total or not counts:
            flags |= FLAG_SUM
    return counts, flags


def run_words(texts, total):
    """C6: the run array of deva_rle.h of valid texts -> (int32 words, flags of all masks or-ed)"""
    first, starts, flags = [0], [], 0
    for t in texts:
        counts, f = read_text(t, total)
        flags |= f
        s = [0]
        for c in counts:
            s.append(s[-1] + c)
        starts += s
        first.append(first[-1] + len(s))
    return np.array([v & 0xffffffff for v in first + starts], dtype=np.uint32).view(np.int32), flags   # (flagged texts may go beyond 32 bits)


# ------------------------------------------------------------------------------------------ C3, C4
def to_bounds(all_counts, first=0):
    """lists of counts (zero only in front) -> (n int32, base int64, bounds int32) as the run-length encoder leaves them"""
    n = np.array([len(c) - 1 for c in all_counts], dtype=np.int32)
    base = (np.cumsum(n) - n).astype(np.int64) + first
    bounds = [b for c in all_counts for b in np.cumsum(np.asarray(c, dtype=np.int64))[:-1].tolist()]
    return n, base, np.array([0] * first + bounds, dtype=np.int64).astype(np.int32)


def counts_of_bounds(n, base, bounds, total):
    out = []
    for k in range(len(n)):
        slots = range(int(base[k]), int(base[k]) + int(n[k]))
        b = [0] + [int(bounds[s]) if 0 <= s < len(bounds) else total for s in slots] + [total]    # (C3: a slot outside `bounds`)
        out.append([b[i + 1] - b[i] for i in range(len(b) - 1)])
    return out


def encode_statement(n, base, bounds, total, first=0):
    """C3, C4 -> dict(texts, text_len int32, text_base int64, text_total, chars)"""
    texts = [text_of(c) for c in counts_of_bounds(n, base, bounds, total)]
    lengths = np.array([len(t) for t in texts], dtype=np.int64)
    return dict(texts=texts, text_len=lengths.astype(np.int32), text_base=np.cumsum(lengths) - lengths + first,
                text_total=int(lengths.sum()) + first, chars=np.frombuffer(b''.join(texts), dtype=np.uint8))


# ------------------------------------------------------------------------------------------ cases: values
POSITIVE_EDGES = [15, 16, 511, 512, 16383, 16384, 2**19 - 1, 2**19, 2**24 - 1, 2**24, 2**29 - 1, 2**29]
NEGATIVE_EDGES = [-16, -17, -512, -513, -16384, -16385, -2**19, -2**19 - 1, -2**24, -2**24 - 1, -2**29, -2**29 - 1]


def filled(counts, total):
    """counts with one more that brings their sum to `total`"""
    rest = total - sum(counts)
    assert rest >= 1 and all(c >= 1 for c in counts[1:]) and counts[0] >= 0
    return list(counts) + [rest]


def edge_masks(total=TOP):
    """masks whose counts (places 0..2) and differences (from place 3 on) sit on both sides of every width edge"""
    out = []
    for e in POSITIVE_EDGES:
        out.append(filled([e, e, e], total))                       # the count itself in every plain place
        out.append(filled([1, 2, 3, 2 + e], total))                # +e as a difference
        out.append(filled([0, e + 5, 1, 5, 2, 5 + e], total))      # -e - ... and +e further down the chain, a zero in front
    for e in NEGATIVE_EDGES:
        out.append(filled([1, 1 - e, 1, 1], total))                # e as a difference: 1 - (1 - e)
        out.append(filled([3, 4, 7 - e, 4, 7], total))             # in the even chain
    return out


def few_counts(total):
    """masks of 1, 2, 3, 4 and 5 counts, with and without a zero in front (an empty mask is the first)"""
    assert total >= 5
    out = [[total], [0, total]]
    for m in (3, 4, 5):
        body = [1] * (m - 1)
        out += [body + [total - (m - 1)], [0] + body[1:] + [total - (m - 2)]]
    return out


def long_mask(m, total, seed):
    """a mask of m counts (m >= 2) that sum to `total`"""
    rng = np.random.default_rng(seed)
    room = (total - 1) // (m - 1)
    assert room >= 1
    body = rng.integers(1, min(room, 40) + 1, size=m - 1).tolist()
    if seed & 1:
        body[0] = 0
    return filled(body, total)


def chunk_edge_masks(total):
    return [long_mask(m, total, m) for m in (SCAN_CHUNK - 1, SCAN_CHUNK, SCAN_CHUNK + 1, 2 * SCAN_CHUNK + 1)]


# ------------------------------------------------------------------------------------------ cases: texts
ALL_CHARS = bytes(range(48, 112))


def every_character_text():
    """one mask whose text holds every character '0'..'o' -> (text, H * W): three large plain counts in front keep both
    chains above zero, then every character that ends a value, then every other one followed by a '1'; a last value brings
    the last count to 7"""
    lift = 1 << 12
    body = bytes(ch for ch in ALL_CHARS if not (ch - 48) & 0x20) + bytes(b for ch in ALL_CHARS if (ch - 48) & 0x20 for b in (ch, 49))
    text = text_of([lift] * 3) + body
    counts, flags = read_text(text)
    assert flags == 0 and min(counts) >= 0
    text += value_chars(7 - counts[-2])
    counts, _ = read_text(text)
    total = sum(counts)
    assert read_text(text, total)[1] == 0 and set(text) >= set(ALL_CHARS) and counts[-1] == 7
    return text, total


def padded_texts(total):
    """per width 1 .. 12 one mask whose values are all padded to that width, and one canonical mask"""
    base = filled([0, 3, 1, 2, 9, 2], total)
    return [text_of(base)] + [text_of(base, [max(width, len(value_chars(x))) for x in _values(base)]) for width in range(1, MAX_CHARS + 1)]


def _values(counts):
    return [int(c) - (int(counts[j - 2]) if j > 2 else 0) for j, c in enumerate(counts)]


def zero_count_masks(total):
    half = total // 2
    return [[0, total], [half, 0, 0, total - half], [total, 0], [0, half, 0, 0, total - half, 0], [0, 0, 0, total, 0, 0]]


def straddling_texts(total):
    """masks whose multi-character values cross every boundary between two steps of a workgroup's walk over the text: for
    every offset 1 .. 11 a text in which a 12-character value begins that many characters before the second step"""
    out = []
    for back in range(1, MAX_CHARS):
        lead = SCAN_CHUNK - back                            # characters before the wide value
        ones = [1] * lead                                   # (counts 1, 1, 1, then differences 0: one character each)
        counts = filled(ones, total)
        widths = [None] * lead + [MAX_CHARS]
        text = text_of(counts, widths)
        assert len(text) == lead + MAX_CHARS
        out.append(text)
    return out


def parity_chunk_texts(total):
    """value totals at the scan-chunk edges, in both parities of the chain"""
    return [text_of(long_mask(m, total, m)) for m in (SCAN_CHUNK - 1, SCAN_CHUNK, SCAN_CHUNK + 1, SCAN_CHUNK + 2, 2 * SCAN_CHUNK + 1,
                                                       2 * SCAN_CHUNK + 2)]


def flag_cases(total):
    """name -> (a text that breaks exactly that rule of C7, the flag)"""
    good = filled([2, 3, 4], total)
    return {
        'char-low': (text_of(good)[:1] + b'/' + text_of(good)[1:], FLAG_CHAR),
        'char-high': (text_of(good) + b'p', FLAG_CHAR),
        'char-byte': (b'\xff' + text_of(good), FLAG_CHAR),
        'open': (text_of(good) + b'P', FLAG_OPEN),
        'long': (text_of(filled([2], total), [MAX_CHARS + 1, None]), FLAG_LONG),
        'negative': (text_of([1, -1, total]), FLAG_COUNT),
        'above': (text_of([0, total + 1]), FLAG_COUNT | FLAG_SUM),
        'short-sum': (text_of([1, 1, 1]) if total != 3 else text_of([1, 1]), FLAG_SUM),
        'empty-text': (b'', FLAG_SUM),
    }


@functools.lru_cache(maxsize=None)
def blob_counts(h, w, n=6):
    return [LC.counts_of(LC.blobs(h, w, seed)) for seed in range(1, n + 1)]
