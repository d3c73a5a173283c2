"""The numpy statement of rules Z1-Z8 of include/deva_png.h: the zlib stream that `deva.hip.png` codes on the device,
written from the rules and from RFC 1951's tables (not from the kernel's closed forms), and the planes of the PNG tests.

    row_strings(plane)        Z2: uint8 [H, n + 1]
    runs(strings)             Z3: the runs of consecutive rows, never across a row's end
    segment(strings)          Z3-Z5: the bytes of one segment
    stream(plane, R)          Z6: (the whole zlib stream, info = [total, adler, 0, segments])
    stream_size(plane, R)     the total alone, vectorised over all runs: for the full-frame planes
    plan(H, W, bpp)           what deva_png_plan answers, by hand"""
import numpy as np

R = 8                 # DEVA_PNG_ROWS_PER_SEGMENT
STEP = 1024
ADLER = 65521

# RFC 1951, 3.2.5: length symbols 257 .. 285
LENGTH_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LENGTH_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]


def _reversed(code, n):
    return int(format(code, f'0{n}b')[::-1], 2)


def _fixed_code(symbol):
    """RFC 1951, 3.2.6 -> (code, bits)"""
    if symbol <= 143:
        return 0b00110000 + symbol, 8
    if symbol <= 255:
        return 0b110010000 + symbol - 144, 9
    if symbol <= 279:
        return symbol - 256, 7
    return 0b11000000 + symbol - 280, 8


def _literal(b):
    code, n = _fixed_code(b)
    return _reversed(code, n), n


def _match(length):
    """a match of `length` at distance 1 -> (its bits LSB first, how many): the length code MSB first, its extra bits
    LSB first, the distance code 00000"""
    i = max(k for k, base in enumerate(LENGTH_BASE) if base <= length)
    code, n = _fixed_code(257 + i)
    extra = length - LENGTH_BASE[i]
    assert 0 <= extra < (1 << LENGTH_EXTRA[i])
    return _reversed(code, n) | extra << n, n + LENGTH_EXTRA[i] + 5


LIT_VALUE = np.array([_literal(b)[0] for b in range(256)], dtype=np.int64)
LIT_BITS = np.array([_literal(b)[1] for b in range(256)], dtype=np.int64)
MATCH_VALUE = np.array([0, 0, 0] + [_match(m)[0] for m in range(3, 259)], dtype=np.int64)
MATCH_BITS = np.array([0, 0, 0] + [_match(m)[1] for m in range(3, 259)], dtype=np.int64)


# ------------------------------------------------------------------------------------------ Z2, Z3
def row_strings(plane):
    plane = np.asarray(plane, dtype=np.uint8)
    rows = plane.reshape(plane.shape[0], -1)
    up = np.zeros_like(rows)
    up[1:] = rows[:-1]
    out = np.empty((rows.shape[0], rows.shape[1] + 1), dtype=np.uint8)
    out[:, 0] = 2
    out[:, 1:] = rows - up
    return out


def runs(strings):
    """uint8 [rows, S] -> (value, length, row) of every run in order"""
    rows, s = strings.shape
    flat = strings.reshape(-1)
    first = np.ones(flat.size, dtype=bool)
    first[1:] = flat[1:] != flat[:-1]
    first[::s] = True
    starts = np.nonzero(first)[0]
    lengths = np.diff(np.append(starts, flat.size))
    return flat[starts].astype(np.int64), lengths.astype(np.int64), starts // s


def run_bit_counts(values, lengths):
    lit = LIT_BITS[values]
    full, rest = (lengths - 1) // 258, (lengths - 1) % 258
    return lit + 13 * full + np.where(rest >= 3, MATCH_BITS[rest], rest * lit)


def tokens(values, lengths):
    """Z3 -> (bits LSB first, bit count) of every token in order"""
    full, rest = (lengths - 1) // 258, (lengths - 1) % 258
    tail_match = rest >= 3
    count = 1 + full + np.where(tail_match, 1, rest)
    run = np.repeat(np.arange(values.size), count)
    k = np.arange(int(count.sum())) - np.repeat(np.cumsum(count) - count, count)
    literal = (k == 0) | ((k > full[run]) & ~tail_match[run])
    length = np.where(literal, 3, np.where(k <= full[run], 258, rest[run]))
    return np.where(literal, LIT_VALUE[values[run]], MATCH_VALUE[length]), np.where(literal, LIT_BITS[values[run]], MATCH_BITS[length])


def pack(values, counts):
    """tokens -> bytes: LSB first, zero bits up to the byte boundary"""
    values, counts = np.asarray(values, dtype=np.int64), np.asarray(counts, dtype=np.int64)
    token = np.repeat(np.arange(values.size), counts)
    k = np.arange(int(counts.sum())) - np.repeat(np.cumsum(counts) - counts, counts)
    return np.packbits(((values[token] >> k) & 1).astype(np.uint8), bitorder='little').tobytes()


def segment(strings):
    """Z5: the fixed-code block of these rows (BFINAL = 0), then the empty stored block"""
    values, lengths, _ = runs(strings)
    v, c = tokens(values, lengths)
    v = np.concatenate([[0b010], v, [0], [0b000]])      # block header, tokens, end-of-block, the stored block's header
    c = np.concatenate([[3], c, [7], [3]])
    return pack(v, c) + b'\x00\x00\xff\xff'


def adler32(strings):
    flat = strings.reshape(-1).astype(np.uint64)
    a = np.uint64(1) + np.cumsum(flat)
    return int(a.sum() % np.uint64(ADLER)) << 16 | int(a[-1] % np.uint64(ADLER))


def stream(plane, rows_per_segment=R):
    """Z6 -> (bytes, info)"""
    strings = row_strings(plane)
    parts = [segment(strings[y:y + rows_per_segment]) for y in range(0, strings.shape[0], rows_per_segment)]
    adler = adler32(strings)
    data = b'\x78\x01' + b''.join(parts) + b'\x03\x00' + adler.to_bytes(4, 'big')
    return data, [len(data), adler, 0, len(parts)]


def stream_size(plane, rows_per_segment=R):
    strings = row_strings(plane)
    values, lengths, row = runs(strings)
    segments = -(-strings.shape[0] // rows_per_segment)
    bits = np.bincount(row // rows_per_segment, weights=run_bit_counts(values, lengths), minlength=segments).astype(np.int64)
    return int(2 + ((3 + bits + 7 + 3 + 7) // 8 + 4).sum() + 6)


# ------------------------------------------------------------------------------------------ the plan, by hand
def plan(height, width, bpp):
    n = width * bpp
    segments = -(-height // R)

    def worst(rows):
        return -(-(3 + 9 * rows * (n + 1) + 7 + 3) // 8) + 4
    slot = -(-worst(R) // 16) * 16

    def r256(v):
        return -(-v // 256) * 256
    return dict(rows_per_segment=R, segments=segments, row_bytes=n, steps_per_row=-(-(n + 1) // STEP), block=256, slot_bytes=slot,
                scratch_bytes=3 * r256(8 * segments) + r256(slot * segments),
                worst_case=2 + (segments - 1) * worst(R) + worst(height - (segments - 1) * R) + 6)


# ------------------------------------------------------------------------------------------ planes
def blobs(height, width, objects=14, seed=0, rgb=False):
    """an id map of `objects` ellipses over background 0: uint8 [H,W] of ids, or [H,W,3] of their long-id colours"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:height, 0:width].astype(np.float32)
    ids = np.zeros((height, width), dtype=np.int64)
    for k in range(1, objects + 1):
        cy, cx = rng.uniform(0, height), rng.uniform(0, width)
        ry, rx = rng.uniform(0.05, 0.25) * height, rng.uniform(0.05, 0.25) * width
        ids[((y - cy) / ry) ** 2 + ((x - cx) / rx) ** 2 <= 1.0] = k
    if not rgb:
        return ids.astype(np.uint8)
    long_ids = ids * 1000003 % (1 << 24)
    return np.stack([long_ids % 256, long_ids // 256 % 256, long_ids // 65536], axis=-1).astype(np.uint8)


def run_rows(width, lengths=(1, 2, 3, 4, 258, 259, 260, 261, 262, 516, 517, 519), seed=0):
    """uint8 [len(lengths) + 2, W]: row k is made of runs of lengths[k] (values that differ from run to run), on top of an
    all-zero first row so the `Up` filter hands the runs on as they are; the last row repeats the one above (all zero after the filter)"""
    rng = np.random.default_rng(seed)
    rows = [np.zeros(width, dtype=np.uint8)]
    total = np.zeros(width, dtype=np.int64)
    for m in lengths:
        count = -(-width // m)
        values = (np.arange(count) * 37 + rng.integers(0, 256)) % 256     # (neighbours differ; both sides of 143 / 144)
        filtered = np.repeat(values, m)[:width]
        total = (total + filtered) % 256
        rows.append(total.astype(np.uint8))
    rows.append(rows[-1].copy())
    return np.stack(rows)
