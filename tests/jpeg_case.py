"""The numpy statement of rules J1-J10 of include/deva_jpeg.h: the baseline JPEG that `deva.hip.jpeg` codes on the device,
written from the rules and from the tables of ITU-T T.81 Annex K (not from the kernel), and the images of the JPEG tests.

    quant_tables(quality)                 J5: (luminance, chrominance), uint8 [64] each in zigzag order, as a DQT holds them
    coefficients(rgb, quality, sub)       J1-J5, J7: int32 [blocks, 64] in zigzag order, blocks in scan order; component of each
    tokens(coef, comp, interval_of)       J6, J8: (value, bits, interval) of every code word in stream order, and the symbols
    scan(rgb, quality, sub, restart)      J6-J9: (the entropy-coded data with its restart markers, info = [total, blocks, 0, intervals])
    file_bytes(scan, h, w, ...)           J10, by hand (the binding's own `file_bytes` must agree)
    plan(h, w, sub, restart)              what deva_jpeg_plan answers, by hand
    overlay(h, w, seed)                   a frame with translucent blobs on it, as `blend` looks
    crafted()                             the image of black, white and checkerboard blocks that reaches the corners of the code"""
import numpy as np

BLOCK = 256                      # blocks a workgroup codes in one step
BLOCK_BITS = 20 + 63 * 26        # the longest block: a DC code of 9 + 11 bits, 63 AC codes of 16 + 10 bits
MAX_SIDE = 16384
MAX_BYTES = 1 << 29

# ITU-T T.81, Annex K.1 (natural order)
LUMINANCE = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
             18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99]
CHROMINANCE = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32

# Annex K.3: (how many codes of each length 1 .. 16, the symbols in code order)
DC_LUMINANCE = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMINANCE = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMINANCE = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d], list(bytes.fromhex(
    '01020300041105122131410613516107227114328191a1082342b1c11552d1f0243362728209'
    '0a161718191a25262728292a3435363738393a434445464748494a535455565758595a636465'
    '666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9'
    'aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9ea'
    'f1f2f3f4f5f6f7f8f9fa')))
AC_CHROMINANCE = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77], list(bytes.fromhex(
    '000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a16'
    '2434e125f11718191a262728292a35363738393a434445464748494a535455565758595a6364'
    '65666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7'
    'a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9'
    'eaf2f3f4f5f6f7f8f9fa')))
assert len(AC_LUMINANCE[1]) == len(AC_CHROMINANCE[1]) == 162 and sum(AC_LUMINANCE[0]) == sum(AC_CHROMINANCE[0]) == 162


def _zigzag():
    """ZIGZAG[z] = the natural index (row * 8 + column) of the z-th coefficient of the scan (T.81, figure A.6)"""
    order = sorted(range(64), key=lambda i: (i // 8 + i % 8, (i // 8) if (i // 8 + i % 8) % 2 else (i % 8)))
    return np.array(order, dtype=np.int64)


ZIGZAG = _zigzag()
assert ZIGZAG[:10].tolist() == [0, 1, 8, 16, 9, 2, 3, 10, 17, 24] and ZIGZAG[-3:].tolist() == [55, 62, 63]


def _codes(table):
    """Annex C: the canonical code of every symbol -> (code [256], bits [256]); bits 0 where the table has no code"""
    counts, symbols = table
    code = np.zeros(256, dtype=np.int64)
    bits = np.zeros(256, dtype=np.int64)
    value, k = 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            code[symbols[k]], bits[symbols[k]] = value, length
            value += 1
            k += 1
        value <<= 1
    return code, bits


CODES = {name: _codes(table) for name, table in (('dc0', DC_LUMINANCE), ('dc1', DC_CHROMINANCE), ('ac0', AC_LUMINANCE), ('ac1', AC_CHROMINANCE))}

# J4: the integer DCT matrix
DCT = np.array([[int(np.rint(8192 * (np.sqrt(1 / 8) if k == 0 else 0.5) * np.cos((2 * n + 1) * k * np.pi / 16))) for n in range(8)] for k in range(8)],
               dtype=np.int64)
assert int(np.abs(DCT).sum(axis=1).max()) * 128 < 1 << 22                                   # the row pass, before its shift
assert int(np.abs(DCT).sum(axis=1).max()) * (((int(np.abs(DCT).sum(axis=1).max()) * 128 + 1024) >> 11) + 1) < 1 << 28   # the column pass


def sub_code(subsampling):
    return {'4:2:0': 420, '4:4:4': 444}[subsampling]


# ------------------------------------------------------------------------------------------ J5
def quant_tables(quality):
    q = int(quality)
    assert 1 <= q <= 100
    s = 5000 // q if q < 50 else 200 - 2 * q
    out = []
    for base in (LUMINANCE, CHROMINANCE):
        table = np.clip((np.array(base, dtype=np.int64) * s + 50) // 100, 1, 255)
        out.append(table[ZIGZAG].astype(np.uint8))
    return out


# ------------------------------------------------------------------------------------------ J1-J5, J7
def _pad(plane, mcu):
    h, w = plane.shape
    return np.pad(plane, ((0, -h % mcu), (0, -w % mcu)), mode='edge')


def _blocks(plane):
    """[H8, W8] -> [H8 / 8, W8 / 8, 8, 8]"""
    h, w = plane.shape
    return plane.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3)


def _transform(blocks, table_zigzag):
    """J4, J5 on [..., 8, 8] samples (0 .. 255) -> [..., 64] in zigzag order"""
    x = blocks.astype(np.int64) - 128
    t = (np.einsum('kn,...rn->...rk', DCT, x) + 1024) >> 11
    u = np.einsum('kr,...rc->...kc', DCT, t)
    assert np.abs(u).max(initial=0) < 1 << 28
    natural = np.empty(64, dtype=np.int64)
    natural[ZIGZAG] = table_zigzag.astype(np.int64)
    q = natural.reshape(8, 8)
    c = np.sign(u) * ((np.abs(u) + (q << 14)) // (q << 15))
    return c.reshape(*c.shape[:-2], 64)[..., ZIGZAG]


def coefficients(rgb, quality=75, subsampling='4:2:0'):
    """-> (int64 [blocks, 64] in zigzag order, blocks in the order of J7; the component 0 / 1 / 2 of every block; the
    MCU of every block)"""
    rgb = np.asarray(rgb)
    assert rgb.dtype == np.uint8 and rgb.ndim == 3 and rgb.shape[2] == 3
    r, g, b = (rgb[..., k].astype(np.int64) for k in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = ((-11059 * r - 21709 * g + 32768 * b + 32767) >> 16) + 128
    cr = ((32768 * r - 27439 * g - 5329 * b + 32767) >> 16) + 128
    assert min(y.min(), cb.min(), cr.min()) >= 0 and max(y.max(), cb.max(), cr.max()) <= 255
    lum, chrom = quant_tables(quality)
    if subsampling == '4:2:0':
        y, cb, cr = (_pad(p, 16) for p in (y, cb, cr))
        cb, cr = ((p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + 2) >> 2 for p in (cb, cr))
        yb = _transform(_blocks(y), lum)                                  # [2 my, 2 mx, 64]
        my, mx = yb.shape[0] // 2, yb.shape[1] // 2
        yb = yb.reshape(my, 2, mx, 2, 64).transpose(0, 2, 1, 3, 4).reshape(my, mx, 4, 64)
        parts = [yb, _transform(_blocks(cb), chrom)[:, :, None], _transform(_blocks(cr), chrom)[:, :, None]]
        comp = [0, 0, 0, 0, 1, 2]
    else:
        assert subsampling == '4:4:4'
        y, cb, cr = (_pad(p, 8) for p in (y, cb, cr))
        parts = [_transform(_blocks(y), lum)[:, :, None], _transform(_blocks(cb), chrom)[:, :, None], _transform(_blocks(cr), chrom)[:, :, None]]
        my, mx = parts[0].shape[:2]
        comp = [0, 1, 2]
    coef = np.concatenate(parts, axis=2)                                  # [my, mx, blocks per MCU, 64]
    per = coef.shape[2]
    mcu = np.repeat(np.arange(my * mx), per)
    return coef.reshape(-1, 64), np.tile(np.array(comp), my * mx), mcu


def geometry(h, w, subsampling='4:2:0', restart=0):
    """-> (MCU side, MCUs across, MCUs down, blocks per MCU, MCUs per interval, intervals)"""
    side, per = (16, 6) if subsampling == '4:2:0' else (8, 3)
    mx, my = -(-w // side), -(-h // side)
    every = int(restart) if restart else mx
    assert 0 < every <= 65535
    return side, mx, my, per, every, -(-(mx * my) // every)


# ------------------------------------------------------------------------------------------ J6, J8
def _category(v):
    """bits of |v|"""
    a = np.abs(v)
    out = np.zeros(a.shape, dtype=np.int64)
    for k in range(12):
        out += a >= (1 << k)
    return out


def tokens(coef, comp, interval):
    """the code words of all blocks in stream order -> (value, bits, interval, symbols) with symbols a list of
    (kind 'dc' / 'ac', table 0 / 1, symbol) arrays for the coverage test"""
    n = coef.shape[0]
    chroma = (comp > 0).astype(np.int64)
    # the DC difference against the previous block of the same component within the interval
    dc = coef[:, 0]
    diff = dc.copy()
    for c in range(3):
        idx = np.nonzero(comp == c)[0]
        prev = np.concatenate([[0], dc[idx[:-1]]])
        first = np.concatenate([[True], interval[idx[1:]] != interval[idx[:-1]]])
        diff[idx] = dc[idx] - np.where(first, 0, prev)
    size = _category(diff)
    assert size.max(initial=0) <= 11
    dc_code = np.where(chroma == 0, CODES['dc0'][0][size], CODES['dc1'][0][size])
    dc_bits = np.where(chroma == 0, CODES['dc0'][1][size], CODES['dc1'][1][size])
    extra = np.where(diff >= 0, diff, diff + (1 << size) - 1)
    # every token: (block, position within the block's tokens, value, bits)
    block = [np.arange(n)]
    order = [np.zeros(n, dtype=np.int64)]
    value = [dc_code << size | extra]
    bits = [dc_bits + size]
    # AC: the non-zero coefficients in (block, k) order
    b, k = np.nonzero(coef[:, 1:])
    k = k + 1
    v = coef[b, k]
    first = np.concatenate([[True], b[1:] != b[:-1]])
    prev = np.where(first, 0, np.concatenate([[0], k[:-1]]))
    run = k - prev - 1
    size = _category(v)
    assert size.max(initial=0) <= 10
    symbol = (run & 15) << 4 | size
    ch = chroma[b]
    code = np.where(ch == 0, CODES['ac0'][0][symbol], CODES['ac1'][0][symbol])
    nbits = np.where(ch == 0, CODES['ac0'][1][symbol], CODES['ac1'][1][symbol])
    assert (nbits > 0).all()
    extra = np.where(v >= 0, v, v + (1 << size) - 1)
    block.append(b), order.append(4 * k + 3), value.append(code << size | extra), bits.append(nbits + size)
    # ZRL: run >> 4 of them in front of the coefficient's own code (up to 3)
    zrl_symbols = []
    for j in range(3):
        sel = (run >> 4) > j
        ch_j = ch[sel]
        block.append(b[sel]), order.append(4 * k[sel] + j)
        value.append(np.where(ch_j == 0, CODES['ac0'][0][0xF0], CODES['ac1'][0][0xF0]))
        bits.append(np.where(ch_j == 0, CODES['ac0'][1][0xF0], CODES['ac1'][1][0xF0]))
        zrl_symbols.append(ch_j)
    # EOB unless coefficient 63 is non-zero
    eob = np.nonzero(coef[:, 63] == 0)[0]
    block.append(eob), order.append(np.full(eob.size, 4 * 64, dtype=np.int64))
    value.append(np.where(chroma[eob] == 0, CODES['ac0'][0][0], CODES['ac1'][0][0]))
    bits.append(np.where(chroma[eob] == 0, CODES['ac0'][1][0], CODES['ac1'][1][0]))
    block, order, value, bits = (np.concatenate(p) for p in (block, order, value, bits))
    at = np.lexsort((order, block))
    symbols = dict(dc=_category(diff), ac=symbol, zrl=int(sum(z.size for z in zrl_symbols)), eob=int(eob.size), blocks=n)
    return value[at], bits[at], interval[block[at]], symbols


def _pack(value, bits, interval, intervals):
    """J8: MSB first, every interval padded with 1-bits to a byte -> (uint8 bytes, the interval of every byte)"""
    per = np.bincount(interval, weights=bits, minlength=intervals).astype(np.int64)
    pad = -per % 8
    nbytes = (per + pad) // 8
    base = np.concatenate([[0], np.cumsum(nbytes)])
    value = np.concatenate([value, (1 << pad) - 1])
    bits = np.concatenate([bits, pad])
    inter = np.concatenate([interval, np.arange(intervals)])
    at = np.argsort(inter, kind='stable')                    # the padding behind its interval's tokens
    value, bits, inter = value[at], bits[at], inter[at]
    ends = np.cumsum(bits)
    start = ends - bits - (np.concatenate([[0], np.cumsum(per + pad)])[inter]) + 8 * base[inter]
    out = np.zeros(int(base[-1]) + 5, dtype=np.uint8)
    window = value << (40 - (start & 7) - bits)              # bits <= 27: five bytes hold it at any of the 8 phases
    assert bits.max(initial=0) <= 27
    first = start >> 3
    for j in range(5):
        np.bitwise_or.at(out, first + j, ((window >> (32 - 8 * j)) & 255).astype(np.uint8))
    return out[:int(base[-1])], np.repeat(np.arange(intervals), nbytes)


def _stuff(data, of, intervals):
    """J9, and the RSTm marker behind every interval but the last"""
    ff = (data == 0xFF).astype(np.int64)
    before = np.cumsum(ff) - ff
    at = np.arange(data.size) + before + 2 * of
    total = data.size + int(ff.sum()) + 2 * (intervals - 1)
    out = np.zeros(total, dtype=np.uint8)
    out[at] = data
    ends = np.nonzero(np.concatenate([of[1:] != of[:-1], [False]]))[0] if data.size else np.zeros(0, dtype=np.int64)
    assert ends.size == intervals - 1                       # (no interval is empty: each has a DC code at least)
    m = of[ends]
    out[at[ends] + ff[ends] + 1] = 0xFF
    out[at[ends] + ff[ends] + 2] = 0xD0 + (m & 7)
    return out


def scan(rgb, quality=75, subsampling='4:2:0', restart=0, detail=False):
    """-> (the entropy-coded data with its restart markers as bytes, info = [total, blocks, 0, intervals])"""
    h, w = np.asarray(rgb).shape[:2]
    _, mx, my, per, every, intervals = geometry(h, w, subsampling, restart)
    coef, comp, mcu = coefficients(rgb, quality, subsampling)
    value, bits, interval, symbols = tokens(coef, comp, mcu // every)
    data, of = _pack(value, bits, interval, intervals)
    out = _stuff(data, of, intervals)
    info = [int(out.size), int(coef.shape[0]), 0, int(intervals)]
    if detail:
        symbols.update(stuffed=int((data == 0xFF).sum()), intervals=intervals)
        return out.tobytes(), info, symbols
    return out.tobytes(), info


# ------------------------------------------------------------------------------------------ J10 by hand
def _segment(marker, payload):
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, 'big') + payload


def file_bytes(data, h, w, quality=75, subsampling='4:2:0', restart=0):
    _, mx, _, _, every, _ = geometry(h, w, subsampling, restart)
    lum, chrom = quant_tables(quality)
    out = [b'\xff\xd8', _segment(0xE0, b'JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00')]
    out += [_segment(0xDB, bytes([0]) + lum.tobytes()), _segment(0xDB, bytes([1]) + chrom.tobytes())]
    sampling = 0x22 if subsampling == '4:2:0' else 0x11
    out.append(_segment(0xC0, bytes([8]) + h.to_bytes(2, 'big') + w.to_bytes(2, 'big') + bytes([3, 1, sampling, 0, 2, 0x11, 1, 3, 0x11, 1])))
    for ident, (counts, symbols) in ((0x00, DC_LUMINANCE), (0x10, AC_LUMINANCE), (0x01, DC_CHROMINANCE), (0x11, AC_CHROMINANCE)):
        out.append(_segment(0xC4, bytes([ident]) + bytes(counts) + bytes(symbols)))
    out.append(_segment(0xDD, every.to_bytes(2, 'big')))
    out.append(_segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])))
    return b''.join(out) + bytes(data) + b'\xff\xd9'


def encode(rgb, quality=75, subsampling='4:2:0', restart=0):
    h, w = np.asarray(rgb).shape[:2]
    return file_bytes(scan(rgb, quality, subsampling, restart)[0], h, w, quality, subsampling, restart)


def segments(file):
    """the marker segments in front of the scan of a JPEG file -> {marker: [payloads]}"""
    assert file[:2] == b'\xff\xd8'
    out, at = {}, 2
    while True:
        assert file[at] == 0xFF
        marker, size = file[at + 1], int.from_bytes(file[at + 2:at + 4], 'big')
        out.setdefault(marker, []).append(file[at + 4:at + 2 + size])
        at += 2 + size
        if marker == 0xDA:
            return out


# ------------------------------------------------------------------------------------------ the plan by hand
def _round256(v):
    return -(-v // 256) * 256


def interval_worst(blocks):
    """every block at BLOCK_BITS, padded to a byte, every byte stuffed, and the marker"""
    return 2 * -(-(blocks * BLOCK_BITS) // 8) + 2


def plan(h, w, subsampling='4:2:0', restart=0):
    side, mx, my, per, every, intervals = geometry(h, w, subsampling, restart)
    blocks = mx * my * per
    last = mx * my - (intervals - 1) * every
    slot = -(-interval_worst(min(every, mx * my) * per) // 16) * 16 + 16
    coef_bytes = blocks * 128
    scratch = 2 * _round256(8 * intervals) + _round256(coef_bytes) + _round256(slot * intervals)
    worst = (intervals - 1) * interval_worst(every * per) + interval_worst(last * per) - 2
    return dict(mcu=side, mcus_x=mx, mcus_y=my, blocks_per_mcu=per, restart=every, intervals=intervals, blocks=blocks, block=BLOCK,
                coef_bytes=coef_bytes, slot_bytes=slot, scratch_bytes=scratch, worst_case=worst)


# ------------------------------------------------------------------------------------------ images
def overlay(h, w, seed):
    """a smooth frame with sensor noise and a few translucent coloured blobs with hard edges on it: what `blend` holds"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    frame = np.stack([128 + 90 * np.sin(xx / (17 + 5 * k) + k) * np.cos(yy / (23 - 3 * k)) for k in range(3)], axis=-1)
    frame += rng.normal(0, 4, frame.shape)
    for _ in range(6):
        cy, cx, ry, rx = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(h / 12 + 1, h / 3 + 2), rng.uniform(w / 12 + 1, w / 3 + 2)
        inside = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1
        frame[inside] = 0.5 * frame[inside] + 0.5 * rng.uniform(0, 255, 3)
    return np.clip(np.rint(frame), 0, 255).astype(np.uint8)


def psnr(a, b):
    err = np.mean((np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)) ** 2)
    return 99.0 if err == 0 else float(10 * np.log10(255 ** 2 / err))


def crafted(rows=20, cols=12, seed=7):
    """8 x 8 blocks drawn from black, white, a single-pixel black / white checkerboard and a single-pixel checkerboard of
    two neighbouring grays (one level apart: only its highest frequencies survive, behind a long run of zeros)"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:8, 0:8]
    board = ((yy + xx) & 1).astype(np.uint8)
    kinds = [np.zeros((8, 8), np.uint8), np.full((8, 8), 255, np.uint8), board * 255, 255 - board * 255, 128 + board]
    pick = rng.integers(0, len(kinds), (rows, cols))
    pick[0, :5] = [0, 1, 2, 4, 3]
    gray = np.block([[kinds[k] for k in row] for row in pick])
    return np.repeat(gray[:, :, None], 3, axis=2)
