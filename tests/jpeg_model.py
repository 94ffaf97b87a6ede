"""The integer model of the JPEG encoder in NumPy and the checker every JPEG test uses.

`model_file(img, quality, subsampling)` restates the whole format of include/dvd_hip.h from the standard's definitions (ITU-T
T.81: the zig-zag walk, the Annex C code assignment, the Annex K tables, the DCT-II matrix from its cosine formula) and returns
the file's bytes; the library and the CPU restatement must produce the same bytes.  `check_jpeg` is the other direction: it
takes a file apart by hand - markers, tables, DRI, the RST sequence, byte stuffing, and a Huffman decode of the intervals that
ends on the padding of each - and opens it with PIL."""
import io
import os
import struct

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SUBSAMPLINGS = {"420": 0, "444": 1}              # DVD_JPEG_420, DVD_JPEG_444
HEADER_BYTES = 613
BLOCK_BITS_MAX = (11 + 11) + 63 * (16 + 11)      # the longest DC / AC codes of Annex K.3, 11 magnitude bits each

BASE_QUANT = np.array([
    [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112,
     100, 103, 99],
    [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99]
    + [99] * 32])
DC_BITS = [[0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0]]
DC_VALS = list(range(12))
AC_BITS = [[0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d], [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77]]
AC_VALS = [bytes.fromhex(
    "01 02 03 00 04 11 05 12 21 31 41 06 13 51 61 07 22 71 14 32 81 91 a1 08 23 42 b1 c1 15 52 d1 f0 24 33 62 72 82 09 0a 16 17 18"
    " 19 1a 25 26 27 28 29 2a 34 35 36 37 38 39 3a 43 44 45 46 47 48 49 4a 53 54 55 56 57 58 59 5a 63 64 65 66 67 68 69 6a 73 74 75"
    " 76 77 78 79 7a 83 84 85 86 87 88 89 8a 92 93 94 95 96 97 98 99 9a a2 a3 a4 a5 a6 a7 a8 a9 aa b2 b3 b4 b5 b6 b7 b8 b9 ba c2 c3"
    " c4 c5 c6 c7 c8 c9 ca d2 d3 d4 d5 d6 d7 d8 d9 da e1 e2 e3 e4 e5 e6 e7 e8 e9 ea f1 f2 f3 f4 f5 f6 f7 f8 f9 fa"), bytes.fromhex(
    "00 01 02 03 11 04 05 21 31 06 12 41 51 07 61 71 13 22 32 81 08 14 42 91 a1 b1 c1 09 23 33 52 f0 15 62 72 d1 0a 16 24 34 e1 25"
    " f1 17 18 19 1a 26 27 28 29 2a 35 36 37 38 39 3a 43 44 45 46 47 48 49 4a 53 54 55 56 57 58 59 5a 63 64 65 66 67 68 69 6a 73 74"
    " 75 76 77 78 79 7a 82 83 84 85 86 87 88 89 8a 92 93 94 95 96 97 98 99 9a a2 a3 a4 a5 a6 a7 a8 a9 aa b2 b3 b4 b5 b6 b7 b8 b9 ba"
    " c2 c3 c4 c5 c6 c7 c8 c9 ca d2 d3 d4 d5 d6 d7 d8 d9 da e2 e3 e4 e5 e6 e7 e8 e9 ea f2 f3 f4 f5 f6 f7 f8 f9 fa")]
ZRL, EOB = 0xF0, 0x00


def _zigzag():
    """position in the zig-zag sequence -> natural index 8 v + u: the anti-diagonals of T.81 figure 5, alternating direction."""
    order = []
    for s in range(15):
        diag = [(v, s - v) for v in range(8) if 0 <= s - v < 8]          # v ascending: walking down-left
        order += diag if s % 2 else diag[::-1]
    return np.array([8 * v + u for v, u in order])


ZIGZAG = _zigzag()
_u, _x = np.arange(8)[:, None], np.arange(8)[None, :]
DCT = np.rint(8192 * np.where(_u == 0, np.sqrt(0.5), 1.0) / 2 * np.cos((2 * _x + 1) * _u * np.pi / 16)).astype(np.int64)


def huff_codes(bits, vals):
    """symbol -> (code, length) by T.81 Annex C."""
    codes, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            codes[vals[k]] = (code, length)
            code, k = code + 1, k + 1
        code <<= 1
    return codes


DC_CODES = [huff_codes(DC_BITS[t], DC_VALS) for t in range(2)]
AC_CODES = [huff_codes(AC_BITS[t], AC_VALS[t]) for t in range(2)]


def quant_tables(quality):
    """[2,64] natural order: the Annex K.1 tables scaled by s = 5000 / q below 50, else 200 - 2 q."""
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return np.clip((BASE_QUANT * s + 50) // 100, 1, 255)


def geometry(h, w, subsampling):
    m = 16 if subsampling == "420" else 8
    return m, -(-w // m), -(-h // m), 6 if subsampling == "420" else 3       # MCU side, MCUs per row, MCU rows, blocks / MCU


def bound(h, w, subsampling):
    """dvd_jpeg_bound restated: per interval its blocks at BLOCK_BITS_MAX bits, rounded up to a word, every byte stuffed, and a
    marker; the header in front."""
    m, mx, my, bpm = geometry(h, w, subsampling)
    raw = (mx * bpm * BLOCK_BITS_MAX + 31) // 32 * 4
    return HEADER_BYTES + my * (2 * raw + 2)


# ---- the transform ------------------------------------------------------------------------------------------------------------
def coefficients(img, quality, subsampling):
    """[H,W,3] uint8 -> [MCU rows, MCUs per row, blocks per MCU, 64] quantised coefficients in zig-zag order."""
    h, w, _ = img.shape
    m, mx, my, bpm = geometry(h, w, subsampling)
    p = np.pad(img, ((0, my * m - h), (0, mx * m - w), (0, 0)), mode="edge").astype(np.int64)
    r, g, b = p[..., 0], p[..., 1], p[..., 2]
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    if subsampling == "420":
        cb, cr = [(c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + 2) >> 2 for c in (cb, cr)]
    q = quant_tables(quality)

    def blocks(plane, table):
        hh, ww = plane.shape
        s = (plane - 128).reshape(hh // 8, 8, ww // 8, 8).transpose(0, 2, 1, 3)                  # [by, bx, y, x]
        rows = (np.einsum("ux,abyx->abyu", DCT, s) + (1 << 10)) >> 11                             # 2 fraction bits
        f = (np.einsum("vy,abyu->abvu", DCT, rows) + (1 << 11)) >> 12                             # 3 fraction bits
        qq = 8 * table.reshape(8, 8)
        f = np.sign(f) * ((np.abs(f) + (qq >> 1)) // qq)                                         # half away from zero
        return f.reshape(hh // 8, ww // 8, 64)[..., ZIGZAG]

    yb, cbb, crb = blocks(y, q[0]), blocks(cb, q[1]), blocks(cr, q[1])
    if subsampling == "420":
        ys = [yb[dy::2, dx::2] for dy in (0, 1) for dx in (0, 1)]                                # Y00 Y01 Y10 Y11
        return np.stack(ys + [cbb, crb], axis=2)
    return np.stack([yb, cbb, crb], axis=2)


# ---- entropy coding -----------------------------------------------------------------------------------------------------------
def _symbol(code_len, value, size):
    code, length = code_len
    mag = (value if value >= 0 else value - 1) & ((1 << size) - 1)
    return (code << size) | mag, length + size


def block_bits(zz, pred, t, stats=None):
    """(bits as an int, their count) of one block; t = 0 luminance, 1 chrominance tables."""
    acc, n = 0, 0
    diff = int(zz[0]) - pred
    v, k = _symbol(DC_CODES[t][abs(diff).bit_length()], diff, abs(diff).bit_length())
    acc, n = (acc << k) | v, n + k
    last = 0
    for pos in np.flatnonzero(zz[1:]) + 1:
        run, val = int(pos) - last - 1, int(zz[pos])
        while run >= 16:
            c, k = AC_CODES[t][ZRL]
            acc, n, run = (acc << k) | c, n + k, run - 16
            if stats is not None:
                stats["zrl"] = stats.get("zrl", 0) + 1
        size = abs(val).bit_length()
        v, k = _symbol(AC_CODES[t][(run << 4) | size], val, size)
        acc, n, last = (acc << k) | v, n + k, int(pos)
    if last != 63:
        c, k = AC_CODES[t][EOB]
        acc, n = (acc << k) | c, n + k
        if stats is not None:
            stats["eob"] = stats.get("eob", 0) + 1
    return acc, n


def interval_bytes(row, stats=None):
    """One MCU row [MCUs, blocks per MCU, 64] -> its stuffed, padded bytes.  DC predictors start at 0."""
    bpm = row.shape[1]
    pred = [0, 0, 0]
    out, acc, n = bytearray(), 0, 0
    for mcu in row:
        for k in range(bpm):
            comp = max(0, k - (bpm - 3))                          # 0 for every Y block, 1 Cb, 2 Cr
            v, nb = block_bits(mcu[k], pred[comp], comp > 0, stats)
            pred[comp] = int(mcu[k][0])
            acc, n = (acc << nb) | v, n + nb
            whole = n // 8
            out += (acc >> (n - 8 * whole)).to_bytes(whole, "big")
            n -= 8 * whole
            acc &= (1 << n) - 1
    if n:
        out.append((acc << (8 - n)) | ((1 << (8 - n)) - 1))       # padded with 1-bits
    if stats is not None:
        stats["stuffed"] = stats.get("stuffed", 0) + out.count(0xFF)
    return bytes(out).replace(b"\xff", b"\xff\x00")


def header(h, w, quality, subsampling):
    m, mx, my, bpm = geometry(h, w, subsampling)
    q = quant_tables(quality)
    out = b"\xff\xd8" + b"\xff\xe0" + struct.pack(">H5sBBBHHBB", 16, b"JFIF\0", 1, 1, 0, 1, 1, 0, 0)
    out += b"\xff\xdb" + struct.pack(">H", 2 + 2 * 65) + b"".join(bytes([t]) + bytes(q[t][ZIGZAG].tolist()) for t in range(2))
    ys = 0x22 if subsampling == "420" else 0x11
    out += b"\xff\xc0" + struct.pack(">HBHHB", 17, 8, h, w, 3) + bytes([1, ys, 0, 2, 0x11, 1, 3, 0x11, 1])
    dht = b""
    for t in range(2):
        dht += bytes([t]) + bytes(DC_BITS[t]) + bytes(DC_VALS) + bytes([0x10 | t]) + bytes(AC_BITS[t]) + AC_VALS[t]
    out += b"\xff\xc4" + struct.pack(">H", 2 + len(dht)) + dht
    out += b"\xff\xdd" + struct.pack(">HH", 4, mx)
    out += b"\xff\xda" + struct.pack(">HB", 12, 3) + bytes([1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])
    assert len(out) == HEADER_BYTES
    return out


def model_intervals(img, quality, subsampling, stats=None):
    return [interval_bytes(row, stats) for row in coefficients(img, quality, subsampling)]


def assemble(h, w, quality, subsampling, intervals):
    out = header(h, w, quality, subsampling)
    for i, data in enumerate(intervals):
        out += data + (b"\xff\xd9" if i == len(intervals) - 1 else bytes([0xFF, 0xD0 + i % 8]))
    return out


def model_file(img, quality=90, subsampling="420", stats=None):
    """The whole file.  stats (a dict) receives counts of ZRL and EOB symbols and of 0xFF bytes that were stuffed."""
    h, w, _ = img.shape
    return assemble(h, w, quality, subsampling, model_intervals(img, quality, subsampling, stats))


# ---- the checker --------------------------------------------------------------------------------------------------------------
def split_file(data):
    """-> (list of (marker, body) up to and including SOS, list of interval bytes still stuffed).  Asserts the marker grammar of
    the entropy-coded data: 0xFF is followed by 0x00, by the RST marker whose number is the interval's index mod 8, or - at the
    very end - by EOI."""
    data = bytes(data)
    assert data[:2] == b"\xff\xd8"
    pos, segs = 2, []
    while True:
        assert data[pos] == 0xFF, pos
        marker, n = data[pos + 1], struct.unpack(">H", data[pos + 2:pos + 4])[0]
        segs.append((marker, data[pos + 4:pos + 2 + n]))
        pos += 2 + n
        if marker == 0xDA:
            break
    intervals, start = [], pos
    while True:
        k = data.find(b"\xff", pos)
        assert k >= 0 and k + 1 < len(data), "no EOI"
        nxt = data[k + 1]
        if nxt == 0x00:
            pos = k + 2
            continue
        intervals.append(data[start:k])
        if nxt == 0xD9:
            assert k + 2 == len(data), "bytes after EOI"
            return segs, intervals
        assert nxt == 0xD0 + (len(intervals) - 1) % 8, (hex(nxt), len(intervals) - 1)
        pos = start = k + 2


def parse_tables(segs):
    """-> (quantisation tables {id: 64 entries in zig-zag order}, Huffman tables {(class, id): (BITS, HUFFVAL)})."""
    dqt, dht = {}, {}
    for marker, body in segs:
        while marker == 0xDB and body:
            assert body[0] >> 4 == 0
            dqt[body[0] & 15], body = list(body[1:65]), body[65:]
        while marker == 0xC4 and body:
            n = sum(body[1:17])
            dht[(body[0] >> 4, body[0] & 15)], body = (list(body[1:17]), bytes(body[17:17 + n])), body[17 + n:]
    return dqt, dht


def decode_interval(data, mcus, bpm):
    """Huffman-decode one interval (still stuffed) -> [mcus, bpm, 64] coefficients in zig-zag order.  Asserts that no 0xFF in it
    is unstuffed, that exactly mcus * bpm blocks use it up to less than 8 remaining bits, and that those are 1-bits."""
    assert data.count(b"\xff") == data.count(b"\xff\x00")
    raw = data.replace(b"\xff\x00", b"\xff")
    nbits = 8 * len(raw)
    bits = bin(int.from_bytes(b"\x01" + raw, "big"))[3:]             # the stream as a string of '0' / '1'
    look = [{format(code, f"0{length}b"): sym for sym, (code, length) in table.items()} for table in DC_CODES + AC_CODES]
    pos = 0

    def take(n):
        nonlocal pos
        assert pos + n <= nbits, "interval too short"
        pos += n
        return int(bits[pos - n:pos], 2) if n else 0

    def symbol(table):
        nonlocal pos
        window = bits[pos:pos + 16]
        for length in range(1, len(window) + 1):
            sym = table.get(window[:length])
            if sym is not None:
                pos += length
                return sym
        raise AssertionError("no such code")

    def extend(size):
        v = take(size)
        return v if size == 0 or v >> (size - 1) else v - (1 << size) + 1

    out = np.zeros((mcus, bpm, 64), np.int64)
    pred = [0, 0, 0]
    for m in range(mcus):
        for k in range(bpm):
            comp = max(0, k - (bpm - 3))
            pred[comp] += extend(symbol(look[comp > 0]))
            out[m, k, 0] = pred[comp]
            i = 1
            while i < 64:
                rs = symbol(look[2 + (comp > 0)])
                if rs == EOB:
                    break
                i += rs >> 4
                if rs != ZRL:
                    assert i < 64
                    out[m, k, i] = extend(rs & 15)
                i += 1
            assert i <= 64
    rest = nbits - pos
    assert 0 <= rest < 8 and take(rest) == (1 << rest) - 1, "the interval does not end on 1-bit padding within a byte"
    return out


def check_jpeg(data, img, quality, subsampling, decode="all"):
    """Take the file apart by hand.  Returns the list of its intervals.
    1. marker order SOI APP0 DQT SOF0 DHT DRI SOS, the JFIF fields, both quantisation tables against the quality rule, SOF0
       (8 bit, h, w, three components with the subsampling's factors), the four Huffman tables, the scan header;
    2. DRI = MCUs per row, one interval per MCU row, RSTm in sequence, no unstuffed 0xFF, EOI last (`split_file`);
    3. intervals `decode` ('all' or a list of indices) are Huffman-decoded: each holds exactly its row's blocks and ends
       byte-aligned on 1-bit padding - and its coefficients are the model's for those MCU rows;
    4. PIL opens and decodes the file: mode RGB, size (w, h)."""
    from PIL import Image
    data = bytes(data)
    h, w, _ = img.shape
    m, mx, my, bpm = geometry(h, w, subsampling)
    segs, intervals = split_file(data)
    assert [mk for mk, _ in segs] == [0xE0, 0xDB, 0xC0, 0xC4, 0xDD, 0xDA]
    body = dict(segs)
    assert body[0xE0] == struct.pack(">5sBBBHHBB", b"JFIF\0", 1, 1, 0, 1, 1, 0, 0)
    dqt, dht = parse_tables(segs)
    q = quant_tables(quality)
    assert dqt == {t: q[t][ZIGZAG].tolist() for t in range(2)}
    ys = 0x22 if subsampling == "420" else 0x11
    assert body[0xC0] == struct.pack(">BHHB", 8, h, w, 3) + bytes([1, ys, 0, 2, 0x11, 1, 3, 0x11, 1])
    assert dht == {(c, t): ((DC_BITS, AC_BITS)[c][t], (bytes(DC_VALS), AC_VALS[t])[c]) for c in range(2) for t in range(2)}
    assert body[0xDD] == struct.pack(">H", mx)
    assert body[0xDA] == bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])
    assert len(intervals) == my, (len(intervals), my)
    which = range(my) if decode == "all" else decode
    for i in which:
        rows = img[i * m:(i + 1) * m]
        got = decode_interval(intervals[i], mx, bpm)
        assert np.array_equal(got, coefficients(rows, quality, subsampling)[0]), i
    im = Image.open(io.BytesIO(data))
    assert im.format == "JPEG" and im.mode == "RGB" and im.size == (w, h)
    im.load()
    return intervals


# ---- the inputs both test files use -------------------------------------------------------------------------------------------
SHAPES = [(1, 1), (8, 8), (9, 17), (17, 33), (80, 8), (8, 4104)]       # (h, w): 80 x 8 in 4:4:4 = ten intervals (RST wraps past
QUALITIES = (1, 50, 90, 100)                                           # 7), 8 x 4104 in 4:4:4 = 513 MCUs in one interval


def noise_image(h, w, seed=0):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


def smooth_image(h=48, w=200):
    """A slow ramp with a faint texture: at quality 30 most coefficients quantise to zero (long zero runs, EOB)."""
    y, x = np.mgrid[0:h, 0:w]
    v = 96 + 0.35 * x + 0.8 * y + 6 * np.sin(x / 3.0) * np.cos(y / 5.0)
    return np.stack([v, v * 0.9 + 10, 255 - v * 0.5], axis=2).clip(0, 255).astype(np.uint8)


def synthetic_page(kind, h=700, w=500, seed=0):
    """A 500 x 700 portrait page: 'smooth' (paper under uneven light), 'bars' (dark text-like bars on it), 'noisy' (the bars plus
    sensor-like noise)."""
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w]
    v = 225 - 40 * ((x / w - 0.3) ** 2 + (y / h - 0.4) ** 2) + 8 * np.sin(x / 90.0)
    page = np.stack([v, v - 4, v - 12], axis=2)
    if kind in ("bars", "noisy"):
        for row in range(40, h - 40, 18):
            start = 40
            while start < w - 60:
                length = int(rng.randint(8, 50))
                page[row:row + 9, start:min(start + length, w - 40)] = 35
                start += length + int(rng.randint(4, 12))
    if kind == "noisy":
        page = page + rng.normal(0, 6, page.shape)
    return page.clip(0, 255).astype(np.uint8)


def stress_cases():
    """name -> (image, quality): uniform noise at quality 100, full-range in the upper half (stuffed 0xFF bytes) and one-bit in
    the lower (runs of sixteen zeros between coefficients: ZRL) - test_jpeg_cpu.py asserts both on the model - and a smooth image
    at quality 30 (long zero runs, EOB)."""
    img = noise_image(48, 96, seed=7)
    img[24:] &= 1                                 # the lower half: one-bit noise, whose coefficients are mostly zero at Q = 1
    return {"noise_q100": (img, 100), "smooth_q30": (smooth_image(), 30)}
