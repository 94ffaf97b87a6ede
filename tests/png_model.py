"""A small pure-Python model of the PNG encoder's CONTAINER and the checker every PNG test uses.

The model restates the format of include/dvd_hip.h without its compressor: the per-row filter choice in NumPy, the cut of the
filtered stream into segments of S bytes, per segment ONE fixed-Huffman block of literals only followed by the empty stored
block, one IDAT per segment (the first with 78 01, the last with 03 00 and the Adler-32), the Adler-32 folded from per-segment
partials.  zlib is used for CRC-32 and Adler-32 only - never to compress.  `check_png` is the other direction: it takes a file
apart by hand and decodes it with zlib and PIL."""
import io
import os
import re
import struct
import zlib

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
ADLER_MOD = 65521
SIGNATURE = b"\x89PNG\r\n\x1a\n"


def header_segment():
    """DVD_PNG_SEGMENT as include/dvd_hip.h states it."""
    text = open(os.path.join(ROOT, "include", "dvd_hip.h")).read()
    return int(re.search(r"#define\s+DVD_PNG_SEGMENT\s+(\d+)", text).group(1))


# ---- filters ------------------------------------------------------------------------------------------------------------------
def filter_rows(img):
    """[H,W,3] uint8 -> (choice [H], filtered stream bytes): per row the filter 0..4 with the least sum of |residual as a
    signed byte|, the lowest number on a tie (np.argmin returns the first minimum)."""
    h, w, _ = img.shape
    cur = img.reshape(h, 3 * w).astype(np.int32)
    a, b, c = np.zeros_like(cur), np.zeros_like(cur), np.zeros_like(cur)
    a[:, 3:] = cur[:, :-3]
    b[1:] = cur[:-1]
    c[1:, 3:] = cur[:-1, :-3]
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    res = np.stack([(cur - pred) & 255 for pred in (0, a, b, (a + b) >> 1, paeth)])          # [5,H,3W]
    cost = np.where(res < 128, res, 256 - res).sum(axis=2)                                      # [5,H]
    choice = np.argmin(cost, axis=0)
    rows = res[choice, np.arange(h)].astype(np.uint8)
    stream = np.concatenate([choice[:, None].astype(np.uint8), rows], axis=1).tobytes()
    return choice, stream


# ---- Adler-32 from per-segment partials ---------------------------------------------------------------------------------------
def adler_partial(data):
    """(a, b) = (sum d_k, sum (n - k) d_k) mod 65521: what the segment adds to (A, B) from A = 0."""
    d = np.frombuffer(data, np.uint8).astype(np.uint64)
    n = len(d)
    return int(d.sum() % ADLER_MOD), int((d * (n - np.arange(n, dtype=np.uint64))).sum() % ADLER_MOD)


def adler_fold(A, B, n, a, b):
    """(A, B) after a segment of n bytes with partial (a, b): B += n A + b, A += a."""
    return (A + a) % ADLER_MOD, (B + (n % ADLER_MOD) * A + b) % ADLER_MOD


def adler_of_segments(segments):
    A, B = 1, 0
    for seg in segments:
        A, B = adler_fold(A, B, len(seg), *adler_partial(seg))
    return (B << 16) | A


# ---- deflate: literals only, fixed Huffman ------------------------------------------------------------------------------------
class _Bits:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, value, nbits):                 # LSB first
        self.acc |= value << self.n
        self.n += nbits
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, value, nbits):                # a Huffman code: MSB first
        self.put(int(format(value, f"0{nbits}b")[::-1], 2), nbits)

    def pad(self):
        if self.n:
            self.put(0, 8 - self.n)


def literal_segment(data, first, last):
    """The deflate bytes of one segment without any match: [78 01] block(BFINAL 0, BTYPE 01) literals, end of block, the empty
    stored block 00 00 FF FF after padding to a byte, [03 00]."""
    bits = _Bits()
    if first:
        bits.put(0x78, 8)
        bits.put(0x01, 8)
    bits.put(0, 1)
    bits.put(1, 2)
    for v in data:
        if v < 144:
            bits.code(0x30 + v, 8)
        else:
            bits.code(0x190 + v - 144, 9)
    bits.code(0, 7)
    bits.put(0, 3)
    bits.pad()
    bits.put(0x0000, 16)
    bits.put(0xFFFF, 16)
    if last:
        bits.put(1, 1)
        bits.put(1, 2)
        bits.code(0, 7)
        bits.pad()
    return bytes(bits.out)


def chunk(kind, body):
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body))


def model_file(img, segment):
    """The container around literal-only segments of `segment` stream bytes."""
    h, w, _ = img.shape
    _, stream = filter_rows(img)
    segs = [stream[i:i + segment] for i in range(0, len(stream), segment)]
    out = SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0))
    for k, seg in enumerate(segs):
        body = literal_segment(seg, k == 0, k == len(segs) - 1)
        if k == len(segs) - 1:
            body += struct.pack(">I", adler_of_segments(segs))
        out += chunk(b"IDAT", body)
    return out + chunk(b"IEND", b"")


def bound(h, w, segment):
    """dvd_png_bound restated: 10 + 9 n bits of fixed block rounded up to bytes, 5 bytes of stored block per segment."""
    stream = h * (3 * w + 1)
    ns = -(-stream // segment)
    data = lambda n: (10 + 9 * n + 7) // 8 + 5  # noqa: E731
    return 8 + 25 + 12 * ns + (ns - 1) * data(segment) + data(stream - (ns - 1) * segment) + 2 + 2 + 4 + 12


# ---- the checker --------------------------------------------------------------------------------------------------------------
def check_png(data, img, segment, limit=None):
    """Take the file apart by hand.  Returns the filter byte of every row.
    1. signature, chunk order (IHDR, one IDAT per segment, IEND, nothing else), every CRC against zlib.crc32, IHDR fields;
    2. zlib.decompress of the concatenated IDAT data (verifies the Adler-32, raises otherwise);
    3. h * (3w + 1) bytes, every filter byte in 0..4 - and equal to the NumPy restatement's choice;
    4. PIL decodes the file to the input exactly;
    5. the file is no longer than `limit` (dvd_png_bound)."""
    from PIL import Image
    data = bytes(data)
    h, w, _ = img.shape
    assert data[:8] == SIGNATURE
    pos, chunks = 8, []
    while pos < len(data):
        n, kind = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        assert len(body) == n and pos + 12 + n <= len(data), (kind, pos)
        assert struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(kind + body), (kind, pos)
        chunks.append((kind, body))
        pos += 12 + n
    assert pos == len(data)
    nseg = -(-(h * (3 * w + 1)) // segment)
    assert [k for k, _ in chunks] == [b"IHDR"] + [b"IDAT"] * nseg + [b"IEND"]
    assert chunks[0][1] == struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0) and chunks[-1][1] == b""
    idat = b"".join(body for kind, body in chunks if kind == b"IDAT")
    assert idat[:2] == b"\x78\x01"
    raw = zlib.decompress(idat)
    assert len(raw) == h * (3 * w + 1)
    rows = np.frombuffer(raw, np.uint8).reshape(h, 3 * w + 1)
    assert rows[:, 0].max() <= 4
    choice, stream = filter_rows(img)
    assert np.array_equal(rows[:, 0], choice), (rows[:, 0].tolist()[:16], choice.tolist()[:16])
    assert raw == stream
    got = np.asarray(Image.open(io.BytesIO(data)))
    assert got.shape == img.shape and np.array_equal(got, img)
    if limit is not None:
        assert len(data) <= limit, (len(data), limit)
    return rows[:, 0].copy()
