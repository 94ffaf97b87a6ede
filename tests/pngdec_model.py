"""NumPy / Python model of the PNG decoder, written from RFC 1950 / 1951 and the PNG specification, and a PNG
WRITER for test files built on the standard zlib module.

The model restates what the kernels do, not how: the refusals, the block finder over every bit position (a dynamic block
whose header passes the checks zlib's inflate applies), the chain from segment 0 over the candidates, the val / src table,
the synchronous pointer-doubling rounds, the bands and the five filters.  `decode` returns the pixels and the statistics
(candidates, segments, rounds, bands) that pngdec_host_check prints and dvd_png_decode_rgb8 reports."""
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
DEFAULT_MAX_WORK = 1 << 20
BPP = {0: 1, 2: 3, 6: 4}


# ---- the writer ---------------------------------------------------------------------------------------------------------------
def chunk(ctype: bytes, data: bytes, crc=None) -> bytes:
    crc = zlib.crc32(ctype + data) if crc is None else crc
    return struct.pack(">I", len(data)) + ctype + data + struct.pack(">I", crc & 0xFFFFFFFF)


def paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if pa <= pb and pa <= pc else (b if pb <= pc else c)


def _paeth_np(a, b, c):
    a, b, c = a.astype(np.int32), b.astype(np.int32), c.astype(np.int32)
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def filter_rows(rows: np.ndarray, bpp: int, filters) -> bytes:
    """rows [h, w bpp] uint8 -> the filtered stream, row r with filter filters[r % len(filters)]."""
    h, n = rows.shape
    out = np.zeros((h, n + 1), np.uint8)
    zero = np.zeros(n, np.uint8)
    for r in range(h):
        f = filters[r % len(filters)]
        x = rows[r]
        a = np.concatenate([np.zeros(bpp, np.uint8), x[:-bpp]]) if n > bpp else np.zeros(n, np.uint8)
        b = rows[r - 1] if r else zero
        c = (np.concatenate([np.zeros(bpp, np.uint8), b[:-bpp]]) if n > bpp else np.zeros(n, np.uint8)) if r else zero
        xi, ai, bi = x.astype(np.int32), a.astype(np.int32), b.astype(np.int32)
        pred = (0 * xi, ai, bi, (ai + bi) >> 1, _paeth_np(a, b, c))[min(f, 4)]
        out[r, 0] = f
        out[r, 1:] = (xi - pred) & 255
    return out.tobytes()


def deflate(raw: bytes, level=6, mem_level=8, strategy=0, flushes=(), wbits=15) -> bytes:
    """zlib stream of raw; flushes: [(offset into raw, zlib.Z_SYNC_FLUSH | zlib.Z_FULL_FLUSH)]."""
    co = zlib.compressobj(level, zlib.DEFLATED, wbits, mem_level, strategy)
    out, at = [], 0
    for off, mode in sorted(flushes):
        out.append(co.compress(raw[at:off]))
        out.append(co.flush(mode))
        at = off
    out.append(co.compress(raw[at:]))
    out.append(co.flush())
    return b"".join(out)


def make_png(pixels, colour_type=2, filters=None, level=6, mem_level=8, strategy=0, idat_cuts=(), flushes=(), extra_chunks=(),
             ihdr=None, stream=None, trailer=b"") -> bytes:
    """pixels [h,w] (colour type 0), [h,w,3] (2) or [h,w,4] (6) uint8.  filters: one number or a per-row list, repeated
    (default [1, 2, 4, 3, 0]).  idat_cuts: positions of the zlib stream where a new IDAT chunk starts (a repeated position gives
    an empty chunk).  extra_chunks: [(type, data, 'before' | 'after' the IDATs)].  ihdr: fields to overwrite (depth, ctype,
    compression, filter, interlace).  stream: the zlib stream to carry instead of the one made here."""
    pixels = np.asarray(pixels, np.uint8)
    bpp = BPP[colour_type]
    h, w = pixels.shape[:2]
    rows = pixels.reshape(h, w * bpp)
    filters = [1, 2, 4, 3, 0] if filters is None else ([filters] if isinstance(filters, int) else list(filters))
    if stream is None:
        stream = deflate(filter_rows(rows, bpp, filters), level, mem_level, strategy, flushes)
    f = dict(depth=8, ctype=colour_type, compression=0, filter=0, interlace=0)
    f.update(ihdr or {})
    out = [SIGNATURE, chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, f["depth"], f["ctype"], f["compression"], f["filter"], f["interlace"]))]
    out += [chunk(t, d) for t, d, where in extra_chunks if where == "before"]
    cuts = [0] + sorted(idat_cuts) + [len(stream)]
    out += [chunk(b"IDAT", stream[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
    out += [chunk(t, d) for t, d, where in extra_chunks if where == "after"]
    out.append(chunk(b"IEND", b""))
    return b"".join(out) + trailer


def zlib_stream_of(png: bytes) -> bytes:
    """The concatenated IDAT data of a file."""
    return b"".join(d for t, d, _ in chunks_of(png) if t == b"IDAT")


def chunks_of(png: bytes):
    i, out = 8, []
    while i + 12 <= len(png):
        n = struct.unpack(">I", png[i:i + 4])[0]
        out.append((png[i + 4:i + 8], png[i + 8:i + 8 + n], struct.unpack(">I", png[i + 8 + n:i + 12 + n])[0]))
        i += 12 + n
    return out


def content(h, w, c=3, seed=0, noise=12):
    """A smooth ramp with noise and a flat margin: literals, matches near and far."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    img = (yy * 3 + xx * 2)[..., None] + np.arange(c) * 37 + rng.randint(0, noise + 1, (h, w, c))
    img[: max(1, h // 6)] = 250
    img = (img % 256).astype(np.uint8)
    return img[..., 0] if c == 1 else img


def expected_rgb(pixels, colour_type):
    pixels = np.asarray(pixels, np.uint8)
    if colour_type == 0:
        return np.repeat(pixels[..., None], 3, axis=2)
    return np.ascontiguousarray(pixels[..., :3])


# ---- the decoder model ----------------------------------------------------------------------------------------------------------
class Refused(Exception):
    def __init__(self, code):
        super().__init__(code)
        self.code = code


def parse(png: bytes):
    """-> (h, w, colour type, [(offset, data, crc ok)] of the IDAT chunks) or Refused(code)."""
    if png[:8] != SIGNATURE:
        raise Refused("HEADER")
    i, head, idat, seen, done = 8, None, [], False, False
    while True:
        if i + 12 > len(png):
            raise Refused("HEADER")
        n = struct.unpack(">I", png[i:i + 4])[0]
        if n > 0x7FFFFFFF or i + 12 + n > len(png):
            raise Refused("HEADER")
        t, d = png[i + 4:i + 8], png[i + 8:i + 8 + n]
        crc_ok = zlib.crc32(t + d) == struct.unpack(">I", png[i + 8 + n:i + 12 + n])[0]
        if head is None:
            if t != b"IHDR" or n != 13 or not crc_ok:
                raise Refused("HEADER")
            w, h, depth, ctype, comp, filt, lace = struct.unpack(">IIBBBBB", d)
            if not (1 <= w <= 0x7FFFFFFF and 1 <= h <= 0x7FFFFFFF) or ctype not in (0, 2, 3, 4, 6) or comp or filt or lace > 1:
                raise Refused("HEADER")
            if lace:
                raise Refused("INTERLACE")
            if ctype in (3, 4):
                raise Refused("COLOUR")
            if depth != 8:
                raise Refused("DEPTH")
            if 3 * h * w >= 2 ** 31:
                raise Refused("SIZE")
            head = (h, w, ctype)
        elif t == b"IHDR":
            raise Refused("HEADER")
        elif t == b"IDAT":
            if done:
                raise Refused("HEADER")
            seen = True
            idat.append((i + 8, d, crc_ok))
        else:
            done = seen
            if t == b"IEND":
                break
            if t == b"tRNS":
                raise Refused("TRNS")
            if t == b"acTL":
                raise Refused("APNG")
            if t == b"eXIf":
                raise Refused("METADATA")
            if t in (b"tEXt", b"zTXt", b"iTXt"):
                key = d.split(b"\0")[0]
                if key.startswith(b"Raw profile type") or key == b"XML:com.adobe.xmp":
                    raise Refused("METADATA")
            elif not (t[0] & 0x20) and t != b"PLTE":
                raise Refused("HEADER")
        i += 12 + n
    if not seen:
        raise Refused("HEADER")
    payload = b"".join(d for _, d, _ in idat)
    if len(payload) < 2:
        raise Refused("ZLIB")
    if payload[0] & 15 != 8 or payload[0] >> 4 > 7 or (payload[0] * 256 + payload[1]) % 31 or payload[1] & 0x20:
        raise Refused("ZLIB")
    return head + (idat, payload)


class Stream:
    """The payload as one integer: bit p of the stream is bit p of N (deflate packs from the least significant bit)."""

    def __init__(self, payload: bytes):
        self.N = int.from_bytes(payload, "little")
        self.end = 8 * len(payload)

    def peek(self, p, n):
        return (self.N >> p) & ((1 << n) - 1)


def _complete(lens, allow_single):
    """zlib's verdict on a code given by its lengths: complete; or (not for the code-length code) one code of one bit; or -
    the caller decides - no code at all."""
    used = [l for l in lens if l]
    kraft = sum(1 << (15 - l) for l in used)
    if kraft == 1 << 15:
        return True
    return allow_single and len(used) == 1 and used[0] == 1


def _canon(lens):
    """lengths -> {(length, code): symbol}, RFC 1951 3.2.2."""
    code, table = 0, {}
    for l in range(1, 16):
        for s, sl in enumerate(lens):
            if sl == l:
                table[(l, code)] = s
                code += 1
        code <<= 1
    return table


def _decode(S, p, table, maxlen):
    code = 0
    for l in range(1, maxlen + 1):
        code = (code << 1) | S.peek(p + l - 1, 1)
        if (l, code) in table:
            return table[(l, code)], l
    return None, 0


def dyn_header(S, p):
    """The header of a dynamic block whose HLIT stands at p: (position behind it, literal/length lengths, distance lengths) or
    None if zlib's inflate would refuse it."""
    hlit, hdist, hclen = S.peek(p, 5) + 257, S.peek(p + 5, 5) + 1, S.peek(p + 10, 4) + 4
    if hlit > 286 or hdist > 30:
        return None
    p += 14
    cl = [0] * 19
    for k in range(hclen):
        cl[CL_ORDER[k]] = S.peek(p + 3 * k, 3)
    p += 3 * hclen
    if sum(128 >> l for l in cl if l) != 128 or p > S.end:
        return None
    table, lens = _canon(cl), []
    while len(lens) < hlit + hdist:
        if p > S.end:
            return None
        sym, l = _decode(S, p, table, 7)
        if sym is None:
            return None
        p += l
        if sym < 16:
            lens.append(sym)
            continue
        if sym == 16:
            if not lens:
                return None
            rep, v, p = 3 + S.peek(p, 2), lens[-1], p + 2
        elif sym == 17:
            rep, v, p = 3 + S.peek(p, 3), 0, p + 3
        else:
            rep, v, p = 11 + S.peek(p, 7), 0, p + 7
        if len(lens) + rep > hlit + hdist:
            return None
        lens += [v] * rep
    ll, dd = lens[:hlit], lens[hlit:]
    if p > S.end or not ll[256] or not _complete(ll, True) or not (_complete(dd, True) or not any(dd)):
        return None
    return p, ll, dd


def find_candidates(S):
    """Bit 16 and every later bit position where a dynamic block that zlib accepts starts: sorted."""
    nbits = S.end - 16
    bits = np.unpackbits(np.frombuffer(S.N.to_bytes(S.end // 8 + 8, "little"), np.uint8), bitorder="little").astype(np.int32)
    pos = np.arange(16, S.end)
    field = lambda off, n: sum(bits[pos + off + k] << k for k in range(n))   # noqa: E731
    keep = (bits[pos + 1] == 0) & (bits[pos + 2] == 1) & (field(3, 5) <= 29) & (field(8, 5) <= 29)
    out = [16]
    for p in pos[keep].tolist():
        if p != 16 and dyn_header(S, p + 3) is not None:
            out.append(p)
    assert nbits > 0
    return out


FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 32


def walk(S, pos, max_work=DEFAULT_MAX_WORK):
    """The segment that starts at pos -> (end, tokens, flag): the block there whatever its type, then stored and fixed blocks,
    up to the next dynamic block's header ('next'), the end of the final block ('final'), invalid data ('bad') or the budget
    ('budget').  tokens: ints (literals) and (length, distance) pairs."""
    work, first, tokens = 0, True, []
    while True:
        if pos + 3 > S.end:
            return pos, tokens, "bad"
        bfinal, btype = S.peek(pos, 1), S.peek(pos + 1, 2)
        if btype == 3:
            return pos, tokens, "bad"
        if btype == 2 and not first:
            return pos, tokens, "next"
        first = False
        pos += 3
        if btype == 0:
            pos = (pos + 7) & ~7
            if pos + 32 > S.end:
                return pos, tokens, "bad"
            n = S.peek(pos, 16)
            if S.peek(pos + 16, 16) != n ^ 0xFFFF:
                return pos, tokens, "bad"
            pos += 32
            if pos + 8 * n > S.end:
                return pos, tokens, "bad"
            work += n
            if work > max_work:
                return pos, tokens, "budget"
            tokens += list(S.peek(pos, 8 * n).to_bytes(n, "little"))
            pos += 8 * n
        else:
            if btype == 1:
                ll, dd = FIXED_LL, FIXED_D
            else:
                hdr = dyn_header(S, pos)
                if hdr is None:
                    return pos, tokens, "bad"
                pos, ll, dd = hdr
            tl, td = _canon(ll), _canon(dd)
            while True:
                work += 1
                if work > max_work:
                    return pos, tokens, "budget"
                sym, l = _decode(S, pos, tl, 15)
                if sym is None or sym > 285:
                    return pos, tokens, "bad"
                pos += l
                if pos > S.end:
                    return pos, tokens, "bad"
                if sym < 256:
                    tokens.append(sym)
                    continue
                if sym == 256:
                    break
                length = LEN_BASE[sym - 257] + S.peek(pos, LEN_EXTRA[sym - 257])
                pos += LEN_EXTRA[sym - 257]
                ds, l = _decode(S, pos, td, 15)
                if ds is None or ds > 29:
                    return pos, tokens, "bad"
                dist = DIST_BASE[ds] + S.peek(pos + l, DIST_EXTRA[ds])
                pos += l + DIST_EXTRA[ds]
                if pos > S.end:
                    return pos, tokens, "bad"
                tokens.append((length, dist))
        if bfinal:
            return pos, tokens, "final"


def unfilter(stream: np.ndarray, h, w, bpp):
    """The filtered stream [h, 1 + w bpp] -> (pixels [h, w bpp], the first rows of the bands).  A band starts at row 0 and at
    every None / Sub row; within a band the rows are rebuilt top to bottom."""
    rows = stream.reshape(h, 1 + w * bpp)
    ft = rows[:, 0]
    bands = [r for r in range(h) if r == 0 or ft[r] <= 1]
    out = np.zeros((h, w * bpp), np.uint8)
    n = w * bpp
    for r in range(h):
        f, x = int(ft[r]), rows[r, 1:].astype(np.int32)
        up = out[r - 1].astype(np.int32) if r else np.zeros(n, np.int32)
        if f == 0:
            out[r] = x
        elif f == 2:
            out[r] = (x + up) & 255
        elif f == 1:
            for c in range(bpp):
                out[r, c::bpp] = np.cumsum(x[c::bpp]) & 255
        else:
            row = [0] * n
            xl, ul = x.tolist(), up.tolist()
            for i in range(n):
                a = row[i - bpp] if i >= bpp else 0
                c = ul[i - bpp] if i >= bpp else 0
                row[i] = (xl[i] + ((a + ul[i]) >> 1 if f == 3 else paeth(a, ul[i], c))) & 255
            out[r] = row
    return out, bands


def decode(png: bytes, max_work=DEFAULT_MAX_WORK):
    """-> {'status': 'OK' | a refusal code, 'rgb': [h,w,3] uint8 (OK only), 'candidates', 'segments', 'rounds', 'bands'}."""
    res = dict(status="OK", rgb=None, candidates=0, segments=0, rounds=0, bands=0)
    try:
        h, w, ctype, idat, payload = parse(png)
    except Refused as e:
        res["status"] = e.code
        return res
    bpp = BPP[ctype]
    total = h * (1 + w * bpp)
    if len(payload) < 7:
        res["status"] = "DATA"
        return res
    S = Stream(payload)
    cands = find_candidates(S)
    res["candidates"] = len(cands)
    index = {p: k for k, p in enumerate(cands)}
    pos, segs, n = 16, [], 0
    while True:
        end, tokens, flag = walk(S, pos, max_work)
        if flag in ("budget", "bad"):
            res["status"] = "NOSPLIT" if flag == "budget" else "DATA"
            res["segments"] = len(segs)
            return res
        segs.append(tokens)
        n += sum(1 if isinstance(t, int) else t[0] for t in tokens)
        res["segments"] = len(segs)
        if n > total or (flag == "next" and end not in index):
            res["status"] = "DATA"
            return res
        if flag == "final":
            break
        pos = end
    adler_at = (end + 7) // 8
    if n != total or adler_at + 4 > len(payload):
        res["status"] = "DATA"
        return res
    val, src, bad, i = np.zeros(total, np.uint8), np.arange(total, dtype=np.int64), False, 0
    for tokens in segs:
        for t in tokens:
            if isinstance(t, int):
                val[i] = t
                i += 1
            else:
                length, dist = t
                if dist > i:
                    bad = True
                else:
                    src[i:i + length] = np.arange(i - dist, i - dist + length)
                i += length
    while True:
        nxt = src[src]
        res["rounds"] += 1
        changed = bool((nxt != src).any())
        src = nxt
        if not changed:
            break
    inflated = val[src]
    bad |= zlib.adler32(inflated.tobytes()) != struct.unpack(">I", payload[adler_at:adler_at + 4])[0]
    bad |= not all(ok for _, _, ok in idat)
    ft = inflated.reshape(h, 1 + w * bpp)[:, 0]
    bad |= bool((ft > 4).any())
    res["bands"] = int(sum(1 for r in range(h) if r == 0 or ft[r] <= 1))
    if bad:
        res["status"] = "DATA"
        return res
    pix, bands = unfilter(inflated, h, w, bpp)
    assert len(bands) == res["bands"]
    pix = pix.reshape(h, w, bpp)
    res["rgb"] = np.repeat(pix, 3, axis=2) if bpp == 1 else np.ascontiguousarray(pix[..., :3])
    return res


# ---- the corpus ---------------------------------------------------------------------------------------------------------------
MIXED = [4, 4, 1, 4, 3, 0, 2, 2, 4, 1]


def corpus():
    """[(name, file, expected [h,w,3] uint8)]: small files that go wrong where pages do (the issue's table)."""
    out = []

    def add(name, pixels, ct=2, **kw):
        out.append((name, make_png(pixels, ct, **kw), expected_rgb(pixels, ct)))

    page = content(49, 64)
    add("mem2", page, mem_level=2)                       # dynamic, fixed and stored blocks in one stream
    add("mem3", page, mem_level=3)
    add("mem5_120x88", content(88, 120, seed=1), mem_level=5, filters=MIXED)
    add("level0", page, level=0)
    add("fixed", page, strategy=zlib.Z_FIXED)
    add("huffman_only", page, strategy=zlib.Z_HUFFMAN_ONLY)
    add("rle", page, strategy=zlib.Z_RLE)
    raw_len = 49 * (1 + 64 * 3)
    add("sync_flush", page, mem_level=3, flushes=[(raw_len // 3, zlib.Z_SYNC_FLUSH), (raw_len // 2, zlib.Z_SYNC_FLUSH)])
    add("full_flush", page, mem_level=3, flushes=[(raw_len // 2, zlib.Z_FULL_FLUSH)])
    # every byte of the stream equal (black, filter None): one chain of distance-1 copies as long as the stream
    add("flat_40x600", np.zeros((600, 40, 3), np.uint8), filters=0)
    # the bytes of another file's deflate stream as stored data: valid dynamic headers that the chain must step over
    inner = zlib_stream_of(out[1][1])
    wide = 1024                                           # rows longer than a header, so the filter bytes break few of them
    tall = -(-len(inner) // wide)
    hidden = np.frombuffer(inner + b"\0" * (wide * tall - len(inner)), np.uint8).reshape(tall, wide)
    add("headers_in_stored", hidden, 0, filters=0, level=0)
    for h, w in ((1, 1), (7, 1), (1, 7), (5, 3), (6, 5), (9, 7)):
        for ct in (0, 2, 6):
            add(f"edge_{h}x{w}_ct{ct}", content(h, w, BPP[ct], seed=h * w), ct, filters=MIXED)
    for ct, R in ((0, 64), (2, 21), (6, 16)):
        for h in (R - 1, R, R + 1, 2 * R + 1):
            add(f"strip_ct{ct}_h{h}", content(h, 11, BPP[ct], seed=h), ct, filters=[1, 4] + [4] * (h - 2) if h > 2 else [1])
    for ct in (0, 2, 6):
        for f in range(5):
            add(f"filter{f}_ct{ct}", content(23, 19, BPP[ct], seed=f, noise=40), ct, filters=f)
        add(f"mixed_ct{ct}", content(37, 29, BPP[ct], seed=9, noise=40), ct, filters=MIXED)
    add("all_paeth", content(45, 33, seed=4, noise=60), filters=4)
    add("all_up", content(45, 33, seed=5, noise=60), filters=2)
    # IDAT cuts: everywhere in a short stream, 1-byte and empty chunks, inside the first block's header
    tiny = content(5, 6, seed=2, noise=200)
    stream = zlib_stream_of(make_png(tiny))
    for cut in range(0, len(stream) + 1):
        add(f"cut_{cut}", tiny, idat_cuts=[cut])
    add("cut_bytes", tiny, idat_cuts=list(range(1, len(stream))))
    add("cut_empty", page, mem_level=3, idat_cuts=[0, 0, 3, 3, 4, 5, 700, 700])
    add("ancillary", page, extra_chunks=[(b"gAMA", struct.pack(">I", 45455), "before"), (b"pHYs", b"\0" * 9, "before"),
                                         (b"tEXt", b"Comment\0hello", "before"), (b"tIME", b"\0" * 7, "after")])
    return out


def refusals():
    """[(name, file, code)]: one crafted file per reason."""
    px = content(9, 8)
    good = make_png(px)
    stream = zlib_stream_of(good)
    mk = lambda **kw: make_png(px, **kw)   # noqa: E731
    cs = chunks_of(good)
    out = [
        ("signature", b"\x89PNX" + good[4:], "HEADER"),
        ("truncated", good[:-5], "HEADER"),
        ("no_iend", good[:-12], "HEADER"),
        ("chunk_too_long", good[:33] + struct.pack(">I", 1 << 20) + good[37:], "HEADER"),
        ("ihdr_crc", good[:29] + b"\0\0\0\0" + good[33:], "HEADER"),
        ("compression_method", mk(ihdr=dict(compression=1)), "HEADER"),
        ("split_idat", make_png(px, idat_cuts=[5], extra_chunks=[]).replace(chunk(b"IDAT", stream[5:]), chunk(b"tIME", b"\0" * 7) + chunk(b"IDAT", stream[5:])), "HEADER"),
        ("interlace", mk(ihdr=dict(interlace=1)), "INTERLACE"),
        ("depth16", mk(ihdr=dict(depth=16)), "DEPTH"),
        ("depth4_gray", make_png(px[..., 0], 0, ihdr=dict(depth=4)), "DEPTH"),
        ("palette", mk(ihdr=dict(ctype=3)), "COLOUR"),
        ("gray_alpha", mk(ihdr=dict(ctype=4)), "COLOUR"),
        ("trns", mk(extra_chunks=[(b"tRNS", b"\0\1\0\2\0\3", "before")]), "TRNS"),
        ("apng", mk(extra_chunks=[(b"acTL", struct.pack(">II", 1, 0), "before")]), "APNG"),
        ("exif", mk(extra_chunks=[(b"eXIf", b"MM\0*\0\0\0\x08\0\0", "before")]), "METADATA"),
        ("raw_profile", mk(extra_chunks=[(b"tEXt", b"Raw profile type exif\0\n", "before")]), "METADATA"),
        ("xmp", mk(extra_chunks=[(b"iTXt", b"XML:com.adobe.xmp\0\0\0\0\0<x/>", "before")]), "METADATA"),
        ("zlib_cm", mk(stream=bytes([0x79, 0x9C ^ 0]) + stream[2:]), "ZLIB"),
        ("zlib_check", mk(stream=bytes([stream[0], stream[1] ^ 1]) + stream[2:]), "ZLIB"),
        ("zlib_dict", mk(stream=bytes([0x78, 0xBB]) + stream[2:]), "ZLIB"),
        ("size", SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", 30000, 30000, 8, 2, 0, 0, 0)) + b"".join(chunk(t, d) for t, d, _ in cs[1:]), "SIZE"),
    ]
    # after launches: damaged data
    flip = bytearray(stream)
    flip[len(stream) // 2] ^= 0x10
    adler = stream[:-4] + bytes([stream[-4] ^ 1]) + stream[-3:]
    crc = bytearray(good)
    at = good.index(b"IDAT") + 4 + len(stream)
    crc[at] ^= 1
    out += [
        ("flipped_bit", mk(stream=bytes(flip)), "DATA"),
        ("adler", mk(stream=adler), "DATA"),
        ("idat_crc", bytes(crc), "DATA"),
        ("filter_byte", mk(stream=zlib.compress(b"\5" + filter_rows(px.reshape(9, 24), 3, [0])[1:])), "DATA"),
        ("too_short", mk(stream=zlib.compress(filter_rows(px.reshape(9, 24), 3, [0])[:-3])), "DATA"),
        ("too_long", mk(stream=zlib.compress(filter_rows(px.reshape(9, 24), 3, [0]) + b"\0")), "DATA"),
        ("distance", mk(stream=b"\x78\x9c" + _far_match() + b"\0\0\0\0"), "DATA"),
    ]
    return out


def _far_match():
    """A final fixed block whose first token is a match: a distance reaching before the start of the stream."""
    bits, n = 0, 0

    def put(v, k, msb=False):
        nonlocal bits, n
        if msb:
            v = int(format(v, f"0{k}b")[::-1], 2)
        bits |= v << n
        n += k

    put(1, 1)
    put(1, 2)
    for _ in range(75):                                   # 75 matches of 3 = 225 bytes = 9 rows of 1 + 24
        put(0b0000001, 7, True)                           # length symbol 257: 3
        put(0, 5, True)                                   # distance symbol 0: 1
    put(0, 7, True)                                       # end of block
    return bits.to_bytes((n + 7) // 8, "little")
