"""Numpy / pure-Python model of the JPEG decoder (dvd_amd/csrc/jpegdec.hip, definition: DESIGN.md 4.6): the header, the
self-synchronising entropy decoder (`walk` per subsequence of S bytes, iterated to its fixpoint, with the iteration count),
libjpeg's accurate integer IDCT, its triangle chroma upsampling, its colour conversion and the EXIF orientation.  Written
from the rules, not from the C source; tests/test_jpegdec_cpu.py holds it to PIL byte for byte and the sanitized CPU
restatement of the kernels to it.  It covers the files the tests feed it (baseline, what the library accepts); the library's
refusals are tested on the library."""
import io
import struct

import numpy as np

import jpeg_model as J

ROOT = J.ROOT
S = 128                                   # DVD_JPEGDEC_SUBSEQ
ZIGZAG = np.asarray(J.ZIGZAG).reshape(-1)   # position in the zig-zag sequence -> natural index


class Refused(Exception):
    pass


# ---- header -------------------------------------------------------------------------------------------------------------------
def _decode_table(bits, vals):
    """(maxcode[17], valoff[17], vals): a code of length l is valid if <= maxcode[l]; its symbol is vals[valoff[l] + code]."""
    maxcode, valoff, code, k = [-1] * 17, [0] * 17, 0, 0
    for length in range(1, 17):
        n = bits[length - 1]
        if n:
            valoff[length] = k - code
            code += n
            k += n
            maxcode[length] = code - 1
        code <<= 1
    return maxcode, valoff, list(vals)


def _orientation(payload):
    if payload[:6] != b"Exif\0\0":
        return 0
    t = payload[6:]
    e = "<" if t[:2] == b"II" else ">"
    off = struct.unpack(e + "I", t[4:8])[0]
    for i in range(struct.unpack(e + "H", t[off:off + 2])[0]):
        tag, typ, _, = struct.unpack(e + "HHI", t[off + 2 + 12 * i:off + 10 + 12 * i])
        if tag == 0x0112:
            v = struct.unpack(e + ("H" if typ == 3 else "I"), t[off + 10 + 12 * i:off + 10 + 12 * i + (2 if typ == 3 else 4)])[0]
            return v if 1 <= v <= 8 else 1
    return 0


def parse(data):
    data = bytes(data)
    assert data[:2] == b"\xff\xd8"
    hd = {"qt": {}, "huff": {}, "ri": 0, "orientation": 0}
    i = 2
    while True:
        assert data[i] == 0xFF
        m = data[i + 1]
        n = struct.unpack(">H", data[i + 2:i + 4])[0]
        seg = data[i + 4:i + 2 + n]
        if m == 0xDB:
            for p in range(0, len(seg), 65):
                hd["qt"][seg[p] & 15] = list(seg[p + 1:p + 65])
        elif m == 0xC4:
            p = 0
            while p < len(seg):
                bits = list(seg[p + 1:p + 17])
                hd["huff"][(seg[p] >> 4, seg[p] & 15)] = _decode_table(bits, seg[p + 17:p + 17 + sum(bits)])
                p += 17 + sum(bits)
        elif m == 0xC0:
            hd["h"], hd["w"], nc = struct.unpack(">HHB", seg[1:6])
            hd["comps"] = [(seg[6 + 3 * c], seg[7 + 3 * c] >> 4, seg[7 + 3 * c] & 15, seg[8 + 3 * c]) for c in range(nc)]
        elif m in (0xC1, 0xC2, 0xC3, 0xC5, 0xC6, 0xC7, 0xC9, 0xCA, 0xCB, 0xCD, 0xCE, 0xCF):
            raise Refused(f"SOF{m - 0xC0}")
        elif m == 0xDD:
            hd["ri"] = struct.unpack(">H", seg)[0]
        elif m == 0xE1 and not hd["orientation"]:
            hd["orientation"] = _orientation(seg)
        elif m == 0xDA:
            hd["tabs"] = [(seg[2 + 2 * c] >> 4, seg[2 + 2 * c] & 15) for c in range(seg[0])]
            start = i + 2 + n
            break
        i += 2 + n
    j = start
    while j < len(data):
        if data[j] != 0xFF:
            j += 1
        elif j + 1 < len(data) and (data[j + 1] == 0 or 0xD0 <= data[j + 1] <= 0xD7):
            j += 2
        else:
            break
    hd["scan"] = data[start:j]
    nc = len(hd["comps"])
    hd["hs"], hd["vs"] = hd["comps"][0][1], hd["comps"][0][2]
    hd["mcus_x"] = -(-hd["w"] // (8 * hd["hs"]))
    hd["mcus_y"] = -(-hd["h"] // (8 * hd["vs"]))
    hd["bpm"] = 1 if nc == 1 else hd["hs"] * hd["vs"] + 2
    hd["slot_comp"] = [0 if nc == 1 or s < hd["bpm"] - 2 else s - (hd["bpm"] - 2) + 1 for s in range(hd["bpm"])]
    hd["orientation"] = hd["orientation"] or 1
    return hd


# ---- the byte reader and the walk ---------------------------------------------------------------------------------------------
def _fetch(d, i):
    """('data', value, next) | ('rst', 0, index behind the marker) | ('end', 0, i)"""
    if i >= len(d):
        return "end", 0, i
    if d[i] != 0xFF:
        return "data", d[i], i + 1
    if i + 1 >= len(d):
        return "end", 0, i
    if d[i + 1] == 0:
        return "data", 0xFF, i + 2
    if 0xD0 <= d[i + 1] <= 0xD7:
        return "rst", 0, i + 2
    return "end", 0, i


def _peek(d, p):
    """16 bits at bit position p, how many of them are data, what stands behind them, where a marker ends"""
    i, off, acc, got, kind, resume = p >> 3, p & 7, 0, 0, "data", 0
    for _ in range(3):
        v = 0
        if kind == "data":
            kind, v, nx = _fetch(d, i)
            if kind == "data":
                i, got = nx, got + 8
            else:
                resume = nx
        acc = (acc << 8) | v
    return (acc >> (8 - off)) & 0xFFFF, max(0, min(16, got - off)), kind, resume


def _advance(d, p, n):
    i, t = p >> 3, (p & 7) + n
    while t >= 8:
        i += 2 if d[i] == 0xFF and i + 1 < len(d) and d[i + 1] == 0 else 1
        t -= 8
    return i * 8 + t


def walk(hd, state, stop, sink=None):
    """Decode from state = (bit position, slot, zig-zag index) until the position reaches `stop`; sink(kind, k, v) receives
    ('coef', k, v), ('block', 0, 0) and ('restart', 0, 0)."""
    d, bpm = hd["scan"], hd["bpm"]
    p, slot, k = state
    fresh = (stop, 0, 0)
    while p < stop:
        cls = 0 if k == 0 else 1
        maxcode, valoff, vals = hd["huff"][(cls, hd["tabs"][hd["slot_comp"][slot]][cls])]
        bits, avail, kind, resume = _peek(d, p)
        length = sym = 0
        for ln in range(1, 17):
            code = bits >> (16 - ln)
            if code <= maxcode[ln]:
                length, sym = ln, vals[(valoff[ln] + code) & 255]
                break
        short = length == 0 or length > avail
        s = v = 0
        p1 = p
        if not short:
            p1 = _advance(d, p, length)
            s = sym if k == 0 else sym & 15
            if s > 15:
                return fresh
            if s:
                bits2, avail2, kind2, resume2 = _peek(d, p1)
                if s > avail2:
                    short, kind, resume = True, kind2, resume2
                else:
                    raw = bits2 >> (16 - s)
                    v = raw - (1 << s) + 1 if raw < (1 << (s - 1)) else raw
                    p1 = _advance(d, p1, s)
        if short:
            if kind != "rst" or (length == 0 and avail >= 16):
                return fresh
            p, slot, k = resume * 8, 0, 0
            if sink:
                sink("restart", 0, 0)
            continue
        if k == 0:
            if sink:
                sink("coef", 0, v)
            k = 1
        elif s == 0:
            k = k + 16 if sym >> 4 == 15 else 64
        else:
            k += sym >> 4
            if k > 63:
                return fresh
            if sink:
                sink("coef", k, v)
            k += 1
        if k >= 64:
            if sink:
                sink("block", 0, 0)
            slot, k = (slot + 1) % bpm, 0
        p = p1
    return (p, slot, k)


def fixpoint(hd, max_iters=1024):
    """(E, iterations): E[j] = the state at the start of subsequence j.  Every lane of an iteration reads the states of the
    iteration before; only lanes whose input changed run.  iterations = those that changed a state plus the one that
    confirms; None instead of E when max_iters does not suffice."""
    nsub = -(-len(hd["scan"]) // S)
    E = [(j * S * 8, 0, 0) for j in range(nsub + 1)]
    changed = [True] * nsub
    for it in range(max_iters):
        new, nxt = list(E), [False] * (nsub + 1)
        for j in range(nsub):
            if changed[j]:
                s = walk(hd, E[j], (j + 1) * S * 8)
                if j + 1 < nsub and s != E[j + 1]:
                    new[j + 1], nxt[j + 1] = s, True
        E, changed = new, nxt[:nsub]
        if not any(changed):
            return E, it + 1
    return None, max_iters


def coefficients(hd, E=None):
    """int [blocks][64] in zig-zag order with DC VALUES, decoded lane by lane from the fixpoint's states (E=None: one walk
    from the start - the same blocks, which test_jpegdec_cpu.py asserts)."""
    nblocks = hd["mcus_x"] * hd["mcus_y"] * hd["bpm"]
    coef = np.zeros((nblocks + 1, 64), np.int64)
    starts = set()
    total = 0
    lanes = [((0, 0, 0), len(hd["scan"]) * 8)] if E is None else [(E[j], (j + 1) * S * 8) for j in range(len(E) - 1)]
    for state, stop in lanes:
        blk = [total]

        def sink(kind, k, v):
            if kind == "coef" and blk[0] < nblocks:
                coef[blk[0], k] = v
            elif kind == "block":
                blk[0] += 1
            elif kind == "restart":
                starts.add(blk[0])
        walk(hd, state, stop, sink)
        total = blk[0]
    if total != nblocks:
        raise Refused(f"DATA: {total} blocks, the header implies {nblocks}")
    coef = coef[:nblocks]
    run = [0, 0, 0]
    for b in range(nblocks):
        if b in starts:
            run = [0, 0, 0]
        c = hd["slot_comp"][b % hd["bpm"]]
        run[c] += coef[b, 0]
        coef[b, 0] = run[c]
    return coef


# ---- pixels -------------------------------------------------------------------------------------------------------------------
def _idct_1d(x, shift):
    """libjpeg's jidctint on the last axis of an int64 array [..., 8]"""
    z2, z3 = x[..., 2], x[..., 6]
    z1 = (z2 + z3) * 4433
    tmp2, tmp3 = z1 - z3 * 15137, z1 + z2 * 6270
    tmp0, tmp1 = (x[..., 0] + x[..., 4]) << 13, (x[..., 0] - x[..., 4]) << 13
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = x[..., 7], x[..., 5], x[..., 3], x[..., 1]
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * 9633
    tmp0, tmp1, tmp2, tmp3 = tmp0 * 2446, tmp1 * 16819, tmp2 * 25172, tmp3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
    r = 1 << (shift - 1)
    out = [tmp10 + tmp3, tmp11 + tmp2, tmp12 + tmp1, tmp13 + tmp0, tmp13 - tmp0, tmp12 - tmp1, tmp11 - tmp2, tmp10 - tmp3]
    return np.stack([(o + r) >> shift for o in out], axis=-1)


def _samples(coef_zz, q_zz):
    """[n,64] zig-zag coefficients, [64] zig-zag table -> [n,8,8] uint8"""
    nat = np.zeros((coef_zz.shape[0], 64), np.int64)
    nat[:, ZIGZAG] = coef_zz * np.asarray(q_zz, np.int64)
    blk = nat.reshape(-1, 8, 8)
    ws = _idct_1d(blk.transpose(0, 2, 1), 11).transpose(0, 2, 1)          # columns first
    v = _idct_1d(ws, 18) & 1023
    return np.where(v < 128, v + 128, np.where(v < 512, 255, np.where(v < 896, 0, v - 896))).astype(np.uint8)


def _h2v1(p):
    p = p.astype(np.int64)
    cw = p.shape[1]
    if cw <= 2:
        return np.repeat(p, 2, axis=1)
    out = np.zeros((p.shape[0], 2 * cw), np.int64)
    left, right = np.concatenate([p[:, :1], p[:, :-1]], 1), np.concatenate([p[:, 1:], p[:, -1:]], 1)
    out[:, 0::2] = (3 * p + left + 1) >> 2
    out[:, 1::2] = (3 * p + right + 2) >> 2
    out[:, 0], out[:, -1] = p[:, 0], p[:, -1]
    return out


def _h2v2(p):
    p = p.astype(np.int64)
    ch, cw = p.shape
    if cw <= 2:
        return np.repeat(np.repeat(p, 2, axis=0), 2, axis=1)
    above, below = np.concatenate([p[:1], p[:-1]], 0), np.concatenate([p[1:], p[-1:]], 0)
    out = np.zeros((2 * ch, 2 * cw), np.int64)
    for parity, nb in ((0, above), (1, below)):
        cs = 3 * p + nb
        left, right = np.concatenate([cs[:, :1], cs[:, :-1]], 1), np.concatenate([cs[:, 1:], cs[:, -1:]], 1)
        row = np.zeros((ch, 2 * cw), np.int64)
        row[:, 0::2] = (3 * cs + left + 8) >> 4
        row[:, 1::2] = (3 * cs + right + 7) >> 4
        row[:, 0], row[:, -1] = (4 * cs[:, 0] + 8) >> 4, (4 * cs[:, -1] + 7) >> 4
        out[parity::2] = row
    return out


def orient(img, o):
    """ImageOps.exif_transpose's table on an array [H,W,3]"""
    return {1: img, 2: img[:, ::-1], 3: img[::-1, ::-1], 4: img[::-1], 5: img.transpose(1, 0, 2),
            6: img.transpose(1, 0, 2)[:, ::-1], 7: img[::-1, ::-1].transpose(1, 0, 2), 8: img.transpose(1, 0, 2)[::-1]}[o]


def pixels(hd, coef):
    h, w, hs, vs, bpm = hd["h"], hd["w"], hd["hs"], hd["vs"], hd["bpm"]
    mx, my = hd["mcus_x"], hd["mcus_y"]
    nc = len(hd["comps"])
    per_mcu = coef.reshape(my, mx, bpm, 64)
    planes = []
    for c in range(nc):
        q = hd["qt"][hd["comps"][c][3]]
        if c == 0:
            s = _samples(per_mcu[:, :, :hs * vs].reshape(-1, 64), q).reshape(my, mx, vs, hs, 8, 8)
            planes.append(s.transpose(0, 2, 4, 1, 3, 5).reshape(my * vs * 8, mx * hs * 8)[:h, :w])
        else:
            s = _samples(per_mcu[:, :, hs * vs + c - 1].reshape(-1, 64), q).reshape(my, mx, 8, 8)
            plane = s.transpose(0, 2, 1, 3).reshape(my * 8, mx * 8)[:-(-h // vs), :-(-w // hs)]     # cropped BEFORE upsampling
            up = plane.astype(np.int64) if hs == 1 else _h2v1(plane) if vs == 1 else _h2v2(plane)
            planes.append(up[:h, :w])
    y = planes[0].astype(np.int64)
    if nc == 1:
        rgb = np.stack([y, y, y], axis=2)
    else:
        cb, cr = planes[1] - 128, planes[2] - 128
        rgb = np.stack([y + ((91881 * cr + 32768) >> 16), y + ((-22554 * cb - 46802 * cr + 32768) >> 16),
                        y + ((116130 * cb + 32768) >> 16)], axis=2)
    return np.ascontiguousarray(orient(rgb.clip(0, 255).astype(np.uint8), hd["orientation"]))


def decode(data, max_iters=1024, through_fixpoint=True):
    """The file -> ([H,W,3] uint8 with the orientation applied, fixpoint iterations)"""
    hd = parse(data)
    E, iters = fixpoint(hd, max_iters) if through_fixpoint else (None, 0)
    if through_fixpoint and E is None:
        raise Refused("NOSYNC")
    return pixels(hd, coefficients(hd, E)), iters


# ---- the inputs both test files use -------------------------------------------------------------------------------------------
SIZES = [(1, 1), (2, 3), (8, 8), (17, 5), (16, 16), (37, 53), (33, 48), (64, 49), (5, 40)]            # (h, w)
# (quality, subsampling: PIL's 0 = 4:4:4, 1 = 4:2:2, 2 = 4:2:0, 'gray', extra save() arguments): 7 per size and content = 126
SETTINGS = [(5, 0, {}), (50, 1, {}), (90, 2, {}), (100, 0, {}), (75, 2, {"optimize": True}), (90, 2, {"restart_marker_rows": 1}),
            (90, "gray", {"restart_marker_blocks": 3})]
CONTENTS = ("noise", "page")


def content(kind, h, w):
    return J.noise_image(h, w, seed=h * 7 + w) if kind == "noise" else J.synthetic_page("noisy", h, w, seed=h + w)


def pil_file(img, quality, subsampling, **kw):
    from PIL import Image
    out = io.BytesIO()
    if subsampling == "gray":
        Image.fromarray(img).convert("L").save(out, format="JPEG", quality=quality, **kw)
    else:
        Image.fromarray(img).save(out, format="JPEG", quality=quality, subsampling=subsampling, **kw)
    return out.getvalue()


def pil_pixels(data):
    from PIL import Image, ImageOps
    return np.ascontiguousarray(np.asarray(ImageOps.exif_transpose(Image.open(io.BytesIO(bytes(data)))).convert("RGB")))


def oriented_file(img, o, **kw):
    from PIL import Image
    exif = Image.Exif()
    exif[0x0112] = o
    return pil_file(img, kw.pop("quality", 90), kw.pop("subsampling", 2), exif=exif, **kw)


def grid():
    """name -> file: the 126 files of sizes x contents x settings"""
    files = {}
    for h, w in SIZES:
        for kind in CONTENTS:
            img = content(kind, h, w)
            for quality, ss, kw in SETTINGS:
                files[f"{h}x{w}-{kind}-q{quality}-{ss}-{'-'.join(kw) or 'plain'}"] = pil_file(img, quality, ss, **kw)
    return files


def sync_page():
    """The 300 x 400 noisy 4:2:0 page at quality 90: hundreds of subsequences that have to find each other"""
    return pil_file(J.synthetic_page("noisy", 300, 400, seed=0), 90, 2)


def sync_noise():
    return pil_file(J.noise_image(160, 200, seed=3), 95, 2)


def flat_file():
    return pil_file(np.full((400, 600, 3), 200, np.uint8), 90, 2)
