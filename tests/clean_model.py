"""The scan-like page in NumPy int64: the DEFINITION the kernels of dvd_amd/csrc/clean.hip and the stand-alone
restatement clean_host_check.cpp are held to, byte for byte.  Everything is integer arithmetic and `//` is floor division.

  background  cell maxima (the cell cut at the page's edge), a closing with a (2k+1)^2 window clipped to the coarse plane, a
              separable tent 1..b+1..1 over the clipped window rounded once: bg [3,hc,wc] uint8
  flatten     bg sampled bilinearly between the cell centres (i + 1/2) s - 1/2 in units of 1 / 4 s^2, raised to one level;
              q = (v white 4 s^2 + bgQ // 2) // bgQ, out = min(255, q); counts: saturated (q > 255), floored (bgQ raised)
  binarize    Sauvola's rule on g = (R + 2G + B + 2) >> 2 with exact window sums and an exact floor square root; count: ink
"""
import numpy as np

CELLS = (4, 8, 16, 32, 64)
MAX_SIDE, MAX_CLOSE, MAX_SMOOTH, MAX_RADIUS, MAX_KQ, R = 16384, 8, 8, 63, 256, 128
STATS = ("saturated", "floored", "ink")
I = np.int64


def _check_page(img):
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3 or not (1 <= img.shape[0] <= MAX_SIDE and 1 <= img.shape[1] <= MAX_SIDE):
        raise ValueError(f"a page is [H,W,3] uint8 with sides 1..{MAX_SIDE}, got {img.shape} {img.dtype}")
    return img


def kq_of(k):
    """k as round(256 k), a half rounding up"""
    return int(np.floor(256 * float(k) + 0.5))


def gray(img):
    p = np.asarray(img).astype(I)
    return ((p[..., 0] + 2 * p[..., 1] + p[..., 2] + 2) >> 2).astype(np.uint8)


def cell_max(img, cell=16):
    """[3,hc,wc] int64: the maximum of every channel over every cell; a value is at least 0, so padding with 0 cuts the cell"""
    img = _check_page(img)
    h, w = img.shape[:2]
    hc, wc = -(-h // cell), -(-w // cell)
    pad = np.zeros((hc * cell, wc * cell, 3), I)
    pad[:h, :w] = img
    return pad.reshape(hc, cell, wc, cell, 3).max(axis=(1, 3)).transpose(2, 0, 1)


def _window(plane, k, fill, fn):
    """fn over the (2k+1)^2 window clipped to the plane: `fill` is neutral under fn"""
    n, hc, wc = plane.shape
    pad = np.full((n, hc + 2 * k, wc + 2 * k), fill, I)
    pad[:, k:k + hc, k:k + wc] = plane
    out = pad[:, k:k + hc, k:k + wc].copy()
    for dy in range(2 * k + 1):
        for dx in range(2 * k + 1):
            out = fn(out, pad[:, dy:dy + hc, dx:dx + wc])
    return out


def closing(cmax, close=2):
    return _window(_window(np.asarray(cmax, I), close, 0, np.maximum), close, 255, np.minimum)


def _tent_axis(a, b, axis):
    """the tent 1..b+1..1 along one axis over the clipped window: what lies outside has no weight"""
    a = np.moveaxis(a, axis, -1)
    n = a.shape[-1]
    pad = np.zeros(a.shape[:-1] + (n + 2 * b,), I)
    pad[..., b:b + n] = a
    out = np.zeros_like(a)
    for d in range(-b, b + 1):
        out += (b + 1 - abs(d)) * pad[..., b + d:b + d + n]
    return np.moveaxis(out, -1, axis)


def tent_terms(closed, smooth=2):
    closed = np.asarray(closed, I)
    num = _tent_axis(_tent_axis(closed, smooth, 2), smooth, 1)
    den = _tent_axis(_tent_axis(np.ones_like(closed), smooth, 2), smooth, 1)
    return num, den


def smoothed(closed, smooth=2):
    num, den = tent_terms(closed, smooth)
    return (2 * num + den) // (2 * den)


def background(img, cell=16, close=2, smooth=2, neutral=True):
    """The paper estimate [3,hc,wc] uint8."""
    if cell not in CELLS or not 0 <= close <= MAX_CLOSE or not 0 <= smooth <= MAX_SMOOTH:
        raise ValueError(f"cell {cell}, close {close}, smooth {smooth}")
    bg = smoothed(closing(cell_max(img, cell), close), smooth)
    if not neutral:
        bg = np.broadcast_to((bg[0] + 2 * bg[1] + bg[2] + 2) >> 2, bg.shape)
    return np.ascontiguousarray(bg).astype(np.uint8)


def axis_terms(n, s, nc):
    """(i0, i1, f) of the pixels 0..n-1: the two cells, clamped to 0..nc-1, and the weight of the second in units of 1/2s"""
    u = 2 * np.arange(n, dtype=I) + 1 - s
    i0 = u // (2 * s)
    f = u - 2 * s * i0
    return np.clip(i0, 0, nc - 1), np.clip(i0 + 1, 0, nc - 1), f


def bg_q(bg, h, w, cell=16):
    """[3,h,w] int64: 4 s^2 times the bilinear sample of bg at every pixel, not yet raised"""
    bg = np.asarray(bg).astype(I)
    s = cell
    y0, y1, fy = axis_terms(h, s, bg.shape[1])
    x0, x1, fx = axis_terms(w, s, bg.shape[2])
    fy = fy[None, :, None]
    top = (2 * s - fx) * bg[:, y0][:, :, x0] + fx * bg[:, y0][:, :, x1]
    bot = (2 * s - fx) * bg[:, y1][:, :, x0] + fx * bg[:, y1][:, :, x1]
    return (2 * s - fy) * top + fy * bot


def flatten(img, bg=None, cell=16, close=2, smooth=2, neutral=True, white=255):
    """(the flattened page [H,W,3] uint8, {saturated, floored})"""
    img = _check_page(img)
    if not 1 <= white <= 255 or cell not in CELLS:
        raise ValueError(f"white {white}, cell {cell}")
    h, w = img.shape[:2]
    if bg is None:
        bg = background(img, cell, close, smooth, neutral)
    one = 4 * cell * cell
    q = bg_q(bg, h, w, cell).transpose(1, 2, 0)
    low = q < one
    q = np.maximum(q, one)
    out = (img.astype(I) * white * one + q // 2) // q
    stats = {"saturated": int((out > 255).sum()), "floored": int(low.sum())}
    return np.minimum(out, 255).astype(np.uint8), stats


def window_sums(g, radius):
    """(N, S1, S2) of the (2r+1)^2 window clipped to the plane, int64 [H,W]"""
    g = np.asarray(g).astype(I)
    h, w = g.shape

    def box(a):
        c = np.zeros((h + 1, w + 1), I)
        c[1:, 1:] = a.cumsum(0).cumsum(1)
        ya, yb = np.clip(np.arange(h) - radius, 0, h), np.clip(np.arange(h) + radius + 1, 0, h)
        xa, xb = np.clip(np.arange(w) - radius, 0, w), np.clip(np.arange(w) + radius + 1, 0, w)
        return c[yb][:, xb] - c[ya][:, xb] - c[yb][:, xa] + c[ya][:, xa]

    return box(np.ones_like(g)), box(g), box(g * g)


def isqrt_floor(d):
    """floor(sqrt(d)) exactly: a float seed corrected by plus or minus 1"""
    d = np.asarray(d, I)
    s = np.floor(np.sqrt(d.astype(np.float64))).astype(I)
    s = np.where((s + 1) * (s + 1) <= d, s + 1, s)
    s = np.where(s * s > d, s - 1, s)
    assert ((s * s <= d) & ((s + 1) * (s + 1) > d)).all()
    return s


def binarize(img_or_gray, radius=15, kq=51):
    """(the plane [H,W] uint8: 0 ink, 255 paper; {ink})"""
    a = np.asarray(img_or_gray)
    g = gray(_check_page(a)) if a.ndim == 3 else a
    if g.dtype != np.uint8 or g.ndim != 2 or not 1 <= radius <= MAX_RADIUS or not 0 <= kq <= MAX_KQ:
        raise ValueError(f"radius {radius}, kq {kq}, plane {g.shape} {g.dtype}")
    g = g.astype(I)
    n, s1, s2 = window_sums(g, radius)
    sn = isqrt_floor(n * s2 - s1 * s1)
    a256 = 256 * R * n
    ink = g * n * a256 <= s1 * a256 + kq * s1 * (sn - R * n)
    return np.where(ink, 0, 255).astype(np.uint8), {"ink": int(ink.sum())}


def clean(img, flatten_page=True, binarize_page=False, cell=16, close=2, smooth=2, neutral=True, white=255, radius=15, kq=51):
    """The chain: (the page or, with binarize_page, the plane; the three counts - 0 for a stage that does not run)."""
    stats = dict.fromkeys(STATS, 0)
    out = _check_page(img)
    if flatten_page:
        out, st = flatten(out, None, cell, close, smooth, neutral, white)
        stats.update(st)
    if binarize_page:
        out, st = binarize(out, radius, kq)
        stats.update(st)
    return out, stats
