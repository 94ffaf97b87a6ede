"""The synthetic-document render in NumPy: THE DEFINITION.  dvd_amd/csrc/synth_core.h is the same arithmetic for
the kernels of synth.hip and for the stand-alone CPU restatement synth_host_check.cpp.

A flat scan [hs,ws,3] u8 is drawn on a photograph of h x w through fwd [h,w,2] f32, the forward field of the map inverse
(tests/mapinv_model.py: photograph pixel -> page position, 0xffffffff where the page does not cover the pixel).  Every float32
line below is one separately rounded operation of the kernels; everything behind the Q8 position is integer."""
import numpy as np

F = np.float32
I = np.int64
INVALID = np.uint32(0xffffffff)
MAX_SIDE, MAX_RADIUS = 16384, 8
NO_SHADING = dict(l0=0.0, lgx=0.0, lgy=0.0, k=0.0, a_ref=1.0)


def covered_of(fwd):
    return np.ascontiguousarray(fwd, F).view(np.uint32)[..., 0] != INVALID


def axis_scale(ns, n):
    return F(ns - 1) / F(n - 1) if n > 1 else F(0)


def scan_q8(u, k, ns):
    """floor(u k 256 + 1/2) clamped to [0, 256 (ns - 1)], each operation rounded to f32; a NaN gives 0."""
    with np.errstate(all="ignore"):
        f = np.floor((((u * k).astype(F) * F(256)).astype(F) + F(0.5)).astype(F))
        return np.where(f >= 0, np.minimum(f, F(256 * (ns - 1))), F(0)).astype(I)


def scan_positions(fwd, hs, ws):
    """(sx, sy int64 [h,w], covered [h,w]): the Q8 scan position of every photograph pixel (0 where uncovered)."""
    fwd = np.ascontiguousarray(fwd, F)
    h, w = fwd.shape[:2]
    cov = covered_of(fwd)
    sx = np.where(cov, scan_q8(fwd[..., 0], axis_scale(ws, w), ws), 0)
    sy = np.where(cov, scan_q8(fwd[..., 1], axis_scale(hs, h), hs), 0)
    return sx, sy, cov


def _shift(a, dy, dx, fill):
    """a[y + dy, x + dx], `fill` off the image."""
    h, w = a.shape
    out = np.full_like(a, fill)
    ys, xs = slice(max(0, -dy), h - max(0, dy)), slice(max(0, -dx), w - max(0, dx))
    yt, xt = slice(max(0, dy), h - max(0, -dy)), slice(max(0, dx), w - max(0, -dx))
    out[ys, xs] = a[yt, xt]
    return out


def _diff2(s, cov, axis):
    """Twice the derivative of s along an axis from the covered neighbours: the central difference where both are covered, the
    doubled one-sided difference where one is, else 0.  Off the image counts as uncovered."""
    d = (0, 1) if axis == 1 else (1, 0)
    lo, hi = _shift(s, -d[0], -d[1], 0), _shift(s, d[0], d[1], 0)
    has_lo, has_hi = _shift(cov, -d[0], -d[1], False), _shift(cov, d[0], d[1], False)
    return np.where(has_lo & has_hi, hi - lo, np.where(has_hi, 2 * (hi - s), np.where(has_lo, 2 * (s - lo), 0)))


def radius_of(a, b):
    """The larger derivative in scan pixels to the nearest integer, a half rounding down, in 1..8: a and b are doubled Q8
    derivatives (512 per scan pixel), so this is ceil(d - 1/2) of d = max(|a|, |b|) / 512."""
    return np.clip((np.maximum(np.abs(a), np.abs(b)) + 255) >> 9, 1, MAX_RADIUS)


def footprint(fwd, hs, ws, detail=False):
    """[h,w,2] uint8: the tent's radii (rx, ry) at every covered pixel, 0 elsewhere.  detail=True: also the doubled derivatives
    (xx, xy, yx, yy) = 2 (dsx/dpx, dsx/dpy, dsy/dpx, dsy/dpy), the positions and the coverage."""
    sx, sy, cov = scan_positions(fwd, hs, ws)
    xx, xy, yx, yy = _diff2(sx, cov, 1), _diff2(sx, cov, 0), _diff2(sy, cov, 1), _diff2(sy, cov, 0)
    rx, ry = radius_of(xx, xy), radius_of(yx, yy)
    out = np.where(cov[..., None], np.stack([rx, ry], axis=-1), 0).astype(np.uint8)
    return (out, (xx, xy, yx, yy), (sx, sy, cov)) if detail else out


def tent_taps(s, r, n):
    """(columns clamped to 0..n-1, weights), each [..., 2 r]: the integer columns floor(s / 256) - r + 1 .. floor(s / 256) + r the
    tent of half-width r around the Q8 position s touches, weight 256 r - |256 c - s|."""
    c = (np.asarray(s, I) >> 8)[..., None] - r + 1 + np.arange(2 * r, dtype=I)
    wgt = 256 * r - np.abs(256 * c - np.asarray(s, I)[..., None])
    return np.clip(c, 0, n - 1), wgt


def sample(scan, sx, sy, rx, ry):
    """The separable integer tent at the pixels listed: sx, sy, rx, ry [n] -> [n,3] int64, (sum w texel + W / 2) // W with
    W = 65536 rx^2 ry^2, the exact weight sum."""
    scan = np.asarray(scan, np.uint8)
    hs, ws = scan.shape[:2]
    out = np.zeros((len(sx), 3), I)
    for a in np.unique(rx):
        for b in np.unique(ry):
            m = np.nonzero((rx == a) & (ry == b))[0]
            if not len(m):
                continue
            cols, wx = tent_taps(sx[m], int(a), ws)
            rows, wy = tent_taps(sy[m], int(b), hs)
            tex = scan[rows[:, :, None], cols[:, None, :]].astype(I)                  # [n, 2b, 2a, 3]
            acc = (tex * (wy[:, :, None] * wx[:, None, :])[..., None]).sum(axis=(1, 2))
            W = 65536 * int(a) ** 2 * int(b) ** 2
            out[m] = (acc + W // 2) // W
    return out


def shade_q16(prm, h, w, det2):
    """Lq [h,w] int64 = clamp(rint(65536 L), 0, 131072); det2 = xx yy - xy yx of the doubled derivatives (4 x the Q8 area)."""
    p = {k: F(v) for k, v in prm.items()}
    px, py = np.arange(w, dtype=F)[None, :], np.arange(h, dtype=F)[:, None]
    with np.errstate(all="ignore"):
        tx = ((px / F(w - 1)).astype(F) if w > 1 else np.zeros_like(px)) - F(0.5)
        ty = ((py / F(h - 1)).astype(F) if h > 1 else np.zeros_like(py)) - F(0.5)
        area = (np.abs(det2).astype(np.float64).astype(F) * F(2.0 ** -18)).astype(F)
        L = (p["l0"] + (p["lgx"] * tx).astype(F)).astype(F)
        L = (L + (p["lgy"] * ty).astype(F)).astype(F)
        L = (L + (p["k"] * ((area / p["a_ref"]).astype(F) - F(1)).astype(F)).astype(F)).astype(F)
        t = (L * F(65536)).astype(F)
        return np.rint(np.where(t >= 0, np.minimum(t, F(131072)), F(0))).astype(I)


def shading_on(prm):
    return any(F(prm[k]) != 0 for k in ("l0", "lgx", "lgy", "k"))


def render(scan, fwd, background=(255, 255, 255), shading=None):
    """The photograph [h,w,3] uint8.  background: an RGB triple or [h,w,3] uint8.  shading: None or a dict l0, lgx, lgy, k,
    a_ref (all of the first four zero: none)."""
    scan = np.asarray(scan, np.uint8)
    hs, ws = scan.shape[:2]
    fwd = np.ascontiguousarray(fwd, F)
    h, w = fwd.shape[:2]
    radii, (xx, xy, yx, yy), (sx, sy, cov) = footprint(fwd, hs, ws, detail=True)
    bg = np.broadcast_to(np.asarray(background, np.uint8), (h, w, 3)).astype(I)
    out = bg.copy()
    m = np.nonzero(cov)
    if len(m[0]):
        page = sample(scan, sx[m], sy[m], radii[..., 0][m].astype(I), radii[..., 1][m].astype(I))
        if shading is not None and shading_on(shading):
            lq = shade_q16(shading, h, w, xx * yy - xy * yx)[m]
            page = np.minimum(255, (page * lq[:, None] + 32768) >> 16)
        n = sum(_shift(cov, dy, dx, False).astype(I) for dy in (-1, 0, 1) for dx in (-1, 0, 1))[m]
        out[m] = (page * n[:, None] + bg[m] * (9 - n)[:, None] + 4) // 9
    return out.astype(np.uint8)
