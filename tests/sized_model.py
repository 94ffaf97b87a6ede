"""Pages at a chosen size in NumPy: THE DEFINITION.  dvd_amd/csrc/sized_core.h is the same arithmetic for the
kernels of sized.hip and for the stand-alone CPU restatement sized_host_check.cpp.

A photograph [H,W,3] u8 is unwarped through the coarse map flow [2,G,G] to a page of (hp, wp): the unwarp tail's own sampling
grid at the page's size (mapinv_model.grid = flow_grid_at) gives every page pixel a Q8 position on the photograph; the first
differences of those positions give integer radii; the photograph is filtered with synth_model's separable integer tent of that
half-width, a tap outside the photograph contributing zero.  Every float32 line below is one separately rounded operation of
the kernels; everything behind the Q8 position is integer.  The page is ROUNDED, not truncated as the native u8 tail is."""
import numpy as np

import mapinv_model as MI
import synth_model as Y

F = np.float32
I = np.int64
MAX_SIDE, MAX_RADIUS, MIN_GRID, MAX_GRID = 16384, 16, 2, 8192
PAD = 17                              # a position further than this many pixels outside the photograph is moved there
STATS = ("capped", "outside", "invalid")


def q8_of(g, n, valid):
    """floor(256 x + 1/2) of x = (g + 1) ((n - 1) / 2), clamped to [-256 PAD, 256 (n - 1 + PAD)]; 0 where not valid."""
    with np.errstate(all="ignore"):
        x = ((g + F(1)).astype(F) * F(F(n - 1) * F(0.5))).astype(F)
        t = np.floor(((x * F(256)).astype(F) + F(0.5)).astype(F))
        lo, hi = F(-256 * PAD), F(256 * (n - 1 + PAD))
        t = np.where(t >= lo, np.minimum(t, hi), lo)
    return np.where(valid, t, F(0)).astype(I)


def positions(flow, src_hw, size, scale=0.987):
    """(qx, qy int64 [hp,wp], valid [hp,wp]): the signed Q8 position on the photograph of every page pixel (0 where the grid
    value is not finite)."""
    (H, W), (hp, wp) = src_hw, size
    gx, gy = MI.grid(flow, hp, wp, scale)
    valid = np.isfinite(gx) & np.isfinite(gy)
    return q8_of(gx, W, valid), q8_of(gy, H, valid), valid


def radius_raw(a, b):
    """synth_model.radius_of without its cap: the larger doubled Q8 derivative in photograph pixels, a half rounding down."""
    return np.maximum((np.maximum(np.abs(a), np.abs(b)) + 255) >> 9, 1)


def footprint(flow, src_hw, size, scale=0.987, max_radius=MAX_RADIUS, detail=False):
    """[hp,wp] uint16: rx | ry << 8 at every valid page pixel, 0 at an invalid one.  detail=True: (rx, ry, ux, uy, qx, qy,
    valid) - the radii, their uncapped values and the positions."""
    qx, qy, valid = positions(flow, src_hw, size, scale)
    ux = radius_raw(Y._diff2(qx, valid, 1), Y._diff2(qx, valid, 0))
    uy = radius_raw(Y._diff2(qy, valid, 1), Y._diff2(qy, valid, 0))
    rx, ry = np.minimum(ux, max_radius), np.minimum(uy, max_radius)
    if detail:
        return rx, ry, ux, uy, qx, qy, valid
    return np.where(valid, rx | ry << 8, 0).astype(np.uint16)


def tent_taps(s, r, n):
    """(columns, weights, inside), each [..., 2 r]: the columns floor(s / 256) - r + 1 .. floor(s / 256) + r, their weights
    256 r - |256 c - s| and whether the column is one of the photograph's."""
    c = (np.asarray(s, I) >> 8)[..., None] - r + 1 + np.arange(2 * r, dtype=I)
    wgt = 256 * r - np.abs(256 * c - np.asarray(s, I)[..., None])
    return c, wgt, (c >= 0) & (c < n)


def sample(src, sx, sy, rx, ry, chunk=2048):
    """The separable integer tent at the pixels listed -> [n,3] int64: (sum w texel + W / 2) // W with W = 65536 rx^2 ry^2,
    the weight sum of ALL taps; a tap outside the photograph contributes zero."""
    src = np.asarray(src, np.uint8)
    H, W = src.shape[:2]
    out = np.zeros((len(sx), 3), I)
    for a in np.unique(rx):
        for b in np.unique(ry):
            group = np.nonzero((rx == a) & (ry == b))[0]
            for k in range(0, len(group), chunk):
                m = group[k:k + chunk]
                cols, wx, okx = tent_taps(sx[m], int(a), W)
                rows, wy, oky = tent_taps(sy[m], int(b), H)
                wx, wy = wx * okx, wy * oky
                tex = src[np.clip(rows, 0, H - 1)[:, :, None], np.clip(cols, 0, W - 1)[:, None, :]].astype(I)   # [n, 2b, 2a, 3]
                acc = (tex * (wy[:, :, None] * wx[:, None, :])[..., None]).sum(axis=(1, 2))
                full = 65536 * int(a) ** 2 * int(b) ** 2
                out[m] = (acc + full // 2) // full
    return out


def unwarp(flow, src, size, scale=0.987, max_radius=MAX_RADIUS):
    """(page [hp,wp,3] uint8, stats): stats = {capped, outside, invalid}, the page pixels whose uncapped radius exceeds
    max_radius, whose centre lies outside the photograph, and whose grid value is not finite (those are black)."""
    src = np.asarray(src, np.uint8)
    H, W = src.shape[:2]
    hp, wp = size
    rx, ry, ux, uy, qx, qy, valid = footprint(flow, (H, W), size, scale, max_radius, detail=True)
    out = np.zeros((hp, wp, 3), np.uint8)
    m = np.nonzero(valid)
    if len(m[0]):
        out[m] = sample(src, qx[m], qy[m], rx[m], ry[m])
    outside = valid & ((qx < 0) | (qx > 256 * (W - 1)) | (qy < 0) | (qy > 256 * (H - 1)))
    stats = {"capped": int((valid & ((ux > max_radius) | (uy > max_radius))).sum()), "outside": int(outside.sum()),
             "invalid": int((~valid).sum())}
    return out, stats


# ---- the float64 statement the model is measured against ---------------------------------------------------------------------
def positions64(flow, src_hw, size, scale=0.987):
    """(x, y) float64 [hp,wp]: the same positions from exact rational coordinates, never quantised."""
    import flowviz_model as FV
    (H, W), (hp, wp) = src_hw, size
    s = FV.upsample64(flow, hp, wp)
    bx = (np.arange(wp, dtype=np.float64) / max(wp - 1, 1))[None, :]
    by = (np.arange(hp, dtype=np.float64) / max(hp - 1, 1))[:, None]
    gx, gy = ((s[0] + bx) * 2 - 1) * scale, ((s[1] + by) * 2 - 1) * scale
    return (gx + 1) * (W - 1) / 2, (gy + 1) * (H - 1) / 2


def tent64(src, x, y, rx, ry):
    """[n,3] float64: the continuous tent of half-widths rx, ry [n] at the positions x, y [n], zeros outside the photograph."""
    src = np.asarray(src, np.float64)
    H, W = src.shape[:2]
    out = np.zeros((len(x), 3))
    for k in range(len(x)):
        a, b = int(rx[k]), int(ry[k])
        cols = int(np.floor(x[k])) - a + 1 + np.arange(2 * a)
        rows = int(np.floor(y[k])) - b + 1 + np.arange(2 * b)
        wx = np.maximum(a - np.abs(cols - x[k]), 0) * ((cols >= 0) & (cols < W))
        wy = np.maximum(b - np.abs(rows - y[k]), 0) * ((rows >= 0) & (rows < H))
        tex = src[np.clip(rows, 0, H - 1)[:, None], np.clip(cols, 0, W - 1)[None, :]]
        out[k] = (tex * (wy[:, None] * wx[None, :])[..., None]).sum(axis=(0, 1)) / (a * a * b * b)
    return out
