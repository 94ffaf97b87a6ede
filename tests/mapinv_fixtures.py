"""The maps the map-inverse tests share (tests/test_mapinv_cpu.py, tests/test_gpu_mapinv.py): the smooth fold-free family, an
affine map with its analytic inverse, a folded, a collapsed and the hostile maps; each case's model result is computed once."""
import functools

import numpy as np

import mapinv_model as M

F = np.float32
SCALE = 0.987
# (h, w, g, step, a): flow_x = a sin(2 pi y) cos(pi x) + 0.02, flow_y = a cos(pi y) sin(2 pi x) - 0.01 on a g x g grid over [0, 1]^2
SMOOTH = [(37, 29, 4, 3, 0.03), (64, 48, 9, 8, 0.03), (64, 48, 9, 4, 0.03), (64, 48, 9, 2, 0.03), (64, 48, 9, 1, 0.03),
          (96, 80, 16, 8, 0.04), (96, 80, 16, 1, 0.04)]
AFFINE = (0.03, 0.05, -0.04, -0.02, 0.03, 0.06)          # flow_x = a0 + a1 x + a2 y, flow_y = b0 + b1 x + b2 y


def smooth(g, a):
    y, x = np.meshgrid(np.linspace(0, 1, g), np.linspace(0, 1, g), indexing="ij")
    return np.stack([a * np.sin(2 * np.pi * y) * np.cos(np.pi * x) + 0.02, a * np.cos(np.pi * y) * np.sin(2 * np.pi * x) - 0.01]).astype(F)


def affine(g=9):
    a0, a1, a2, b0, b1, b2 = AFFINE
    y, x = np.meshgrid(np.linspace(0, 1, g), np.linspace(0, 1, g), indexing="ij")
    return np.stack([a0 + a1 * x + a2 * y, b0 + b1 * x + b2 * y]).astype(F)


def affine_inverse(h, w):
    """(u, v) [h,w] float64: the exact inverse of the affine backward map at every photograph pixel, and the infinity norm of
    the inverse's matrix (pixels of the page per pixel of the photograph)."""
    a0, a1, a2, b0, b1, b2 = AFFINE
    s = SCALE
    # X = (w - 1) (((a0 + (1 + a1) U + a2 V) 2 - 1) s / 2 + 1 / 2), U = u / (w - 1), V = v / (h - 1); Y likewise
    A = np.array([[s * (1 + a1), s * a2 * (w - 1) / (h - 1)], [s * b1 * (h - 1) / (w - 1), s * (1 + b2)]])
    c = np.array([(w - 1) * ((2 * a0 - 1) * s / 2 + 0.5), (h - 1) * ((2 * b0 - 1) * s / 2 + 0.5)])
    inv = np.linalg.inv(A)
    py, px = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    u = inv[0, 0] * (px - c[0]) + inv[0, 1] * (py - c[1])
    v = inv[1, 0] * (px - c[0]) + inv[1, 1] * (py - c[1])
    return u, v, float(np.abs(inv).sum(axis=1).max())


def folded():
    """The smooth 96 x 80 map with one interior grid value pushed past its neighbour: the mesh folds over itself there."""
    flow = smooth(16, 0.04)
    flow[0, 7, 7] += F(0.6)
    return flow


def collapsed(g=9):
    """The flow cancels the base grid: every page pixel samples the photograph's centre."""
    k = np.linspace(0, 1, g)
    return np.stack([np.broadcast_to(0.5 - k[None, :], (g, g)), np.broadcast_to(0.5 - k[:, None], (g, g))]).astype(F)


def hostile(kind):
    flow = smooth(9, 0.03)
    if kind == "nan":
        flow[0, 2, 3] = np.nan
    elif kind == "inf":
        flow[0, 1, 1], flow[1, 6, 5] = np.inf, -np.inf
    elif kind == "huge":
        flow[1, 4, 4] = 1e6                   # beyond 2^22 pixels: the vertices it reaches are invalid
    elif kind == "far":
        flow[:, 6, 6] -= F(30.0)              # valid vertices far beyond the upper left corner: clipped boxes above the budget
    return flow


# name -> (flow, h, w, step)
CASES = {f"smooth_{h}x{w}_g{g}_s{step}": (smooth(g, a), h, w, step) for h, w, g, step, a in SMOOTH}
CASES.update({
    "affine_s8": (affine(), 64, 48, 8), "affine_s1": (affine(), 64, 48, 1),
    "folded": (folded(), 96, 80, 4), "collapsed": (collapsed(), 64, 48, 8),
    "nan": (hostile("nan"), 64, 48, 8), "inf": (hostile("inf"), 64, 48, 4), "huge": (hostile("huge"), 64, 48, 8),
    "far": (hostile("far"), 64, 48, 4), "thin_1xN": (smooth(4, 0.03), 1, 40, 3), "one_cell": (smooth(4, 0.03), 9, 7, 16),
})
OVERLAYS = [dict(lines=17, thickness=1, dim=False), dict(lines=5, thickness=2, dim=True, color=(1, 2, 250), outline_color=(9, 200, 0)),
            dict(lines=2, thickness=3, dim=True)]


@functools.lru_cache(maxsize=None)
def model(name):
    """Everything the model says of a case, computed once: fwd, stats, detail = (lattice, triangles, winner, count), pos, cycle."""
    flow, h, w, step = CASES[name]
    fwd, stats, detail = M.invert(flow, h, w, step, SCALE, detail=True)
    pos = M.positions(flow, h, w, SCALE)
    out = {"fwd": fwd, "stats": stats, "detail": detail, "pos": pos, "cycle": M.cycle_error(flow, fwd, SCALE, pos=pos)}
    for v in (fwd, *pos):
        v.setflags(write=False)
    return out


def photograph(h, w, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def points(h, w, n=64, seed=1):
    """[n,2] float32 positions: most inside the image, some on its border, some outside, one NaN and one infinite."""
    rng = np.random.default_rng(seed)
    pts = (rng.random((n, 2)) * [w + 6, h + 6] - 3).astype(F)
    pts[0], pts[1], pts[2], pts[3] = (0, 0), (w - 1, h - 1), (np.nan, 1), (np.inf, 2)
    pts[4] = (w - 1, 0.5)
    return pts


def interior_points(h, w, n=200, seed=7, margin=0.2):
    """[n,2] float32 page positions (u, v) at least `margin` of the side away from the page's border."""
    rng = np.random.default_rng(seed)
    return (rng.random((n, 2)) * [(1 - 2 * margin) * (w - 1), (1 - 2 * margin) * (h - 1)] + [margin * (w - 1), margin * (h - 1)]).astype(F)


def round_trip_bound(pos, cycle_max):
    """How far transfer_points(fwd, map_points(flow, p)) may lie from a page position p, in pixels of the page, from the backward
    map B = pos itself and the measured cycle_max.  With k = the norm of B's inverse Jacobian, at most 1 / (least diagonal
    slope - largest off-diagonal slope) of B's first differences:
      - fwd at a photograph pixel is off by at most k cycle_max on the page (cycle_max is that error seen through B);
      - transfer_points samples fwd bilinearly between photograph pixels.  The inverse F = B^-1 has |F''| <= k^3 |B''|, and a
        bilinear tap over a unit cell is off by at most a quarter of the slope's change across it, per axis - B is piecewise
        bilinear, so its slope jumps at the coarse grid's lines.  |B''| per axis = the largest second difference of pos.
    Both are upper bounds, so their sum is one."""
    x, y = (np.asarray(p, np.float64) for p in pos)
    diag = min(np.diff(x, axis=1).min(), np.diff(y, axis=0).min())
    off = max(np.abs(np.diff(x, axis=0)).max(), np.abs(np.diff(y, axis=1)).max())
    k = 1.0 / (diag - off)
    second = sum(max(np.abs(np.diff(p, 2, axis=a)).max() for p in (x, y)) for a in (0, 1))
    return k * cycle_max + k ** 3 * second / 4
