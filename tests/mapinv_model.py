"""The map inverse in NumPy: THE DEFINITION.  dvd_amd/csrc/mapinv_core.h is the same arithmetic for the kernels
of mapinv.hip and for the stand-alone CPU restatement mapinv_host_check.cpp.

The network predicts a backward map: page pixel -> photograph position (what grid_sample consumes).  Here that map is turned
round by rasterising the page's triangle mesh on the photograph: vertices in Q8 integers, exact int64 edge functions, the
top-left rule, the smallest triangle id wins.  Every float32 line below is one separately rounded operation of the kernels."""
import numpy as np

import flowviz_model as FV

F = np.float32
I = np.int64
INVALID = np.uint32(0xffffffff)
COORD_CAP = F(4194304.0)          # 2^22: a vertex further out is invalid (its Q8 integer stays below 2^31)
MAX_SIDE = 16384
BLOCK, PER = 256, 4               # the cycle reduction: threads of a workgroup, pixels of a thread


def budget(step):
    """The most pixels a triangle's clipped bounding box may hold."""
    return max(1024, 64 * step * step)


# ---- the backward map at page pixels ------------------------------------------------------------------------------------------
def grid(flow, h, w, scale=0.987):
    """[2,g,g] -> (gx, gy) [h,w] float32: flow_grid_at of dvd_amd/csrc/flowgrid_core.h = ops.unwarp_grid, to the bit."""
    with np.errstate(all="ignore"):
        s = FV.upsample(np.asarray(flow, F), h, w)
    k = (np.arange(512, dtype=F) / F(511)).astype(F)
    base = np.stack([np.broadcast_to(k[None, :], (512, 512)), np.broadcast_to(k[:, None], (512, 512))]).astype(F)
    b = FV.upsample(base, h, w)
    with np.errstate(all="ignore"):
        gx = (((((s[0] + b[0]) * F(1)) * F(2)) - F(1)) * F(scale)).astype(F)
        gy = (((((s[1] + b[1]) * F(1)) * F(2)) - F(1)) * F(scale)).astype(F)
    return gx, gy


def positions(flow, h, w, scale=0.987):
    """(x, y) [h,w] float32: the photograph position the unwarp tail samples for every page pixel, un-normalised as
    grid_sample(align_corners=True) does: ((g + 1) / 2) (size - 1)."""
    gx, gy = grid(flow, h, w, scale)
    with np.errstate(all="ignore"):
        return (((gx + F(1)) * F(0.5)) * F(w - 1)).astype(F), (((gy + F(1)) * F(0.5)) * F(h - 1)).astype(F)


def lattice_axis(n, step):
    """0, step, 2 step, .. and n - 1 appended when it is no multiple of step."""
    v = list(range(0, n, step))
    if (n - 1) % step:
        v.append(n - 1)
    return np.asarray(v, I)


def quantise(x, y):
    """(qx, qy int64, valid): rint(256 x); a vertex that is not finite or beyond 2^22 in a coordinate is invalid (q = 0)."""
    with np.errstate(all="ignore"):
        ok = np.isfinite(x) & np.isfinite(y) & (np.abs(x) <= COORD_CAP) & (np.abs(y) <= COORD_CAP)
        qx = np.rint(np.where(ok, x, F(0)) * F(256)).astype(I)
        qy = np.rint(np.where(ok, y, F(0)) * F(256)).astype(I)
    return qx, qy, ok


def lattice(flow, h, w, step=8, scale=0.987, pos=None):
    """dict: rows, cols (page pixels of the lattice), qx, qy [R,C] int64, valid [R,C]."""
    x, y = positions(flow, h, w, scale) if pos is None else pos
    rows, cols = lattice_axis(h, step), lattice_axis(w, step)
    qx, qy, ok = quantise(x[rows][:, cols], y[rows][:, cols])
    return {"rows": rows, "cols": cols, "qx": qx, "qy": qy, "valid": ok}


# ---- triangles ------------------------------------------------------------------------------------------------------------------
def edge(ax, ay, bx, by, px, py):
    return (bx - ax) * (py - ay) - (by - ay) * (px - ax)


def top_left(ax, ay, bx, by):
    """Whether a pixel exactly on the edge a -> b belongs to the triangle (positive area, y down): the edge runs upward, or it
    is horizontal and runs to the right."""
    return (by < ay) | ((by == ay) & (bx > ax))


def triangles(lat, h, w, step):
    """Every triangle of the mesh in id order: vx, vy [T,3] int64 (after the swap of a flipped one), pu, pv [T,3] the page pixels
    of its vertices, area [T] (positive where it is rasterised), kind [T]: 0 rasterised, 1 flipped and rasterised, 2 degenerate,
    3 skipped; box [T,4] = xmin, xmax, ymin, ymax clipped (empty when xmin > xmax or ymin > ymax)."""
    R, C = len(lat["rows"]), len(lat["cols"])
    r, c = np.meshgrid(np.arange(R - 1), np.arange(C - 1), indexing="ij")
    r, c = r.reshape(-1), c.reshape(-1)
    corners = {"a": (r, c), "b": (r, c + 1), "c": (r + 1, c), "d": (r + 1, c + 1)}

    def gather(names):
        rr = np.stack([corners[n][0] for n in names], axis=1)
        cc = np.stack([corners[n][1] for n in names], axis=1)
        return rr, cc
    r0, c0 = gather("abc")
    r1, c1 = gather("cbd")
    rr = np.stack([r0, r1], axis=1).reshape(-1, 3)            # triangle id = 2 cell + {0, 1}
    cc = np.stack([c0, c1], axis=1).reshape(-1, 3)
    vx, vy, ok = lat["qx"][rr, cc], lat["qy"][rr, cc], lat["valid"][rr, cc].all(axis=1)
    pu, pv = lat["cols"][cc], lat["rows"][rr]
    area = edge(vx[:, 0], vy[:, 0], vx[:, 1], vy[:, 1], vx[:, 2], vy[:, 2])
    flip = ok & (area < 0)
    for arr in (vx, vy, pu, pv):
        arr[flip] = arr[flip][:, [0, 2, 1]]
    area = np.where(flip, -area, area)
    xmin = np.clip((vx.min(axis=1) + 255) >> 8, 0, None)
    xmax = np.clip(vx.max(axis=1) >> 8, None, w - 1)
    ymin = np.clip((vy.min(axis=1) + 255) >> 8, 0, None)
    ymax = np.clip(vy.max(axis=1) >> 8, None, h - 1)
    held = np.clip(xmax - xmin + 1, 0, None) * np.clip(ymax - ymin + 1, 0, None)
    kind = np.where(~ok, 3, np.where(area == 0, 2, np.where(held > budget(step), 3, np.where(flip, 1, 0))))
    return {"vx": vx, "vy": vy, "pu": pu, "pv": pv, "area": area, "kind": kind, "box": np.stack([xmin, xmax, ymin, ymax], axis=1)}


def covers(t, k, px, py):
    """Whether triangle k of `t` covers the pixels (px, py) (arrays), and its three edge values there."""
    vx, vy = t["vx"][k], t["vy"][k]
    X, Y = px * 256, py * 256
    inside, es = np.ones(np.broadcast(px, py).shape, bool), []
    for i, j in ((0, 1), (1, 2), (2, 0)):
        e = edge(vx[..., i], vy[..., i], vx[..., j], vy[..., j], X, Y)
        inside &= (e > 0) | ((e == 0) & top_left(vx[..., i], vy[..., i], vx[..., j], vy[..., j]))
        es.append(e)
    return inside, es


def rasterise(t, h, w, small=16):
    """(winner [h,w] uint32, count [h,w] int64): the smallest covering triangle id and how many triangles cover each pixel."""
    win = np.full(h * w, INVALID, np.uint32)
    cnt = np.zeros(h * w, I)
    live = np.flatnonzero(t["kind"] <= 1)
    box = t["box"][live]
    bw, bh = box[:, 1] - box[:, 0] + 1, box[:, 3] - box[:, 2] + 1
    keep = (bw > 0) & (bh > 0)
    live, box, bw, bh = live[keep], box[keep], bw[keep], bh[keep]
    quick = (bw <= small) & (bh <= small)
    ids, bx = live[quick], box[quick]
    if len(ids):
        for dy in range(int(bh[quick].max())):
            for dx in range(int(bw[quick].max())):
                px, py = bx[:, 0] + dx, bx[:, 2] + dy
                m = (px <= bx[:, 1]) & (py <= bx[:, 3])
                inside, _ = covers(t, ids[m], px[m], py[m])
                at = (py[m] * w + px[m])[inside]
                np.minimum.at(win, at, ids[m][inside].astype(np.uint32))
                np.add.at(cnt, at, 1)
    for k, b in zip(live[~quick], box[~quick]):
        py, px = np.meshgrid(np.arange(b[2], b[3] + 1), np.arange(b[0], b[1] + 1), indexing="ij")
        inside, _ = covers(t, k, px, py)
        at = (py * w + px)[inside]
        np.minimum.at(win, at, np.uint32(k))
        np.add.at(cnt, at, 1)
    return win.reshape(h, w), cnt.reshape(h, w)


def resolve(t, win):
    """fwd [h,w,2] float32 (the bit pattern 0xffffffff in both components of an uncovered pixel): the page position (u, v) of
    every covered photograph pixel, interpolated barycentrically over the winner from its exact edge values:
    wb = f32(E_ca) / f32(area), wc = f32(E_ab) / f32(area), u = f32(ua) + (wb f32(ub - ua) + wc f32(uc - ua))."""
    h, w = win.shape
    out = np.full((h, w, 2), INVALID, np.uint32)
    py, px = np.nonzero(win != INVALID)
    k = win[py, px].astype(I)
    _, (e_ab, _, e_ca) = covers(t, k, px.astype(I), py.astype(I))
    area = t["area"][k].astype(F)
    wb, wc = (e_ca.astype(F) / area).astype(F), (e_ab.astype(F) / area).astype(F)
    for ch, p in enumerate((t["pu"][k], t["pv"][k])):
        d = ((wb * (p[:, 1] - p[:, 0]).astype(F)).astype(F) + (wc * (p[:, 2] - p[:, 0]).astype(F)).astype(F)).astype(F)
        out[py, px, ch] = (p[:, 0].astype(F) + d).astype(F).view(np.uint32)
    return out.view(F)


def invert(flow, h, w, step=8, scale=0.987, detail=False):
    """-> (fwd [h,w,2] float32, stats); with detail also (lattice, triangles, winner, count)."""
    lat = lattice(flow, h, w, step, scale)
    t = triangles(lat, h, w, step)
    win, cnt = rasterise(t, h, w)
    kind = t["kind"]
    stats = {"covered": int((cnt >= 1).sum()), "fold_px": int((cnt >= 2).sum()), "flipped_tris": int((kind == 1).sum()),
             "degenerate_tris": int((kind == 2).sum()), "skipped_tris": int((kind == 3).sum()), "tris": int(len(kind))}
    fwd = resolve(t, win)
    return (fwd, stats, (lat, t, win, cnt)) if detail else (fwd, stats)


def covered_of(fwd):
    return np.asarray(fwd, F).view(np.uint32)[..., 0] != INVALID


# ---- the backward map at fractional page positions -----------------------------------------------------------------------------
def _blend(p00, p01, p10, p11, lx0, lx1, ly0, ly1):
    with np.errstate(all="ignore"):
        t0 = ((p00 * lx0).astype(F) + (p01 * lx1).astype(F)).astype(F)
        t1 = ((p10 * lx0).astype(F) + (p11 * lx1).astype(F)).astype(F)
        return ((t0 * ly0).astype(F) + (t1 * ly1).astype(F)).astype(F)


def _axis_taps(u, n):
    """u clamped to [0, n - 1]; i0 = min(int(u), n - 1), i1 = min(i0 + 1, n - 1), l1 = u - i0, l0 = 1 - l1."""
    uc = np.minimum(np.maximum(u, F(0)), F(n - 1)).astype(F)
    i0 = np.minimum(uc.astype(I), n - 1)
    i1 = np.minimum(i0 + 1, n - 1)
    l1 = (uc - i0.astype(F)).astype(F)
    return i0, i1, (F(1) - l1).astype(F), l1


def backward_at(pos, u, v):
    """The backward map at the page positions (u, v) float32 arrays: bilinear over the four surrounding page pixels' photograph
    positions pos = positions(..).  -> (x, y, ok); ok is False where u or v is not finite."""
    x, y = pos
    h, w = x.shape
    u, v = np.asarray(u, F), np.asarray(v, F)
    ok = np.isfinite(u) & np.isfinite(v)
    u, v = np.where(ok, u, F(0)), np.where(ok, v, F(0))
    j0, j1, lx0, lx1 = _axis_taps(u, w)
    i0, i1, ly0, ly1 = _axis_taps(v, h)
    return (_blend(x[i0, j0], x[i0, j1], x[i1, j0], x[i1, j1], lx0, lx1, ly0, ly1),
            _blend(y[i0, j0], y[i0, j1], y[i1, j0], y[i1, j1], lx0, lx1, ly0, ly1), ok)


def wave_sum(v):
    """block_ops.h's wave_sum over the last axis (64 lanes): v += the value 32, 16, .. 1 lanes further down; lane 0."""
    v = v.copy()
    for d in (32, 16, 8, 4, 2, 1):
        v[..., :d] = v[..., :d] + v[..., d:2 * d]
    return v[..., 0]


def ordered_sum(values):
    """The float64 sum of a flat array in the kernels' order: a workgroup of 256 threads takes 1024 consecutive elements, thread
    t the elements t, t + 256, .. in order; wave_sum; the four waves left to right; then one workgroup adds the block sums, lane
    t the blocks t, t + 256, .. in order, and a tree of strides 128 .. 1."""
    v = np.asarray(values, np.float64).reshape(-1)
    per = BLOCK * PER
    blocks = max((v.size + per - 1) // per, 1)
    v = np.concatenate([v, np.zeros(blocks * per - v.size)]).reshape(blocks, PER, BLOCK)
    acc = np.zeros((blocks, BLOCK))
    for k in range(PER):
        acc = acc + v[:, k]
    ws = wave_sum(acc.reshape(blocks, BLOCK // 64, 64))
    part = ((ws[:, 0] + ws[:, 1]) + ws[:, 2]) + ws[:, 3]
    rounds = (blocks + BLOCK - 1) // BLOCK
    part = np.concatenate([part, np.zeros(rounds * BLOCK - blocks)]).reshape(rounds, BLOCK)
    lane = np.zeros(BLOCK)
    for r in range(rounds):
        lane = lane + part[r]
    st = BLOCK // 2
    while st >= 1:
        lane[:st] = lane[:st] + lane[st:2 * st]
        st //= 2
    return float(lane[0])


def cycle_error(flow, fwd, scale=0.987, pos=None):
    """At every covered pixel p: |backward(fwd(p)) - p| in float32.  -> dict cycle_mean (the ordered float64 sum over the count),
    cycle_max, n (the covered pixels whose distance is finite), dist [h,w] float32 (0 elsewhere)."""
    fwd = np.asarray(fwd, F)
    h, w = fwd.shape[:2]
    pos = positions(flow, h, w, scale) if pos is None else pos
    cov = covered_of(fwd)
    x, y, _ = backward_at(pos, np.where(cov, fwd[..., 0], F(0)), np.where(cov, fwd[..., 1], F(0)))
    py, px = np.meshgrid(np.arange(h, dtype=F), np.arange(w, dtype=F), indexing="ij")
    with np.errstate(all="ignore"):
        dx, dy = (x - px).astype(F), (y - py).astype(F)
        d = np.sqrt(((dx * dx).astype(F) + (dy * dy).astype(F)).astype(F)).astype(F)
    ok = cov & np.isfinite(d)
    d = np.where(ok, d, F(0))
    n = int(ok.sum())
    total = ordered_sum(d)
    return {"cycle_mean": total / n if n else float("nan"), "cycle_max": float(d.max()) if n else float("nan"), "n": n, "sum": total,
            "dist": d}


# ---- the mesh picture ---------------------------------------------------------------------------------------------------------
def mesh_overlay(src, fwd, lines=17, thickness=1, color=(255, 0, 0), outline_color=(0, 255, 0), dim=False):
    """src [h,w,3] uint8, fwd [h,w,2] -> the photograph with the page's grid lines and outline drawn on it."""
    src, fwd = np.asarray(src, np.uint8), np.asarray(fwd, F)
    h, w = fwd.shape[:2]
    cov = covered_of(fwd)
    with np.errstate(all="ignore"):
        u, v = np.where(cov, fwd[..., 0], F(0)), np.where(cov, fwd[..., 1], F(0))
        ku = np.floor(((u * F(lines - 1)).astype(F) / F(max(w - 1, 1))).astype(F)).astype(np.int32)
        kv = np.floor(((v * F(lines - 1)).astype(F) / F(max(h - 1, 1))).astype(F)).astype(np.int32)
    line = np.zeros((h, w), bool)
    differs_r = cov[:, :-1] & cov[:, 1:] & ((ku[:, :-1] != ku[:, 1:]) | (kv[:, :-1] != kv[:, 1:]))
    differs_d = cov[:-1] & cov[1:] & ((ku[:-1] != ku[1:]) | (kv[:-1] != kv[1:]))
    line[:, :-1] |= differs_r
    line[:-1] |= differs_d
    pad = np.pad(cov, 1, constant_values=False)
    edge_px = cov & ~(pad[:-2, 1:-1] & pad[2:, 1:-1] & pad[1:-1, :-2] & pad[1:-1, 2:])

    def widen(m):
        lo, hi = (thickness - 1) // 2, thickness // 2           # the window of p: rows and columns p - lo .. p + hi
        p = np.pad(m, ((lo, hi), (lo, hi)), constant_values=False)
        out = np.zeros_like(m)
        for dy in range(thickness):
            for dx in range(thickness):
                out |= p[dy:dy + h, dx:dx + w]
        return out
    line, edge_px = widen(line), widen(edge_px)
    out = src.copy()
    if dim:
        out[~cov] >>= 1
    out[line] = np.asarray(color, np.uint8)
    out[edge_px] = np.asarray(outline_color, np.uint8)
    return out


# ---- points -------------------------------------------------------------------------------------------------------------------
def transfer_points(fwd, pts):
    """Photograph positions [N,2] float32 (x, y) -> page positions [N,2] float32 (u, v): fwd sampled bilinearly; the bit pattern
    0xffffffff in both components where the point is outside the photograph, not finite, or a tap is uncovered."""
    fwd, pts = np.asarray(fwd, F), np.asarray(pts, F).reshape(-1, 2)
    h, w = fwd.shape[:2]
    x, y = pts[:, 0], pts[:, 1]
    with np.errstate(all="ignore"):
        ok = (x >= 0) & (x <= F(w - 1)) & (y >= 0) & (y <= F(h - 1))
    x, y = np.where(ok, x, F(0)), np.where(ok, y, F(0))
    j0, j1, lx0, lx1 = _axis_taps(x, w)
    i0, i1, ly0, ly1 = _axis_taps(y, h)
    cov = covered_of(fwd)
    ok &= cov[i0, j0] & cov[i0, j1] & cov[i1, j0] & cov[i1, j1]
    out = np.full((len(pts), 2), INVALID, np.uint32)
    for ch in range(2):
        p = fwd[..., ch]
        val = _blend(p[i0, j0], p[i0, j1], p[i1, j0], p[i1, j1], lx0, lx1, ly0, ly1)
        out[:, ch] = np.where(ok, val.view(np.uint32), INVALID)
    return out.view(F)


def map_points(flow, pts, h, w, scale=0.987, pos=None):
    """Page positions [N,2] float32 (u, v) -> photograph positions [N,2] (x, y) through backward_at; a position outside the page
    is clamped to it; 0xffffffff where a component is not finite."""
    pts = np.asarray(pts, F).reshape(-1, 2)
    pos = positions(flow, h, w, scale) if pos is None else pos
    x, y, ok = backward_at(pos, pts[:, 0], pts[:, 1])
    out = np.stack([x, y], axis=1).astype(F).view(np.uint32)
    out[~ok] = INVALID
    return out.view(F)


def inverse_displacement(fwd, unknown=1e10):
    """[h,w,2] float32: fwd(p) - p, `unknown` (the .flo format's own value) at an uncovered pixel."""
    fwd = np.asarray(fwd, F)
    h, w = fwd.shape[:2]
    cov = covered_of(fwd)
    py, px = np.meshgrid(np.arange(h, dtype=F), np.arange(w, dtype=F), indexing="ij")
    with np.errstate(all="ignore"):
        d = np.stack([fwd[..., 0] - px, fwd[..., 1] - py], axis=-1).astype(F)
    d[~cov] = F(unknown)
    return d
