"""Float64 model of F.grid_sample(mode='bicubic', padding_mode='zeros', align_corners=True) as include/dvd_hip.h states
it, and the error bound the bicubic tests hold the kernels to.  A helper, not a test module.

Coordinates are the kernels': ix = (gx + 1) * ((Win - 1) * 0.5) evaluated in f32 (two roundings), fx = floor(ix),
t = ix - fx (exact in f32, hence in f64).  Weights (A = -0.75) and the 16-tap sum are float64.  Zeros padding is per tap.

THE BOUND.  Every comparison is per value: |got - model| <= K * 2^-24 * S, S = the sum of |v| over the in-range taps of
that value (the weights cancel near t = 0 and t = 1, so their error is absolute: the bound is on S, not on sum |w v|).
K follows from the operation sequence of the shared device function (dvd_amd/csrc/warp.hip: cubic_axis, bicubic_sum),
u = 2^-24, every f32 operation rounding its exact result v by at most u |v|:

  weights, per axis (t in [0,1) exact, s = fl(1 - t): error <= u/2, none for t >= 1/2)
    inner, Horner:  p = fma(1.25, x, -2.25)   |p| <= 2.25             error <= 2.25 u
                    q = p * x                 |q| <= 1.02             error <= 2.25 u + 1.02 u = 3.27 u
                    c1 = fma(q, x, 1)         0 <= c1 <= 1            error <= 3.27 u + u = 4.27 u
                    c1(s) also moves by |c1'| * u/2 <= 1.35 * u/2 = 0.68 u                      -> 4.95 u
    outer, factored A x y^2 (c2(1+t) = A t (1-t)^2, c2(2-t) = A (1-t) t^2; |value| <= 1/9):
                    a = -0.75 x (error 0.75 u), b = a y (<= 0.75 u + 0.375 u + 0.19 u = 1.32 u),
                    c = b y (<= 1.32 u + 0.1 u + 0.11 u)                                          -> 1.53 u
    so every weight is within e = 5 u of its exact value, and |w| <= 1 + e.
  the sum  out = sum_i wy_i (sum_j wx_j v_ij), each level one multiply and three fused multiply-adds:
    weight errors:  sum_ij |v_ij| (|Wy_i| e + |wx_j| e) <= 2 e S (1 + e)                          = 10 u S
    row sums:       the first product passes 4 roundings, the others fewer: <= 4 u sum_j |wx_j v_ij| <= 4 u R_i,
                    carried through |wy_i| <= 1:                                                  =  4 u S
    column sum:     <= 4 u sum_i |wy_i r_i| <= 4 u S (1 + 4 u)                                    =  4 u S
  first order K = 18; the second-order terms (e^2, 16 u^2, e * 4u) are below 1e-5.  K = 20 is used.
A shifted window at the plane's border permutes the order of the same terms: the bound does not depend on the order.
"""
import numpy as np

A = -0.75
K = 20.0
U = 2.0 ** -24


def _c1(x):
    return ((A + 2.0) * x - (A + 3.0)) * x * x + 1.0


def _c2(x):
    return ((A * x - 5.0 * A) * x + 8.0 * A) * x - 4.0 * A


def unnorm_f32(g, size):
    """(g + 1) * ((size - 1) * 0.5) with every step rounded to f32, as the kernels' unnorm."""
    g = np.asarray(g, dtype=np.float32)
    return (g + np.float32(1.0)) * (np.float32(size - 1) * np.float32(0.5))


def bicubic_model(src, grid, src_batch_div=1):
    """src [Ns,C,Hin,Win], grid [N,2,H,W] f32 (channel 0 = x) -> (out [N,C,H,W] float64, S [N,C,H,W] float64).
    A non-finite grid value gives NaN there (and S = 0)."""
    src = np.asarray(src, dtype=np.float64)
    grid = np.asarray(grid, dtype=np.float32)
    n, _, h, w = grid.shape
    ns, c, hin, win = src.shape
    assert ns * src_batch_div == n
    with np.errstate(invalid="ignore", over="ignore"):
        ix = unnorm_f32(grid[:, 0], win).astype(np.float64)
        iy = unnorm_f32(grid[:, 1], hin).astype(np.float64)
    bad = ~(np.isfinite(ix) & np.isfinite(iy))
    ix = np.where(bad, 0.0, ix)
    iy = np.where(bad, 0.0, iy)
    fx, fy = np.floor(ix), np.floor(iy)
    tx, ty = ix - fx, iy - fy
    wx = [_c2(tx + 1.0), _c1(tx), _c1(1.0 - tx), _c2(2.0 - tx)]
    wy = [_c2(ty + 1.0), _c1(ty), _c1(1.0 - ty), _c2(2.0 - ty)]
    out = np.zeros((n, c, h, w))
    s_abs = np.zeros((n, c, h, w))
    bidx = (np.arange(n) // src_batch_div)[:, None, None]
    for i in range(4):
        yy = fy.astype(np.int64) - 1 + i
        yok = (yy >= 0) & (yy < hin)
        yc = np.clip(yy, 0, hin - 1)
        for j in range(4):
            xx = fx.astype(np.int64) - 1 + j
            ok = yok & (xx >= 0) & (xx < win)
            xc = np.clip(xx, 0, win - 1)
            v = src[bidx, :, yc, xc]                       # [N,H,W,C]
            v = np.where(ok[..., None], v, 0.0).transpose(0, 3, 1, 2)
            out += (wy[i] * wx[j])[:, None] * v
            s_abs += np.abs(v)
    out[np.broadcast_to(bad[:, None], out.shape)] = np.nan
    s_abs[np.broadcast_to(bad[:, None], out.shape)] = 0.0
    return out, s_abs


def bound(s_abs):
    return K * U * s_abs


def worst_k(got, model, s_abs):
    """max over the values of |got - model| / (2^-24 S) - what K would have to be; 0 where both are exactly 0."""
    err = np.abs(np.asarray(got, dtype=np.float64) - model)
    with np.errstate(invalid="ignore", divide="ignore"):
        k = np.where(err == 0.0, 0.0, err / (U * s_abs))
    return float(np.nanmax(k))


# ---- which route a tile takes: the kernels' own box arithmetic (dvd_amd/csrc/warp.hip), restated for the tests ----
LCAP_C = 3072      # floats per plane the f32 LDS kernel stages
UCAP = 2048        # dwords the u8 tail stages


def _window_base(i, size):
    """cubic_axis: first slot of the 4-wide window of coordinate i (f32 array)."""
    with np.errstate(invalid="ignore"):
        f = np.clip(np.floor(i), -3.0, size + 2.0)
    f = np.where(np.isnan(i), -3.0, f)
    return np.clip(f.astype(np.int64) - 1, 0, max(size - 4, 0))


def _tiles(grid2hw, hin, win):
    """yield (ty, tx, xmin, xmax, ymin, ymax) of every 32 x 32 output tile of one [2,H,W] grid"""
    cb = _window_base(unnorm_f32(grid2hw[0], win), win)
    rb = _window_base(unnorm_f32(grid2hw[1], hin), hin)
    h, w = cb.shape
    for ty in range(0, h, 32):
        for tx in range(0, w, 32):
            c, r = cb[ty:ty + 32, tx:tx + 32], rb[ty:ty + 32, tx:tx + 32]
            yield ty // 32, tx // 32, int(c.min()), int(np.minimum(c + 3, win - 1).max()), int(r.min()), int(np.minimum(r + 3, hin - 1).max())


def lds_tiles_staged(grid2hw, hin, win):
    """grid_sample_bicubic_lds_kernel: per tile, True if its box is staged in LDS (bh * bw <= LCAP_C floats, bw4 <= 64)."""
    out = []
    for _, _, xmin, xmax, ymin, ymax in _tiles(np.asarray(grid2hw, dtype=np.float32), hin, win):
        bw4 = ((xmax - (xmin & ~3)) >> 2) + 1
        out.append((ymax - ymin + 1) * bw4 * 4 <= LCAP_C and bw4 <= 64)
    return out


def u8_tiles_staged(grid2hw, h, w):
    """unwarp_u8_bicubic_tile: per tile, True if its byte footprint is staged (nd <= 64 dwords a row, bh * nd <= UCAP)."""
    out = []
    for _, _, xmin, xmax, ymin, ymax in _tiles(np.asarray(grid2hw, dtype=np.float32), h, w):
        nd = ((xmax - xmin + 1) * 3 + 6) >> 2
        out.append(nd <= 64 and (ymax - ymin + 1) * nd <= UCAP)
    return out
