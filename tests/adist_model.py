"""Integer NumPy model of the project's aligned distortion on top of tests/sflow_model.py: the yardstick of
tests/test_adist_cpu.py and tests/test_gpu_adist.py.  Written from the definition: the least-squares fit of a translation and a
scale per axis to a flow field (exact integer sums, four Q16 coefficients), the fixed-point bilinear resampling of the page
through that fit, the gradient-magnitude weights of the scan, and AD.  Only `ad_sum` follows the kernels: it adds the terms in
their fixed order, as sflow_model.ld_sum does, so that a CPU restatement of them can be held to the model bit for bit."""
import numpy as np

import sflow_model as M

Q31 = (1 << 31) - 1


def _q16(num, den):
    """rint(num / den * 65536) in float64 (one correctly rounded division, ties to even), 0 for den == 0, saturated"""
    if den == 0:
        return 0
    q = np.rint(np.float64(int(num)) / np.float64(int(den)) * np.float64(65536.0))
    return int(min(max(q, -float(Q31)), float(Q31)))


def fit(flow):
    """flow [2,h,w] integers -> (sums int64 [4] = (Su, Sxu, Sv, Syv), coef int32 [4] = (ax, bx, ay, by) in Q16)"""
    fu, fv = (np.asarray(flow[k]).astype(np.int64) for k in (0, 1))
    h, w = fu.shape
    X = 2 * np.arange(w, dtype=np.int64) - (w - 1)
    Y = 2 * np.arange(h, dtype=np.int64) - (h - 1)
    su, sxu, sv, syv = int(fu.sum()), int((fu * X[None, :]).sum()), int(fv.sum()), int((fv * Y[:, None]).sum())
    n, sxx, syy = h * w, h * w * (w * w - 1) // 3, w * h * (h * h - 1) // 3
    assert 3 * sxx == h * w * (w * w - 1) and sxx == h * int((X * X).sum()) and syy == w * int((Y * Y).sum())
    coef = [_q16(su, n), _q16(2 * sxu, sxx), _q16(sv, n), _q16(2 * syv, syy)]
    return np.array([su, sxu, sv, syv], np.int64), np.array(coef, np.int32)


def _fitted(n, a, b):
    """the fitted Q16 position of every coordinate of an axis of n pixels (Python integers: no width to overflow)"""
    return [min(max((x << 16) + int(a) + ((int(b) * (2 * x - (n - 1))) >> 1), 0), (n - 1) << 16) for x in range(n)]


def align(b, coef):
    """B' [h,w] int64: B (integers 0..255) at the fitted position, bilinear with 8-bit fractions"""
    b = np.clip(np.asarray(b).astype(np.int64), 0, 255)
    h, w = b.shape
    cx, cy = np.array(_fitted(w, coef[0], coef[1]), np.int64), np.array(_fitted(h, coef[2], coef[3]), np.int64)
    x0, y0, fx, fy = cx >> 16, cy >> 16, ((cx >> 8) & 255)[None, :], ((cy >> 8) & 255)[:, None]
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    acc = ((256 - fx) * (256 - fy) * b[y0][:, x0] + fx * (256 - fy) * b[y0][:, x1]
           + (256 - fx) * fy * b[y1][:, x0] + fx * fy * b[y1][:, x1])
    return (acc + 32768) >> 16


def weights(a):
    """g [h,w] int64 = floor(sqrt(gx^2 + gy^2)) of the clamped central differences of A; at most 360"""
    a = np.asarray(a).astype(np.int64)
    h, w = a.shape
    ys, xs = np.arange(h), np.arange(w)
    gx = a[:, M._cl(xs + 1, w)] - a[:, M._cl(xs - 1, w)]
    gy = a[M._cl(ys + 1, h)] - a[M._cl(ys - 1, h)]
    return M.isqrt(gx * gx + gy * gy)


def _ordered(v):
    """the sum of a flat float64 array in the kernels' order (sflow_model.ld_sum's, without the division)"""
    hw = v.size
    blocks = -(-hw // 256)
    p = np.zeros(blocks * 256, np.float64)
    p[:hw] = v
    p = p.reshape(blocks * 4, 64)
    for s in (32, 16, 8, 4, 2, 1):
        p = p[:, :s] + p[:, s:2 * s]
    wv = p.reshape(blocks, 4)
    partials = ((wv[:, 0] + wv[:, 1]) + wv[:, 2]) + wv[:, 3]
    red = np.zeros(256, np.float64)
    for t in range(min(256, blocks)):
        a = np.float64(0.0)
        for x in partials[t::256]:
            a += x
        red[t] = a
    for s in (128, 64, 32, 16, 8, 4, 2, 1):
        red = red[:s] + red[s:2 * s]
    return red[0]


def ad_sum(g, flow):
    """AD from the weights g [h,w] and a flow [2,h,w]: sum g |f| / sum g, the numerator in the kernels' order, the denominator an
    exact integer; the plain mean of |f| (the LD of that flow, bit for bit) when sum g = 0."""
    fu, fv = flow[0].astype(np.int64).ravel(), flow[1].astype(np.int64).ravel()
    length = np.sqrt((fu * fu + fv * fv).astype(np.float64))
    gs = int(np.asarray(g).astype(np.int64).sum())
    if gs == 0:
        return float(_ordered(length) / np.float64(fu.size))
    return float(_ordered(np.asarray(g).astype(np.float64).ravel() * length) / np.float64(gs))


def aligned_distortion(a, b, **kw):
    """a (the scan), b (the prediction): [h,w] integers 0..255 -> dict(ad, ld, ld2, flow1, sums, coef, aligned, flow2)"""
    flow1, ld = M.sift_flow(a, b, **kw)
    sums, coef = fit(flow1)
    bp = align(b, coef)
    flow2, ld2 = M.sift_flow(a, bp, **kw)
    return dict(ad=ad_sum(weights(a), flow2), ld=ld, ld2=ld2, flow1=flow1, sums=sums, coef=coef, aligned=bp, flow2=flow2)


# ---- inputs (deterministic) ---------------------------------------------------------------------------------------------------
def scaled(img, sx, sy, su=0.0, sv=0.0):
    """B(q) = A(c + (q - c - s) / scale) about the centre c, s = (su, sv) in (x, y): float bilinear with clamped indices,
    rounded to integers.  The flow from A to B is about (scale - 1)(p - c) + s."""
    img = np.asarray(img).astype(np.float64)
    h, w = img.shape
    px = np.clip((w - 1) / 2 + (np.arange(w) - (w - 1) / 2 - su) / sx, 0, w - 1)
    py = np.clip((h - 1) / 2 + (np.arange(h) - (h - 1) / 2 - sv) / sy, 0, h - 1)
    x0, y0 = np.floor(px).astype(int), np.floor(py).astype(int)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    fx, fy = (px - x0)[None, :], (py - y0)[:, None]
    out = ((1 - fx) * (1 - fy) * img[y0][:, x0] + fx * (1 - fy) * img[y0][:, x1]
           + (1 - fx) * fy * img[y1][:, x0] + fx * fy * img[y1][:, x1])
    return np.clip(np.rint(out), 0, 255).astype(np.int64)
