"""Integer NumPy model of the project's local distortion: the yardstick of tests/test_sflow_cpu.py and
tests/test_gpu_sflow.py.  Written from the definition in int64, not from the kernels of dvd_amd/csrc/sflow.hip: dense SIFT
descriptors, the integer pyramid, per level the cost volume, synchronous min-sum BP with the separable min-convolution (and a
brute-force O(L^2) level kept only to show that the two agree), the argmin, and LD.  Only `ld_sum` follows the kernels: it
adds the flow lengths in their fixed order, so that a CPU restatement of them can be held to the model bit for bit."""
import numpy as np

DEFAULTS = dict(levels=4, w_top=10, w=2, iters_top=60, iters=30, alpha=510, d=10200, gamma=1, T=8160, eps=1 << 17)
FIELDS = ("levels", "w_top", "w", "iters_top", "iters", "alpha", "d", "gamma", "T", "eps")     # dvd_sflow_params, in order
C = np.array([1024, 724, 0, -724, -1024, -724, 0, 724], np.int64)
S = np.array([0, 724, 1024, 724, 0, -724, -1024, -724], np.int64)


def params(**kw):
    unknown = set(kw) - set(DEFAULTS)
    assert not unknown, unknown
    return dict(DEFAULTS, **kw)


def _cl(i, n):
    return np.clip(i, 0, n - 1)


def isqrt(s):
    """floor(sqrt(s)) of an int64 array, exactly"""
    n = np.floor(np.sqrt(s.astype(np.float64))).astype(np.int64)
    n = np.where(n * n > s, n - 1, n)
    return np.where((n + 1) * (n + 1) <= s, n + 1, n)


def dsift(img, eps=DEFAULTS["eps"]):
    """[h,w] integers 0..255 -> [h,w,128] uint8"""
    img = np.asarray(img).astype(np.int64)
    h, w = img.shape
    ys, xs = np.arange(h), np.arange(w)
    gx = img[:, _cl(xs + 1, w)] - img[:, _cl(xs - 1, w)]
    gy = img[_cl(ys + 1, h)] - img[_cl(ys - 1, h)]
    r = np.maximum(0, gx[..., None] * C + gy[..., None] * S)
    c = np.zeros_like(r)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            c += r[_cl(ys + dy, h)][:, _cl(xs + dx, w)]
    hist = np.zeros((h, w, 128), np.int64)
    for i in range(4):
        for j in range(4):
            hist[:, :, (4 * i + j) * 8:(4 * i + j) * 8 + 8] = c[_cl(ys + 3 * i - 5, h)][:, _cl(xs + 3 * j - 5, w)]
    n = isqrt((hist * hist).sum(-1))
    return np.minimum(255, (512 * hist) // (n + eps)[..., None]).astype(np.uint8)


def reduce2(img):
    """[1,4,6,4,1] x [1,4,6,4,1] centred on (2i, 2j), indices clamped, (sum + 128) >> 8; ceil(n/2) per axis"""
    img = np.asarray(img).astype(np.int64)
    h, w = img.shape
    wt = (1, 4, 6, 4, 1)
    oy, ox = np.arange((h + 1) // 2) * 2, np.arange((w + 1) // 2) * 2
    t = sum(wt[k] * img[_cl(oy + k - 2, h)] for k in range(5))
    o = sum(wt[k] * t[:, _cl(ox + k - 2, w)] for k in range(5))
    return (o + 128) >> 8


def labels(win):
    """(lu, lv) of every label index (lv + win)(2 win + 1) + (lu + win)"""
    n = 2 * win + 1
    return np.tile(np.arange(-win, win + 1), n), np.repeat(np.arange(-win, win + 1), n)


def cost_volume(da, db, off, win, gamma=DEFAULTS["gamma"], T=DEFAULTS["T"]):
    """Dc [h,w,L] int64; off = (o_u, o_v), each [h,w]"""
    h, w, _ = da.shape
    lu, lv = labels(win)
    ys, xs = np.mgrid[0:h, 0:w]
    fu, fv = off[0][..., None] + lu, off[1][..., None] + lv
    qx, qy = xs[..., None] + fu, ys[..., None] + fv
    inside = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
    dc = np.full((h, w, lu.size), T, np.int64)
    a64 = da.astype(np.int64)
    for k in range(lu.size):
        m = inside[..., k]
        dist = np.abs(a64[m] - db[qy[..., k][m], qx[..., k][m]].astype(np.int64)).sum(-1)
        dc[..., k][m] = np.minimum(T, dist)
    dc = dc + gamma * (np.abs(fu) + np.abs(fv))
    assert dc.max() <= 65535 and dc.min() >= 0, "a cost leaves 16 bits"
    return dc


def _conv_separable(hq, op, oq, win, alpha, d):
    """min over l_q of hq[l_q] + V(o_p + l_p, o_q + l_q) as a pass over u and a pass over v"""
    n = 2 * win + 1
    ar = np.arange(-win, win + 1)
    g = hq.reshape(hq.shape[:-1] + (n, n))                                      # [..., v', u']
    du = (op[0] - oq[0])[..., None, None] + ar[:, None] - ar[None, :]           # [..., u, u']
    t = (g[..., :, None, :] + np.minimum(alpha * np.abs(du), d)[..., None, :, :]).min(-1)          # [..., v', u]
    dv = (op[1] - oq[1])[..., None, None] + ar[:, None] - ar[None, :]           # [..., v, v']
    o = (t.swapaxes(-1, -2)[..., :, None, :] + np.minimum(alpha * np.abs(dv), d)[..., None, :, :]).min(-1)   # [..., u, v]
    return o.swapaxes(-1, -2).reshape(hq.shape)


def _conv_brute(hq, op, oq, win, alpha, d):
    """the same minimum over all L^2 pairs of labels"""
    lu, lv = labels(win)
    fpu, fpv = op[0][..., None] + lu, op[1][..., None] + lv
    fqu, fqv = oq[0][..., None] + lu, oq[1][..., None] + lv
    v = (np.minimum(alpha * np.abs(fpu[..., :, None] - fqu[..., None, :]), d)
         + np.minimum(alpha * np.abs(fpv[..., :, None] - fqv[..., None, :]), d))
    return (hq[..., None, :] + v).min(-1)


def propagate(dc, off, win, iters, alpha=DEFAULTS["alpha"], d=DEFAULTS["d"], conv=_conv_separable):
    """`iters` synchronous iterations from zero messages -> msg [4,h,w,L]: slot k of a pixel holds the message from its left
    (0), right (1), upper (2), lower (3) neighbour; the slot of an absent neighbour stays 0."""
    ou, ov = off
    msg = np.zeros((4,) + dc.shape, np.int64)
    for _ in range(iters):
        tot = dc + msg.sum(0)
        new = np.zeros_like(msg)
        new[0][:, 1:] = conv((tot - msg[1])[:, :-1], (ou[:, 1:], ov[:, 1:]), (ou[:, :-1], ov[:, :-1]), win, alpha, d)
        new[1][:, :-1] = conv((tot - msg[0])[:, 1:], (ou[:, :-1], ov[:, :-1]), (ou[:, 1:], ov[:, 1:]), win, alpha, d)
        new[2][1:] = conv((tot - msg[3])[:-1], (ou[1:], ov[1:]), (ou[:-1], ov[:-1]), win, alpha, d)
        new[3][:-1] = conv((tot - msg[2])[1:], (ou[:-1], ov[:-1]), (ou[1:], ov[1:]), win, alpha, d)
        new -= new.min(-1, keepdims=True)
        new[0][:, 0] = 0
        new[1][:, -1] = 0
        new[2][0] = 0
        new[3][-1] = 0
        msg = new
        assert msg.min() >= 0 and msg.max() <= 2 * d, "a message leaves 0..2d"
    return msg


def select(dc, msg, off, win):
    """the belief's argmin (numpy's argmin takes the smallest index on ties) -> flow [2,h,w] int64"""
    lu, lv = labels(win)
    arg = (dc + msg.sum(0)).argmin(-1)
    return np.stack([off[0] + lu[arg], off[1] + lv[arg]])


def level(da, db, off, win, iters, p, conv=_conv_separable):
    dc = cost_volume(da, db, off, win, p["gamma"], p["T"])
    return select(dc, propagate(dc, off, win, iters, p["alpha"], p["d"], conv), off, win)


def level_brute(da, db, off, win, iters, p):
    return level(da, db, off, win, iters, p, conv=_conv_brute)


def ld_sum(flow):
    """LD of a flow [2,h,w] in float64, the terms added in the kernels' fixed order: 256 consecutive pixels per partial (per 64
    a pairwise tree, then the four in order), partial t of 256 lanes adds partials t, t + 256, ... in order, a pairwise tree
    over the lanes, one division by h w."""
    fu, fv = flow[0].astype(np.int64).ravel(), flow[1].astype(np.int64).ravel()
    hw = fu.size
    blocks = -(-hw // 256)
    v = np.zeros(blocks * 256, np.float64)
    v[:hw] = np.sqrt((fu * fu + fv * fv).astype(np.float64))
    v = v.reshape(blocks * 4, 64)
    for s in (32, 16, 8, 4, 2, 1):
        v = v[:, :s] + v[:, s:2 * s]
    wv = v.reshape(blocks, 4)
    partials = ((wv[:, 0] + wv[:, 1]) + wv[:, 2]) + wv[:, 3]
    red = np.zeros(256, np.float64)
    for t in range(min(256, blocks)):
        a = 0.0
        for x in partials[t::256]:
            a += x
        red[t] = a
    for s in (128, 64, 32, 16, 8, 4, 2, 1):
        red = red[:s] + red[s:2 * s]
    return float(red[0] / np.float64(hw))


def pyramid(img, levels):
    out = [np.asarray(img).astype(np.int64)]
    for _ in range(levels - 1):
        out.append(reduce2(out[-1]))
    return out


def sift_flow(a, b, **kw):
    """a (the scan), b (the prediction): [h,w] integers 0..255 -> (flow [2,h,w] int16, LD float)"""
    p = params(**kw)
    pa, pb = pyramid(a, p["levels"]), pyramid(b, p["levels"])
    flow = None
    for lv in range(p["levels"] - 1, -1, -1):
        h, w = pa[lv].shape
        da, db = dsift(pa[lv], p["eps"]), dsift(pb[lv], p["eps"])
        if flow is None:
            off, win, iters = (np.zeros((h, w), np.int64), np.zeros((h, w), np.int64)), p["w_top"], p["iters_top"]
        else:
            ys, xs = np.mgrid[0:h, 0:w]
            off, win, iters = (2 * flow[0][ys >> 1, xs >> 1], 2 * flow[1][ys >> 1, xs >> 1]), p["w"], p["iters"]
        flow = level(da, db, off, win, iters, p)
    return flow.astype(np.int16), ld_sum(flow)


# ---- inputs (deterministic) ---------------------------------------------------------------------------------------------------
def page(h, w, seed):
    """A text-like page: rows of dark runs (20..90) on 235, noise of sigma 2."""
    rng = np.random.default_rng(seed)
    img = np.full((h, w), 235.0)
    for y in range(6, h - 6, 7):
        x = 5
        while x < w - 8:
            run = rng.integers(2, 7)
            img[y:y + rng.integers(2, 5), x:x + run] = rng.integers(20, 90)
            x += run + rng.integers(1, 4)
    img += rng.normal(0, 2, (h, w))
    return np.clip(np.rint(img), 0, 255).astype(np.int64)


def shifted(img, su, sv):
    """B(q) = A(q - s), s = (su, sv) in (x, y), indices clamped: the flow from A to B is s"""
    h, w = img.shape
    return img[_cl(np.arange(h) - sv, h)][:, _cl(np.arange(w) - su, w)]
