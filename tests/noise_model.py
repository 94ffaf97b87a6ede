"""NumPy statement of the keyed sampler noise and of the map deviation: THE definition of dvd_randn_keyed /
ops.randn_keyed and of dvd_map_deviation / ops.map_deviation, bit for bit.  Every float32 line below is one operation of
dvd_amd/csrc/noise_core.h, in its order; NumPy rounds each on its own, as the kernel does.

Counter of a quad: Philox4x32-10(key (seed & 0xffffffff, crc32(path)), counter (quad, slot, hypothesis, 2))."""
import numpy as np

from corrupt_model import key, philox  # noqa: F401 - the key is the corruption stage's

F = np.float32
STREAM = 2
KPX = 0.987 * 511
DEV_BLOCK, DEV_PER = 256, 4


def uniform_indices(words):
    """The four words of a quad -> (k_a, k_b) pairs: u_a = k_a 2^-24 in (0, 1], u_b = k_b 2^-24 in [0, 1)."""
    w = [np.asarray(v, np.uint64) for v in words]
    return ((w[0] >> np.uint64(8)) + np.uint64(1), w[1] >> np.uint64(8)), ((w[2] >> np.uint64(8)) + np.uint64(1), w[3] >> np.uint64(8))


def neg2ln(k):
    """-2 ln(k 2^-24) for k = 1 .. 2^24, float32."""
    u = np.asarray(k).astype(F) * F(2.0 ** -24)
    b = u.view(np.uint32)
    e = (b >> np.uint32(23)).astype(np.int32) - np.int32(127)
    m = ((b & np.uint32(0x7fffff)) | np.uint32(0x3f800000)).view(F)
    big = m > F(1.41421354)
    m = np.where(big, m * F(0.5), m)
    e = e + big.astype(np.int32)
    f = m - F(1)
    s = f / (F(2) + f)
    z = s * s
    p = F(2.0 / 11.0)
    for c in (2.0 / 9.0, 2.0 / 7.0, 2.0 / 5.0, 2.0 / 3.0):
        p = p * z + F(c)
    lnm = (s + s) + (s * z) * p
    fe = e.astype(F)
    ln = fe * F(0.693359375) + (fe * F(-2.12194440e-4) + lnm)
    return F(-2) * ln


def radius(k):
    """R(u_a) = sqrt(-2 ln u_a), float32."""
    return np.sqrt(neg2ln(k))


def cossin(k):
    """(cos, sin) of 2 pi k 2^-24 for k = 0 .. 2^24 - 1, float32."""
    k = np.asarray(k).astype(np.int64)
    n = (k + (1 << 21)) >> 22
    r = k - (n << 22)
    x = r.astype(F) * F(6.283185307179586 / 16777216.0)
    x2 = x * x
    ps = F(1.0 / 362880.0)
    for c in (-1.0 / 5040.0, 1.0 / 120.0, -1.0 / 6.0):
        ps = ps * x2 + F(c)
    sn = x + (x * x2) * ps
    pc = F(-1.0 / 3628800.0)
    for c in (1.0 / 40320.0, -1.0 / 720.0, 1.0 / 24.0):
        pc = pc * x2 + F(c)
    cs = (F(1) - F(0.5) * x2) + (x2 * x2) * pc
    quad = n & 3
    c = np.where(quad == 0, cs, np.where(quad == 1, -sn, np.where(quad == 2, -cs, sn)))
    s = np.where(quad == 0, sn, np.where(quad == 1, cs, np.where(quad == 2, -sn, -cs)))
    return c.astype(F), s.astype(F)


def box_muller(ka, kb):
    rad = radius(ka)
    c, s = cossin(kb)
    return rad * c, rad * s


def box_muller64(ka, kb):
    """The same uniforms through float64 np.log / np.cos / np.sin."""
    ua, ub = np.asarray(ka, np.float64) * 2.0 ** -24, np.asarray(kb, np.float64) * 2.0 ** -24
    rad = np.sqrt(-2.0 * np.log(ua))
    return rad * np.cos(2.0 * np.pi * ub), rad * np.sin(2.0 * np.pi * ub)


def _sample(k, h, g, slot, pair):
    elems = 2 * g * g
    quads = (elems + 3) // 4
    (a0, b0), (a1, b1) = uniform_indices(philox(*k, np.arange(quads, dtype=np.uint64), slot, h, STREAM))
    z0, z1 = pair(a0, b0)
    z2, z3 = pair(a1, b1)
    return np.stack([z0, z1, z2, z3], axis=1).reshape(-1)[:elems].reshape(2, g, g)


def randn_keyed(keys, n_hyp, g, slot, pair=box_muller):
    """[docs*n_hyp, 2, g, g] float32: sample doc * n_hyp + h is hypothesis h of the document with key keys[doc]."""
    out = [_sample(k, h, g, slot, pair) for k in keys for h in range(n_hyp)]
    dtype = F if pair is box_muller else np.float64
    return np.stack(out).astype(dtype) if out else np.zeros((0, 2, g, g), dtype)


def point_distances(a, b):
    """[docs, g*g] float32: sqrt(dx^2 + dy^2) of maps [docs,2,g,g], each operation rounded."""
    a, b = np.asarray(a, F), np.asarray(b, F)
    dx, dy = a[:, 0] - b[:, 0], a[:, 1] - b[:, 1]
    return np.sqrt(dx * dx + dy * dy).reshape(a.shape[0], -1)


def _tree(v, lanes):
    """Lane 0 of: v += the value lanes/2, .., 1 lanes further down (last axis)."""
    v = v.copy()
    d = lanes // 2
    while d >= 1:
        v[..., :d] = v[..., :d] + v[..., d:2 * d]
        d //= 2
    return v[..., 0]


def ordered_sum(dist):
    """The float64 sum of one document's distances in the kernels' order: per workgroup of 1024 points four per lane
    (stride 256), the wave's tree, the four waves left to right; then lane t of 256 adds partials t, t + 256, ..., and a tree."""
    d = np.asarray(dist, np.float64).reshape(-1)
    per = DEV_BLOCK * DEV_PER
    blocks = (d.size + per - 1) // per
    d = np.concatenate([d, np.zeros(blocks * per - d.size)]).reshape(blocks, DEV_PER, DEV_BLOCK)
    lane = d[:, 0]
    for k in range(1, DEV_PER):
        lane = lane + d[:, k]
    waves = _tree(lane.reshape(blocks, DEV_BLOCK // 64, 64), 64)
    part = ((waves[:, 0] + waves[:, 1]) + waves[:, 2]) + waves[:, 3]
    rows = (blocks + 255) // 256
    part = np.concatenate([part, np.zeros(rows * 256 - blocks)]).reshape(rows, 256)
    lane = np.zeros(256)
    for r in range(rows):
        lane = lane + part[r]
    return float(_tree(lane, 256))


def map_deviation(a, b):
    """[docs] floats: KPX * (ordered sum of the point distances / g^2)."""
    dist = point_distances(a, b)
    return [KPX * (ordered_sum(row) / row.size) for row in dist]
