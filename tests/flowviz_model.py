"""NumPy statement of the flow pictures: THE definition of dvd_flow_to_image_rgb8 / ops.flow_to_image,
dvd_flow_radius_max / ops.flow_radius_max, dvd_flow_full_uv / ops.flow_full_uv and dvd_flow_picture_rgb8 / ops.flow_picture,
byte for byte.  Every float32 line below is one operation of dvd_amd/csrc/flowviz_core.h (and interp_core.h), in its order; NumPy
rounds each on its own, as the kernel does.  The fused multiply-adds of the up-sampling are emulated exactly (`fma32`)."""
import numpy as np

F = np.float32
NORMS = ("diag", "max")
WHEEL_SEGMENTS = (15, 6, 4, 11, 13, 6)          # RY, YG, GC, CB, BM, MR
EPS = F(1e-5)
POLY = (-0.019203662872314453, 0.03365402668714523, -0.045327235013246536, 0.0636562779545784, -0.10610321164131165,
        0.31830987334251404)
RAD_BLOCK, RAD_PER = 256, 16


def make_colorwheel():
    """[55, 3] integers: the Middlebury wheel of Baker et al. (ICCV 2007).  Six segments between the primaries red, yellow,
    green, cyan, blue, magenta; inside a segment of n entries one channel ramps by floor(255 i / n)."""
    ry, yg, gc, cb, bm, mr = WHEEL_SEGMENTS
    rows = []
    rows += [(255, 255 * i // ry, 0) for i in range(ry)]
    rows += [(255 - 255 * i // yg, 255, 0) for i in range(yg)]
    rows += [(0, 255, 255 * i // gc) for i in range(gc)]
    rows += [(0, 255 - 255 * i // cb, 255) for i in range(cb)]
    rows += [(255 * i // bm, 0, 255) for i in range(bm)]
    rows += [(255, 0, 255 - 255 * i // mr) for i in range(mr)]
    return np.asarray(rows, np.int32)


WHEEL = make_colorwheel()


def turn_of(y, x):
    """atan2(y, x) / pi in [-1, 1], float32: exact on the axes and the diagonals, signed zeros as numpy's arctan2 has them."""
    y, x = np.asarray(y, F), np.asarray(x, F)
    ay, ax = np.abs(y), np.abs(x)
    mn, mx = np.where(ay < ax, ay, ax), np.where(ay < ax, ax, ay)
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.where(mx == 0, F(0), np.where(mn == mx, F(1), mn / np.where(mx == 0, F(1), mx))).astype(F)
        upper = q > F(0.41421357)
        r = np.where(upper, (q - F(1)) / (q + F(1)), q).astype(F)
    z = r * r
    p = F(POLY[0])
    for c in POLY[1:]:
        p = p * z + F(c)
    t = r * p
    t = np.where(upper, F(0.25) + t, t)
    t = np.where(ay > ax, F(0.5) - t, t)
    t = np.where(np.signbit(x), F(1) - t, t)
    return np.where(np.signbit(y), -t, t).astype(F)


def _clipped(x, clip):
    if clip is None:
        return x
    c = F(clip)
    return np.where(x < 0, F(0), np.where(x > c, c, x)).astype(F)


def radius(field, clip=None):
    """[..., 2] float32 -> sqrt(u^2 + v^2) of the clipped components; -1 where a component is not finite."""
    field = np.asarray(field, F)
    u, v = field[..., 0], field[..., 1]
    ok = np.isfinite(u) & np.isfinite(v)
    with np.errstate(over="ignore", invalid="ignore"):
        u, v = _clipped(u, clip), _clipped(v, clip)
        return np.where(ok, np.sqrt(u * u + v * v), F(-1)).astype(F)


def radius_max(field, clip=None):
    """The largest radius of one image [h, w, 2], float32, in the kernels' order (any order gives the same maximum)."""
    r = radius(field, clip).reshape(-1)
    per = RAD_BLOCK * RAD_PER
    blocks = (r.size + per - 1) // per
    r = np.concatenate([r, np.zeros(blocks * per - r.size, F)]).reshape(blocks, per)
    return F(max(F(0), r.max(axis=1).max()))


def diag_rad_max(h, w):
    return F(np.sqrt(F((w // 2) ** 2 + (h // 2) ** 2)) + EPS)


def flow_to_image(field, clip_flow=None, convert_to_bgr=False, norm="diag"):
    """[h, w, 2] float32 displacement in pixels -> [h, w, 3] uint8."""
    assert norm in NORMS
    field = np.asarray(field, F)
    h, w = field.shape[:2]
    rad_max = diag_rad_max(h, w) if norm == "diag" else F(radius_max(field, clip_flow) + EPS)
    u, v = field[..., 0], field[..., 1]
    ok = np.isfinite(u) & np.isfinite(v)
    with np.errstate(over="ignore", invalid="ignore"):
        u, v = _clipped(np.where(ok, u, F(0)), clip_flow), _clipped(np.where(ok, v, F(0)), clip_flow)
        rad = (np.sqrt(u * u + v * v) / rad_max).astype(F)
        a = turn_of(-v, -u)
        fk = ((a + F(1)) * F(0.5)) * F(54)
        k0 = np.minimum(fk.astype(np.int32), 54)
        k1 = np.where(k0 + 1 == 55, 0, k0 + 1)
        f = fk - k0.astype(F)
        g = F(1) - f
        out = np.zeros((h, w, 3), np.uint8)
        for ch in range(3):
            col = (g * WHEEL[k0, ch].astype(F) + f * WHEEL[k1, ch].astype(F)) / F(255)
            col = np.where(rad <= F(1), F(1) - rad * (F(1) - col), col * F(0.75)).astype(F)
            byte = np.clip((F(255) * col).astype(np.int32), 0, 255)
            out[..., 2 - ch if convert_to_bgr else ch] = np.where(ok, byte, 0)
    return out


def fma32(a, b, c):
    """round_f32(a b + c) with ONE rounding: the product of two float32 is exact in float64; their sum with c is rounded to
    odd there (the sticky bit of the exact sum, from the error term of the addition), so the final rounding to float32 is the
    rounding of the exact value."""
    a, b, c = (np.asarray(v, F).astype(np.float64) for v in (a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)                 # exact: p + c = s + err
    bits = s.view(np.int64)
    inexact = (err != 0) & np.isfinite(s)
    toward_zero = inexact & ((err > 0) != (s > 0))  # |exact| < |s|: step one unit towards zero first
    bits = np.where(toward_zero, bits - 1, bits)
    bits = np.where(inexact, bits | 1, bits)
    return bits.view(np.float64).astype(F)


def _axis(n_in, n_out):
    """interp_axis for every output index: (i0, i1, l0, l1)."""
    scale = F(n_in - 1) / F(n_out - 1) if n_out > 1 else F(0)
    src = (scale * np.arange(n_out, dtype=F)).astype(F)
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    l1 = np.clip((src - i0.astype(F)).astype(F), F(0), F(1))
    return i0, i1, (F(1) - l1).astype(F), l1


def upsample(flow, h, w, fma=fma32, dtype=F):
    """[2, g, g] -> [2, h, w]: F.interpolate(bilinear, align_corners=True) in interp_sum's order."""
    x = np.asarray(flow, F)
    y0, y1, ly0, ly1 = _axis(x.shape[-2], h)
    x0, x1, lx0, lx1 = _axis(x.shape[-1], w)
    a, b = x[:, y0][:, :, x0], x[:, y0][:, :, x1]
    c, d = x[:, y1][:, :, x0], x[:, y1][:, :, x1]
    ly0, ly1 = ly0[:, None], ly1[:, None]
    if h + w <= 128:
        w00, w01, w10, w11 = ly0 * lx0, ly0 * lx1, ly1 * lx0, ly1 * lx1
        return fma(d, w11, fma(c, w10, fma(a, w00, b * w01)))
    t0 = fma(a, lx0, b * lx1)
    t1 = fma(c, lx0, d * lx1)
    return fma(t0, ly0, t1 * ly1)


def upsample64(flow, h, w):
    """The same interpolation in float64 throughout, from exact rational coordinates: what the float32 one is measured against."""
    x = np.asarray(flow, np.float64)
    g = x.shape[-1]

    def axis(n_out):
        src = np.arange(n_out, dtype=np.float64) * (g - 1) / max(n_out - 1, 1)
        i0 = np.minimum(np.floor(src).astype(np.int64), g - 1)
        return i0, np.minimum(i0 + 1, g - 1), src - i0
    y0, y1, ty = axis(h)
    x0, x1, tx = axis(w)
    a, b = x[:, y0][:, :, x0], x[:, y0][:, :, x1]
    c, d = x[:, y1][:, :, x0], x[:, y1][:, :, x1]
    ty = ty[:, None]
    return (a * (1 - tx) + b * tx) * (1 - ty) + (c * (1 - tx) + d * tx) * ty


def full_uv(flow, h, w):
    """[2, g, g] coarse map -> [h, w, 2] float32 pixel displacement: u = s_x (w - 1), v = s_y (h - 1)."""
    s = upsample(flow, h, w)
    return np.stack([s[0] * F(w - 1), s[1] * F(h - 1)], axis=-1).astype(F)


def flow_picture(flow, h, w, norm="diag", convert_to_bgr=False):
    return flow_to_image(full_uv(flow, h, w), None, convert_to_bgr, norm)


FLO_TAG = 202021.25


def flo_bytes(field):
    """The Middlebury .flo file of a field [h, w, 2]: f32 tag, int32 w, int32 h, then the interleaved (u, v) f32, little endian."""
    field = np.asarray(field, F)
    h, w = field.shape[:2]
    return np.asarray([FLO_TAG], "<f4").tobytes() + np.asarray([w, h], "<i4").tobytes() + field.astype("<f4").tobytes()
