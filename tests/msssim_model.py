"""Float64 NumPy model of the project's MS-SSIM: the yardstick of tests/test_msssim_cpu.py and
tests/test_gpu_msssim.py.  Written from the definition, not from the kernels of dvd_amd/csrc/metrics.hip.

Preparation, from u8 RGB [H,W,3]:
  target size   the ground truth goes to (round(h s), round(w s)), s = sqrt(area / (h w)); the prediction goes to the
                ground truth's resized size.
  resize        separable, anti-aliased, triangle kernel.  Per axis, r = out/in: output o has its centre at
                u = (o + 0.5)/r - 0.5; tap j has weight tri((u - j) min(r,1)), j = ceil(u - 1/min(r,1)) .. floor(u + 1/min(r,1));
                indices clamped into the axis, weights normalised to sum 1 after clamping.  Rows (axis 0) first, then
                columns; no intermediate rounding; rounded half to even to u8 once.
  gray          round(0.2989 R + 0.5870 G + 0.1140 B), clamped to 0..255 (evaluated exactly: the sum is an integer number
                of 1e-4, ties to even).
Per scale s = 1..5 on gray planes x, y (L = 255, C1 = (0.01 L)^2, C2 = (0.03 L)^2): the normalised 11-tap Gaussian (sigma 1.5)
applied separably gives mu_x, mu_y, E[x^2], E[y^2], E[xy];
  cs = (2 s_xy + C2)/(s_x^2 + s_y^2 + C2),   ssim = cs (2 mu_x mu_y + C1)/(mu_x^2 + mu_y^2 + C1);
the scale's two numbers are the means of ssim and cs over the map.  Between scales both planes are reduced by 2 to ceil(n/2).
  preset 'wang'     valid windows only (map (H-10) x (W-10)); box reduce (x[2i] + x[min(2i+1, n-1)])/2;
                    prod_{s<5} cs_s^w_s * ssim_5^w_5
  preset 'docunet'  replicate border (indices clamped, map H x W); [1,4,6,4,1]/16 centred on 2i, clamped;  sum_s w_s ssim_s
"""
import math

import numpy as np

WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
PRESETS = ("docunet", "wang")
C1 = (0.01 * 255.0) ** 2
C2 = (0.03 * 255.0) ** 2
MIN_SIDE = 176
AREA = 598400


def window():
    d = np.arange(11, dtype=np.float64) - 5.0
    g = np.exp(-(d * d) / (2.0 * 1.5 * 1.5))
    return g / g.sum()


def _check_preset(preset):
    if preset not in PRESETS:
        raise ValueError(f"preset must be 'docunet' or 'wang', got {preset!r}")


# ---- preparation ------------------------------------------------------------------------------------------------------------
def target_size(h, w, area=AREA):
    """(rows, columns) of the resized ground truth; Python's round is half to even, as numpy's."""
    s = math.sqrt(area / (h * w))
    return int(round(h * s)), int(round(w * s))


def axis_taps(isize, osize):
    """Per output index: (clamped tap indices, normalised weights)."""
    r = osize / isize
    s = min(r, 1.0)
    taps = []
    for o in range(osize):
        u = (o + 0.5) / r - 0.5
        j = np.arange(math.ceil(u - 1.0 / s), math.floor(u + 1.0 / s) + 1)
        wt = np.maximum(0.0, 1.0 - np.abs((u - j) * s))
        idx = np.clip(j, 0, isize - 1)
        taps.append((idx, wt / wt.sum()))
    return taps


def axis_matrix(isize, osize):
    """The axis resize as an [osize, isize] matrix (clamped taps accumulate on the border samples)."""
    m = np.zeros((osize, isize), dtype=np.float64)
    for o, (idx, wt) in enumerate(axis_taps(isize, osize)):
        np.add.at(m[o], idx, wt)
    return m


def resize_f64(img, out_h, out_w):
    """[H,W,C] (any real dtype) -> [out_h,out_w,C] float64, before the rounding."""
    a = np.asarray(img, dtype=np.float64)
    a = np.einsum("oh,hwc->owc", axis_matrix(a.shape[0], out_h), a)       # rows first
    return np.einsum("pw,owc->opc", axis_matrix(a.shape[1], out_w), a)    # then columns


def resize_u8(img, out_h, out_w):
    return np.clip(np.rint(resize_f64(img, out_h, out_w)), 0, 255).astype(np.uint8)


def gray(rgb_u8):
    """[H,W,3] u8 -> [H,W] float64 integers 0..255."""
    v = rgb_u8.astype(np.int64)
    t = 2989 * v[..., 0] + 5870 * v[..., 1] + 1140 * v[..., 2]           # the weighted sum in units of 1e-4, exact
    q, rem = t // 10000, t % 10000
    q = q + ((rem > 5000) | ((rem == 5000) & (q % 2 == 1)))
    return np.clip(q, 0, 255).astype(np.float64)


def resize_gray(img_u8, out_h, out_w):
    return gray(resize_u8(img_u8, out_h, out_w))


def knife_edge(img_u8, out_h, out_w, eps=2.0 ** -15):
    """[out_h,out_w] bool: pixels where a channel's value before the rounding is within eps of k + 0.5."""
    f = resize_f64(img_u8, out_h, out_w)
    return (np.abs(f - np.floor(f) - 0.5) <= eps).any(axis=-1)


# ---- one scale --------------------------------------------------------------------------------------------------------------
def filter_axis(a, g, axis, border):
    """Correlate `a` with the 11 taps along `axis`: 'valid' (n - 10 outputs) or 'replicate' (n outputs, indices clamped)."""
    a = np.moveaxis(a, axis, -1)
    n = a.shape[-1]
    if border == "valid":
        out = sum(g[k] * a[..., k:k + n - 10] for k in range(11))
    else:
        idx = np.arange(n)
        out = sum(g[k] * a[..., np.clip(idx + k - 5, 0, n - 1)] for k in range(11))
    return np.moveaxis(out, -1, axis)


def moments(x, y, border):
    g = window()
    f = lambda a: filter_axis(filter_axis(a, g, -1, border), g, -2, border)   # noqa: E731
    return f(x), f(y), f(x * x), f(y * y), f(x * y)


def ssim_maps(x, y, border):
    mx, my, exx, eyy, exy = moments(np.asarray(x, np.float64), np.asarray(y, np.float64), border)
    cs = (2.0 * (exy - mx * my) + C2) / ((exx - mx * mx) + (eyy - my * my) + C2)
    return cs * (2.0 * mx * my + C1) / (mx * mx + my * my + C1), cs


def reduce_axis(a, axis, taps):
    a = np.moveaxis(a, axis, -1)
    n = a.shape[-1]
    i = np.arange((n + 1) // 2)
    if taps == 2:
        out = (a[..., 2 * i] + a[..., np.minimum(2 * i + 1, n - 1)]) / 2.0
    else:
        out = sum(c * a[..., np.clip(2 * i + k - 2, 0, n - 1)] for k, c in enumerate((1.0, 4.0, 6.0, 4.0, 1.0))) / 16.0
    return np.moveaxis(out, -1, axis)


def reduce2(a, taps):
    return reduce_axis(reduce_axis(a, -1, taps), -2, taps)


def ssim_scales(x, y, preset="docunet"):
    """x, y [..., H, W] -> [..., 5, 2] float64: per scale (mean ssim, mean cs)."""
    _check_preset(preset)
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    if x.shape != y.shape or min(x.shape[-2:]) < MIN_SIDE:
        raise ValueError(f"planes of one shape with each side >= {MIN_SIDE} expected, got {x.shape} and {y.shape}")
    border, taps = ("valid", 2) if preset == "wang" else ("replicate", 5)
    out = []
    for s in range(5):
        ssim, cs = ssim_maps(x, y, border)
        out.append(np.stack([ssim.mean(axis=(-2, -1)), cs.mean(axis=(-2, -1))], axis=-1))
        if s < 4:
            x, y = reduce2(x, taps), reduce2(y, taps)
    return np.stack(out, axis=-2)


def combine(scales, preset="docunet"):
    """[..., 5, 2] -> [...] float64."""
    _check_preset(preset)
    s = np.asarray(scales, np.float64)
    w = np.asarray(WEIGHTS)
    if preset == "wang":
        return np.prod(s[..., :4, 1] ** w[:4], axis=-1) * s[..., 4, 0] ** w[4]
    return (s[..., :, 0] * w).sum(axis=-1)


def ms_ssim(x, y, preset="docunet"):
    return combine(ssim_scales(x, y, preset), preset)


def ms_ssim_u8(pred_u8, gt_u8, preset="docunet", area=AREA):
    """The whole protocol for one pair of u8 RGB images [H,W,3] of any two sizes."""
    th, tw = target_size(gt_u8.shape[0], gt_u8.shape[1], area)
    return float(ms_ssim(resize_gray(pred_u8, th, tw), resize_gray(gt_u8, th, tw), preset))
