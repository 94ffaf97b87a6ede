"""The cases of the page at a chosen size, shared by tests/test_sized_cpu.py (the sanitised restatement) and
tests/test_gpu_sized.py (the kernels): both are held to tests/sized_model.py byte for byte on the same list.  A case's model
result is computed once and never written to."""
import functools
import zlib

import numpy as np

import sized_model as Z

F = np.float32


def photograph(h, w, seed=0):
    """[h,w,3] uint8 random bytes: neighbouring texels differ by up to 255, so a position that is off by one Q8 step shows."""
    return np.random.default_rng(1000 + seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def smooth_flow(g, seed=0, amp=0.03):
    """[2,g,g] f32: a low-order smooth displacement of at most about `amp` of the side, so the page stays inside the frame
    (the scale 0.987 leaves 0.0065 of margin; amp above that leaves the frame on purpose)."""
    rng = np.random.default_rng(2000 + seed)
    t = np.linspace(0, 1, g)
    yy, xx = np.meshgrid(t, t, indexing="ij")
    a = rng.uniform(-1, 1, (2, 4))
    f = [a[c, 0] * np.sin(np.pi * xx) * np.sin(np.pi * yy) + a[c, 1] * np.sin(2 * np.pi * xx) * np.sin(np.pi * yy) +
         a[c, 2] * np.sin(np.pi * xx) * np.sin(2 * np.pi * yy) + a[c, 3] * (xx - 0.5) * (yy - 0.5) for c in range(2)]
    return (amp * np.stack(f) / 2).astype(F)


def make_flow(kind, g, seed):
    if kind == "zero":
        return np.zeros((2, g, g), F)
    if kind == "smooth":
        return smooth_flow(g, seed)
    if kind == "wild":                                        # leaves the frame here and there: zeros padding, centres outside
        return smooth_flow(g, seed, amp=0.4)
    if kind == "nan":                                         # NaN and both infinities among smooth values
        f = smooth_flow(g, seed)
        f[0, 0, 0], f[1, g - 1, g // 2], f[0, g // 2, g - 1] = np.nan, np.inf, -np.inf
        return f
    if kind == "off":                                         # the whole page far off the photograph
        return smooth_flow(g, seed) + F(3)
    if kind == "steep":                                       # node-to-node noise: derivatives far above the cap
        return np.random.default_rng(3000 + seed).uniform(-0.45, 0.45, (2, g, g)).astype(F)
    raise ValueError(kind)


# name -> (flow kind, G, photograph (H, W), page (hp, wp), scale, max_radius)
CASES = {}


def _add(kind, g, src, size, scale=0.987, max_radius=16):
    CASES[f"{kind}_g{g}_{src[0]}x{src[1]}_to_{size[0]}x{size[1]}_s{scale}_r{max_radius}"] = (kind, g, src, size, scale, max_radius)


# the tile of 64 x 16 page pixels: one under, exactly on, one over, several tiles; widths 1, 2, 3, 5, 7 and rows that begin on
# every byte phase of a dword - each size both ways round; hp + wp <= 128 takes interp_sum's `small` order, above it the other
for k, (a, b) in enumerate(((1, 1), (1, 5), (7, 1), (3, 2), (63, 15), (64, 16), (65, 17), (130, 33))):
    for size in sorted({(a, b), (b, a)}):
        _add("smooth", (2, 8, 16)[k % 3], ((48, 64), (97, 61))[k % 2], size)
# tiny photographs: every tap row and column at the photograph's edge
for src, size, g in (((1, 1), (3, 2), 2), ((1, 1), (17, 65), 8), ((2, 2), (7, 1), 2), ((2, 2), (15, 63), 16), ((2, 2), (1, 1), 8)):
    _add("wild", g, src, size)
# the radii: 1 (magnified), 2, 3, 16, and the cap (a photograph of 400 x 300 to a page of 20 x 15 asks for 21)
_add("smooth", 8, (48, 64), (97, 131))
_add("smooth", 8, (97, 61), (49, 31))
_add("smooth", 16, (97, 61), (33, 21))
_add("zero", 2, (400, 300), (25, 19))
_add("zero", 2, (400, 300), (20, 15))
_add("smooth", 8, (400, 300), (20, 15))
# max_radius 1, 4 and 16 on one minified page
for r in (1, 4, 16):
    _add("smooth", 8, (97, 61), (19, 13), max_radius=r)
_add("zero", 8, (64, 64), (32, 32), scale=1.0, max_radius=1)
_add("zero", 8, (64, 64), (32, 32), scale=1.0)
# the hostile maps
_add("nan", 8, (48, 64), (65, 17))
_add("nan", 16, (97, 61), (33, 130), max_radius=4)
_add("off", 8, (48, 64), (17, 65))
_add("wild", 8, (97, 61), (65, 67))
_add("steep", 16, (97, 61), (40, 25))
_add("steep", 16, (400, 300), (20, 15), max_radius=4)


@functools.lru_cache(maxsize=None)
def case(name):
    """dict: flow, src, size, scale, max_radius and the model's page, foot (uint16) and stats."""
    kind, g, src_hw, size, scale, max_radius = CASES[name]
    seed = zlib.crc32(name.encode()) % 1000
    flow, src = make_flow(kind, g, seed), photograph(*src_hw, seed=seed)
    page, stats = Z.unwarp(flow, src, size, scale, max_radius)
    foot = Z.footprint(flow, src_hw, size, scale, max_radius)
    for a in (flow, src, page, foot):
        a.setflags(write=False)
    return dict(flow=flow, src=src, size=size, scale=scale, max_radius=max_radius, page=page, foot=foot, stats=stats)
