"""What the synthetic-document tests share (tests/test_synth_cpu.py, tests/test_gpu_synth.py): forward fields from the map-inverse
fixtures, scans, the render cases, float64 references and the measured bars; each case's model result is computed once."""
import functools

import numpy as np

import mapinv_model as M
import synth_model as Y
from mapinv_fixtures import CASES as INV_CASES, F, SCALE, affine, affine_inverse, collapsed, model as inv_model, photograph, smooth

from dvd_amd import synth_docs

SHADE = dict(l0=0.9, lgx=0.3, lgy=-0.2, k=-0.5)                       # a_ref: hs ws / covered, as ops.synth_document sets it
# The largest difference between the model and the float64 evaluation of the same filter at the analytic position and
# Jacobian of the affine fixture, on smooth_scan, measured on the CPU (test_affine_against_the_analytic_inverse prints it).
AFFINE_MEASURED = {1: 0.52, 3: 0.51}                                   # scan of 1 x and of 3 x the photograph's sides
# unwarp(flow, render(scan, flow)) against the scan, mean absolute difference in levels over the page pixels at least 2 px
# inside, measured on the model with page_scan (test_cycle_returns_the_scan prints it): {case: value}
CYCLE_MEASURED = {"smooth_64x48_g9_s8": 22.94, "smooth_64x48_g9_s1": 22.51, "smooth_96x80_g16_s8": 18.30, "smooth_96x80_g16_s1": 17.98}
CYCLE_BAR = 1.5


@functools.lru_cache(maxsize=None)
def fwd_of(name):
    """A forward field by name: a case of mapinv_fixtures, or one of the sizes only this render needs."""
    if name in INV_CASES:
        return inv_model(name)["fwd"]
    if name.startswith("hand_"):
        return hand_made(name == "hand_1x40")
    flow, h, w, step = {"tall_40x1": (smooth(4, 0.03), 40, 1, 3), "edge_33x31": (smooth(4, 0.03), 33, 31, 3),
                        "wide_20x70": (smooth(9, 0.03), 20, 70, 4), "small_40x32": (smooth(9, 0.06), 40, 32, 3),
                        "calm_40x32": (smooth(4, 0.03), 40, 32, 3),
                        "uncovered_24x20": (collapsed(), 24, 20, 8), "identity_64x48": (np.zeros((2, 9, 9), F), 64, 48, 8)}[name]
    fwd = M.invert(flow, h, w, step, SCALE)[0]
    fwd.setflags(write=False)
    return fwd


def hand_made(row):
    """A field of one row (or one column) with covered pixels - the mesh of such a photograph has no area, so map_invert covers
    none: positions that run past both ends of the page, a gap, a NaN and an infinity."""
    t = np.linspace(-3, 44, 40).astype(F)
    t[7:10] = np.uint32(M.INVALID).view(F)
    fwd = np.stack([t, np.zeros_like(t)] if row else [np.zeros_like(t), t], axis=-1)
    fwd[20, 0 if row else 1], fwd[30, 0 if row else 1] = np.nan, np.inf
    fwd[7:10] = np.uint32(M.INVALID).view(F)
    fwd = np.ascontiguousarray(fwd.reshape((1, 40, 2) if row else (40, 1, 2)))
    fwd.setflags(write=False)
    return fwd


@functools.lru_cache(maxsize=None)
def page_scan(hs, ws, seed=5):
    """The text-like page of the dataset writer, as the tests' scan."""
    page = synth_docs.procedural_page(synth_docs.document_key(seed, f"{hs}x{ws}"), hs, ws)
    page.setflags(write=False)
    return page


@functools.lru_cache(maxsize=None)
def smooth_scan(hs, ws):
    """Low-frequency colour: at most about two levels of curvature per pixel at 64 x 48."""
    y, x = np.meshgrid(np.linspace(0, 1, hs), np.linspace(0, 1, ws), indexing="ij")
    img = np.stack([128 + 100 * np.sin(3 * x + 1) * np.cos(2 * y), 128 + 90 * np.cos(4 * x * y + 0.5), 60 + 150 * x * (1 - y)], axis=-1)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def background_plane(h, w):
    return photograph(h, w, seed=11)


# name -> (fwd name, scan (hs, ws), scan kind, background kind, shading)
RENDER_CASES = {
    "smooth_37x29": ("smooth_37x29_g4_s3", (37, 29), "page", "triple", None),              # radius 1 everywhere
    "smooth_37x29_noise": ("smooth_37x29_g4_s3", (37, 29), "noise", "plane", SHADE),
    "smooth_96x80": ("smooth_96x80_g16_s8", (96, 80), "page", "triple", None),             # dword stores, more than one tile in x and y
    "smooth_96x80_shaded": ("smooth_96x80_g16_s8", (96, 80), "page", "plane", SHADE),
    "folded": ("folded", (96, 80), "page", "triple", SHADE),
    "nan": ("nan", (64, 48), "page", "plane", None),
    "uncovered": ("uncovered_24x20", (24, 20), "page", "plane", SHADE),
    "thin_1x40": ("thin_1xN", (8, 40), "page", "triple", SHADE),
    "tall_40x1": ("tall_40x1", (40, 8), "page", "plane", SHADE),
    "hand_1x40": ("hand_1x40", (8, 40), "noise", "triple", SHADE),
    "hand_40x1": ("hand_40x1", (40, 8), "noise", "plane", SHADE),
    "edge_33x31": ("edge_33x31", (33, 31), "noise", "triple", None),
    "wide_20x70": ("wide_20x70", (45, 130), "page", "plane", SHADE),                         # byte stores across a tile edge in x
    "minify_3": ("small_40x32", (120, 96), "page", "triple", None),                         # mixed radii, none at the cap
    "minify_3_shaded": ("small_40x32", (120, 96), "noise", "plane", SHADE),
    "minify_10": ("calm_40x32", (400, 320), "page", "triple", SHADE),                      # every covered pixel at the cap
    "magnify": ("small_40x32", (9, 11), "noise", "triple", None),
}
TRIPLE = (31, 120, 222)


@functools.lru_cache(maxsize=None)
def render_case(name):
    """dict: scan, fwd, background (triple or plane), shading (None or the five parameters), photo and radii by the model."""
    fwd_name, (hs, ws), scan_kind, bg_kind, shading = RENDER_CASES[name]
    fwd = fwd_of(fwd_name)
    h, w = fwd.shape[:2]
    scan = page_scan(hs, ws) if scan_kind == "page" else photograph(hs, ws, seed=3)
    bg = TRIPLE if bg_kind == "triple" else background_plane(h, w)
    if shading is not None:
        covered = int(Y.covered_of(fwd).sum())
        shading = dict(shading, a_ref=float(F(hs * ws / covered)) if covered else 1.0)
    out = {"scan": scan, "fwd": fwd, "background": bg, "shading": shading, "photo": Y.render(scan, fwd, bg, shading),
           "radii": Y.footprint(fwd, hs, ws)}
    for v in (out["photo"], out["radii"]):
        v.setflags(write=False)
    return out


# ---- float64 references -----------------------------------------------------------------------------------------------------------
def bilinear64(img, x, y):
    """img [h,w,3] at float64 positions (x, y), clamped to the image: the plain bilinear formula."""
    img = np.asarray(img, np.float64)
    h, w = img.shape[:2]
    x, y = np.clip(x, 0, w - 1), np.clip(y, 0, h - 1)
    x0, y0 = np.minimum(np.floor(x).astype(int), max(w - 2, 0)), np.minimum(np.floor(y).astype(int), max(h - 2, 0))
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    fx, fy = (x - x0)[..., None], (y - y0)[..., None]
    return (img[y0, x0] * (1 - fx) + img[y0, x1] * fx) * (1 - fy) + (img[y1, x0] * (1 - fx) + img[y1, x1] * fx) * fy


def tent64(img, x, y, rx, ry):
    """The render's filter in float64: the separable tent of integer half-widths rx, ry at the positions (x, y) [n], the taps
    clamped to the image, normalised by the weights' own sum."""
    img = np.asarray(img, np.float64)
    h, w = img.shape[:2]
    out = np.zeros((len(x), 3))
    for i, (px, py) in enumerate(zip(x, y)):
        cols = np.arange(int(np.floor(px)) - rx + 1, int(np.floor(px)) + rx + 1)
        rows = np.arange(int(np.floor(py)) - ry + 1, int(np.floor(py)) + ry + 1)
        wx, wy = np.maximum(0, rx - np.abs(cols - px)), np.maximum(0, ry - np.abs(rows - py))
        tex = img[np.clip(rows, 0, h - 1)[:, None], np.clip(cols, 0, w - 1)[None, :]]
        out[i] = (tex * (wy[:, None] * wx[None, :])[..., None]).sum(axis=(0, 1)) / (wx.sum() * wy.sum())
    return out


def unwarp_model(flow, photo, scale=SCALE):
    """The page: the photograph sampled bilinearly at the backward map's positions (float64 on mapinv_model.positions)."""
    h, w = photo.shape[:2]
    x, y = M.positions(flow, h, w, scale)
    return np.clip(np.floor(bilinear64(photo, x.astype(np.float64), y.astype(np.float64)) + 0.5), 0, 255).astype(np.uint8)


def cycle_difference(scan, page):
    """Mean absolute difference in levels over the page pixels at least 2 px inside."""
    a, b = np.asarray(scan, np.float64), np.asarray(page, np.float64)
    return float(np.abs(a - b)[2:-2, 2:-2].mean())
