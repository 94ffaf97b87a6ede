"""Deterministic pages for the scan-like-page tests: noise, constant pages and a text-like page with a bold bar
under smooth shading and a colour cast.  Everything is a function of its arguments; arrays are returned read-only."""
import functools

import numpy as np

PAPER, INK = 232, 40                      # the unshaded text page's two levels
CAST = (1.0, 0.94, 0.84)                  # the colour cast: gains of R, G, B
# the page sizes at which a kernel path can go wrong: one pixel, one row, one column, below a tile, a tile, one past it, odd
# sizes with rows that begin off a dword, more than one tile of every kernel
SIZES = ((1, 1), (1, 67), (67, 1), (33, 31), (64, 16), (65, 17), (97, 61), (130, 257))


def _ro(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def noise(h, w, seed=0):
    return _ro(np.random.RandomState(1000 + seed).randint(0, 256, (h, w, 3)).astype(np.uint8))


@functools.lru_cache(maxsize=None)
def constant(h, w, v):
    return _ro(np.full((h, w, 3), v, np.uint8))


@functools.lru_cache(maxsize=None)
def text_page(h=500, w=700, cast=True, seed=3):
    """A dict: `clean` [h,w,3] the unshaded page (PAPER with strokes and a bold bar of INK), `ink` [h,w] bool, `shade` [h,w]
    float64 in 0.45..1, `gain` the channel gains, `page` [h,w,3] uint8 the photograph: clean x shade x gain plus noise of +-2."""
    rng = np.random.RandomState(seed)
    ink = np.zeros((h, w), bool)
    margin = min(30, h // 8, w // 8)
    bar_h = min(45, max(1, h // 8))
    bar_y = h // 2 - bar_h // 2
    y = margin
    while y + 9 <= h - margin:
        if not (y + 9 < bar_y - 6 or y > bar_y + bar_h + 6):                  # leave room around the bar
            y += 16
            continue
        x = margin
        while x < w - margin - 8:
            word = rng.randint(3, 9)
            for _ in range(word):                                            # a glyph: a 2 px stem and a 2 px cross stroke
                if x >= w - margin - 8:
                    break
                ink[y:y + 9, x:x + 2] = True
                ink[y + int(rng.randint(0, 8)):, x:x + 6][:2] = True
                x += 8
            x += 8
        y += 16
    ink[bar_y:bar_y + bar_h, margin:w - margin] = True
    clean = np.where(ink[..., None], INK, PAPER).astype(np.uint8).repeat(3, axis=2)
    yy, xx = np.mgrid[0:h, 0:w]
    u, v = xx / max(w - 1, 1), yy / max(h - 1, 1)
    ramp = 0.45 + 0.55 * (0.7 * u + 0.3 * v)                                  # a shadow across the page
    vignette = 1.0 - 0.25 * ((u - 0.5) ** 2 + (v - 0.5) ** 2) / 0.5
    shade = np.clip(ramp * vignette, 0.45, 1.0)
    gain = np.array(CAST if cast else (1.0, 1.0, 1.0))
    page = clean.astype(np.float64) * shade[..., None] * gain + rng.randint(-2, 3, (h, w, 3))
    return {"clean": _ro(clean), "ink": _ro(ink), "shade": _ro(shade), "gain": gain,
            "page": _ro(np.clip(np.floor(page + 0.5), 0, 255).astype(np.uint8))}


def page_of(size, kind="noise"):
    """A page of `size` for the kernel tests: noise, or the text page cut to it."""
    h, w = size
    if kind == "noise":
        return noise(h, w, seed=h * 31 + w)
    return text_page(h, w)["page"]


# name -> page: what clean_host_check and the kernels are held to on every parameter set of the tests
CASES = {
    "noise_97x61": lambda: noise(97, 61, 1),
    "zeros_33x31": lambda: constant(33, 31, 0),
    "full_33x31": lambda: constant(33, 31, 255),
    "const77_65x17": lambda: constant(65, 17, 77),
    "text_130x257": lambda: text_page(130, 257)["page"],
}
