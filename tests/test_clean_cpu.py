"""Scan-like pages without a device: the NumPy definition tests/clean_model.py against SciPy and float64, its
exact cases, what it does to a shaded text page, the sanitised stand-alone restatement clean_host_check.cpp against it byte for
byte, and what the library, ops and the command-line tools do before any launch."""
import ctypes as C
import json
import os
import struct
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clean_fixtures as X  # noqa: E402
import clean_model as M  # noqa: E402
import msssim_model as S  # noqa: E402
from host_check import build_host_check  # noqa: E402

from dvd_amd import lib, ops  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the definition against independent statements ---------------------------------------------------------------------------
@pytest.mark.parametrize("cell", [4, 16, 64])
def test_cell_maximum_is_a_reshape(cell):
    img = X.noise(128, 192, 2)
    want = img.reshape(128 // cell, cell, 192 // cell, cell, 3).max(axis=(1, 3)).transpose(2, 0, 1)
    assert np.array_equal(M.cell_max(img, cell), want)
    ragged = X.noise(97, 61, 1)                                   # cells cut at the page's edge
    got = M.cell_max(ragged, cell)
    assert got.shape == (3, -(-97 // cell), -(-61 // cell))
    assert np.array_equal(got[:, -1, -1], ragged[(97 - 1) // cell * cell:, (61 - 1) // cell * cell:].reshape(-1, 3).max(axis=0))


@pytest.mark.parametrize("k", [0, 1, 2, 8])
def test_closing_equals_scipy(k):
    """mode='nearest' replicates an edge cell that the clipped window already holds, so neither extremum changes."""
    ndi = pytest.importorskip("scipy.ndimage")
    for shape in ((3, 7, 9), (3, 23, 31), (3, 1, 5)):             # also windows wider than the plane
        plane = np.random.RandomState(k).randint(0, 256, shape)
        size = (1, 2 * k + 1, 2 * k + 1)
        want = ndi.minimum_filter(ndi.maximum_filter(plane, size=size, mode="nearest"), size=size, mode="nearest")
        assert np.array_equal(M.closing(plane, k), want)


@pytest.mark.parametrize("b", [0, 1, 2, 8])
def test_smoothing_is_within_half_a_level_of_float64(b):
    for shape in ((3, 7, 9), (3, 23, 31), (3, 1, 5)):
        plane = np.random.RandomState(b).randint(0, 256, shape)
        hc, wc = shape[1:]
        want = np.zeros(shape)
        for y in range(hc):
            for x in range(wc):
                ys, xs = np.arange(max(0, y - b), min(hc, y + b + 1)), np.arange(max(0, x - b), min(wc, x + b + 1))
                wgt = np.outer(b + 1.0 - abs(ys - y), b + 1.0 - abs(xs - x))
                want[:, y, x] = (plane[:, ys][:, :, xs] * wgt).sum(axis=(1, 2)) / wgt.sum()
        got = M.smoothed(plane, b)
        assert np.abs(got - want).max() <= 0.5 + 1e-9
        assert got.min() >= plane.min() and got.max() <= plane.max()


@pytest.mark.parametrize("cell,white", [(4, 255), (16, 255), (16, 200), (64, 131)])
def test_flatten_is_within_half_a_level_of_float64(cell, white):
    img = X.text_page(130, 257)["page"]
    bg = M.background(img, cell)
    h, w = img.shape[:2]
    # the float64 bilinear sample between the cell centres (i + 1/2) s - 1/2, clamped at the plane's edge
    cy = np.clip((np.arange(h) + 0.5) / cell - 0.5, 0, bg.shape[1] - 1)
    cx = np.clip((np.arange(w) + 0.5) / cell - 0.5, 0, bg.shape[2] - 1)
    y0, x0 = np.minimum(np.floor(cy).astype(int), bg.shape[1] - 1), np.minimum(np.floor(cx).astype(int), bg.shape[2] - 1)
    y1, x1 = np.minimum(y0 + 1, bg.shape[1] - 1), np.minimum(x0 + 1, bg.shape[2] - 1)
    fy, fx = (cy - y0)[None, :, None], (cx - x0)[None, None, :]
    b = bg.astype(np.float64)
    sample = (1 - fy) * ((1 - fx) * b[:, y0][:, :, x0] + fx * b[:, y0][:, :, x1]) + fy * ((1 - fx) * b[:, y1][:, :, x0] + fx * b[:, y1][:, :, x1])
    assert np.abs(M.bg_q(bg, h, w, cell) / (4.0 * cell * cell) - sample).max() < 1e-9          # bgQ / 4 s^2 IS that sample
    quotient = img.transpose(2, 0, 1) * float(white) / np.maximum(sample, 1.0)
    got, stats = M.flatten(img, bg, cell, white=white)
    ok = quotient <= 255
    assert ok.any() and np.abs(got.transpose(2, 0, 1) - quotient)[ok].max() <= 0.5 + 1e-9
    assert (got.transpose(2, 0, 1)[~ok] == 255).all() and stats["saturated"] == int((np.floor(quotient + 0.5) > 255).sum())


def test_exact_flatten_cases():
    for size in ((33, 31), (1, 1), (97, 61)):
        for white in (255, 200, 1):
            for v in (77, 1, 254):
                out, stats = M.flatten(X.constant(*size, v), white=white)
                assert (out == white).all() and stats == {"saturated": 0, "floored": 0}          # a constant page: exactly white
        out, stats = M.flatten(X.constant(*size, 255))
        assert (out == 255).all() and stats == {"saturated": 0, "floored": 0}
        out, stats = M.flatten(X.constant(*size, 0), white=200)
        assert (out == 0).all() and stats == {"saturated": 0, "floored": 3 * size[0] * size[1]}


SAUVOLA = [(1, 128), (7, 256), (15, 51), (63, 51)]


@pytest.mark.parametrize("r,kq", SAUVOLA)
@pytest.mark.parametrize("page", ["noise", "text"])
def test_sauvola_against_float64(page, r, kq):
    """The integer decision may differ from g <= m (1 + (kq / 256)(sd / 128 - 1)) only where |g - T| <= kq 255 / (256 128 N) +
    1e-9: sN = floor(sqrt(D)) is less than 1 short, so T is less than kq m / (256 128 N) short and m <= 255.  Measured
    of 350 000 pixels: on the noise page 51, 1, 2 and 0 differ at the four (r, kq), on the text page 13, 0, 0 and 0 - every one
    inside the bound."""
    img = X.noise(500, 700, 5) if page == "noise" else X.text_page()["page"]
    g = M.gray(img).astype(np.float64)
    plane, stats = M.binarize(img, r, kq)
    n, s1, s2 = (a.astype(np.float64) for a in M.window_sums(M.gray(img), r))
    m = s1 / n
    sd = np.sqrt(np.maximum(s2 / n - m * m, 0.0))
    t = m * (1 + (kq / 256.0) * (sd / 128.0 - 1))
    want = g <= t
    differ = (plane == 0) != want
    print(f"sauvola {page} r={r} kq={kq}: {int(differ.sum())} of {differ.size} differ, ink {stats['ink']}")
    assert stats["ink"] == int((plane == 0).sum()) and set(np.unique(plane)) <= {0, 255}
    assert (np.abs(g - t)[differ] <= kq * 255 / (256.0 * 128 * n[differ]) + 1e-9).all()


def _paper_and_ink(flat, page, white=255):
    truth = page["clean"].astype(np.float64) * (white / float(X.PAPER))               # v / shade x white / paper of the unshaded page
    err = np.abs(flat.astype(np.float64) - truth)
    ink = np.broadcast_to(page["ink"][..., None], err.shape)
    return err[~ink].mean(), err[~ink].max(), err[ink].mean(), err[ink].max()


def test_shaded_text_page():
    """Flatten at the defaults on the 500 x 700 text page (paper 232, ink 40, a 45 px bar, shading 0.45..1 with a vignette, a
    colour cast, noise of +-2).  Truth: the unshaded page times white / paper - paper at 255, ink at 40 * 255 / 232 = 43.97.
    Measured on this model: the paper is off by 6.90 on average (its mean is 248.1) and 35 at most (beside the bar), the ink by
    2.27 on average and 9 at most; 3699 samples saturate.  The model is deterministic; the bounds are twice the measured values
    and cover later fixture edits only."""
    page = X.text_page()
    flat, stats = M.flatten(page["page"])
    paper_mean, paper_max, ink_mean, ink_max = _paper_and_ink(flat, page)
    print(f"text page: paper mean {paper_mean:.3f} max {paper_max:.0f}; ink mean {ink_mean:.3f} max {ink_max:.0f}; {stats}")
    assert paper_mean <= 2 * 6.90 and paper_max <= 2 * 35 and ink_mean <= 2 * 2.27 and ink_max <= 2 * 9
    before = _paper_and_ink(page["page"], page)
    assert paper_mean < before[0] and ink_mean < before[2]                            # and far better than the photograph


def test_colour_cast():
    page = X.text_page()
    paper = ~page["ink"]
    assert X.CAST[0] > X.CAST[1] > X.CAST[2]
    neutral = M.flatten(page["page"], neutral=True)[0][paper].mean(axis=0)
    kept = M.flatten(page["page"], neutral=False)[0][paper].mean(axis=0)
    print("paper channel means: neutral", neutral, "cast kept", kept)
    assert neutral.max() - neutral.min() <= 1.0
    assert kept[0] > kept[1] > kept[2] and kept[0] - kept[2] > 1.0                     # the order of the cast, still apart


def test_msssim_improves():
    """MS-SSIM (tests/msssim_model.py) against the unshaded page: the flattened page scores strictly higher than the
    photograph.  Measured at an area of 120 000 pixels (the metric's own 598 400 gives 0.9914 and 0.8420, five times slower):
    0.9890 flattened, 0.8120 shaded."""
    page = X.text_page(cast=False)
    flat = M.flatten(page["page"])[0]
    a, b = S.ms_ssim_u8(flat, page["clean"], area=120000), S.ms_ssim_u8(page["page"], page["clean"], area=120000)
    print(f"ms-ssim against the unshaded page: flattened {a:.4f}, shaded {b:.4f}")
    assert a > b


def test_binarize_with_and_without_flatten():
    """The share of pixels that differ from the true ink mask.  Measured at the defaults: 0.0292 binarising the photograph,
    0.0282 binarising the flattened page (the bold bar's inside is wider than the window and reads as paper either way).  Asserted: flatten does not make it worse."""
    page = X.text_page()
    direct = (M.binarize(page["page"])[0] == 0) != page["ink"]
    chain = (M.clean(page["page"], True, True)[0] == 0) != page["ink"]
    print(f"wrong pixels: without flatten {direct.mean():.4f}, with flatten {chain.mean():.4f}")
    assert chain.mean() <= direct.mean()
    bar = page["ink"].copy()
    assert chain[bar].mean() < 0.5                                                     # the ink mask is recovered, not inverted


# ---- the sanitised stand-alone restatement -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("clean_host_check")
    exe = build_host_check("clean", tmp)

    def run(img, cell=16, close=2, smooth=2, neutral=1, white=255, radius=15, kq=51, dims=None):
        h, w = dims if dims else img.shape[:2]
        (tmp / "in.bin").write_bytes(struct.pack("<9i", h, w, cell, close, smooth, neutral, white, radius, kq) + img.tobytes())
        out = tmp / "out.bin"
        if out.exists():
            out.unlink()
        p = subprocess.run([str(exe), str(tmp / "in.bin"), str(out)], capture_output=True, text=True)
        assert p.returncode == 0 and p.stderr == "", (p.returncode, p.stderr[-2000:])          # a status, never a sanitizer report
        return int(p.stdout), (out.read_bytes() if out.exists() else None)
    return run


HOST_PARAMS = [dict(), dict(cell=4, close=0, smooth=8, neutral=0, white=200, radius=1, kq=0),
               dict(cell=64, close=8, smooth=0, radius=7, kq=256), dict(cell=8, close=1, smooth=1, neutral=0, radius=63, kq=128)]


@pytest.mark.parametrize("params", HOST_PARAMS, ids=lambda p: "-".join(f"{k}{v}" for k, v in p.items()) or "defaults")
@pytest.mark.parametrize("name", list(X.CASES))
def test_host_check_equals_the_model(host_check, name, params):
    img = X.CASES[name]()
    if params.get("radius") == 63 and img.shape[0] * img.shape[1] > 2000:
        img = img[:40, :45]                                       # the restatement sums every window pixel by pixel
    img = np.ascontiguousarray(img)
    h, w = img.shape[:2]
    p = dict(cell=16, close=2, smooth=2, neutral=1, white=255, radius=15, kq=51)
    p.update(params)
    status, out = host_check(img, **p)
    bg = M.background(img, p["cell"], p["close"], p["smooth"], bool(p["neutral"]))
    page, st = M.flatten(img, bg, p["cell"], white=p["white"])
    plane, ink = M.binarize(page, p["radius"], p["kq"])
    plane_img, ink_img = M.binarize(img, p["radius"], p["kq"])
    n, nb = h * w, bg.size
    assert status == 0 and len(out) == nb + 5 * n + 32
    assert np.array_equal(np.frombuffer(out, np.uint8, nb).reshape(bg.shape), bg)               # byte for byte
    assert np.array_equal(np.frombuffer(out, np.uint8, 3 * n, nb).reshape(h, w, 3), page)
    assert np.array_equal(np.frombuffer(out, np.uint8, n, nb + 3 * n).reshape(h, w), plane)
    assert np.array_equal(np.frombuffer(out, np.uint8, n, nb + 4 * n).reshape(h, w), plane_img)
    assert list(np.frombuffer(out[nb + 5 * n:], np.uint64)) == [st["saturated"], st["floored"], ink["ink"], ink_img["ink"]]


def test_host_check_refuses_with_a_status(host_check):
    img = np.zeros((5, 5, 3), np.uint8)
    for dims in ((0, 5), (5, 0), (16385, 5), (5, 16385), (-1, 5)):
        assert host_check(img, dims=dims) == (lib.E_CLEAN_SHAPE, None)
    for bad in (dict(cell=5), dict(cell=128), dict(cell=0), dict(close=-1), dict(close=9), dict(smooth=9), dict(smooth=-1), dict(white=0),
                dict(white=256), dict(radius=0), dict(radius=64), dict(kq=-1), dict(kq=257)):
        assert host_check(img, **bad) == (lib.E_CLEAN_PARAM, None)


# ---- the library and ops before any launch ---------------------------------------------------------------------------------------
@pytest.fixture
def no_launch(monkeypatch):
    def fail(name, *args):
        raise AssertionError(f"{name} was called")
    monkeypatch.setattr(lib, "call", fail)


def test_ops_refuse_before_any_launch(no_launch):
    img = torch.zeros(40, 56, 3, dtype=torch.uint8)               # on the host: a good call gets as far as this and no further
    for fn in (ops.page_background, ops.page_flatten, ops.page_clean):
        for cell in (5, 0, 128, 16.0, True, "16", None):
            with pytest.raises(ValueError, match="cell"):
                fn(img, cell=cell)
        for close in (-1, 9, 2.0, None):
            with pytest.raises(ValueError, match="close"):
                fn(img, close=close)
        for smooth in (-1, 9, True, "2"):
            with pytest.raises(ValueError, match="smooth"):
                fn(img, smooth=smooth)
        with pytest.raises(ValueError, match="img.*device"):
            fn(img)
    for fn in (ops.page_flatten, ops.page_clean):
        for white in (0, 256, 255.0, None):
            with pytest.raises(ValueError, match="white"):
                fn(img, white=white)
    for fn, kw in ((ops.page_binarize, {}), (ops.page_clean, dict(binarize=True))):
        for radius in (0, 64, 15.0, None, True):
            with pytest.raises(ValueError, match="radius"):
                fn(img, radius=radius, **kw)
        for k in (-0.01, 1.01, float("nan"), "0.2", None, True):
            with pytest.raises(ValueError, match="k must"):
                fn(img, k=k, **kw)
    with pytest.raises(ValueError, match="img_or_gray.*device"):
        ops.page_binarize(img)
    with pytest.raises(ValueError, match="nothing to do"):
        ops.page_clean(img, flatten=False, binarize=False)
    for bad in (np.zeros((4, 4, 3), np.uint8), None):
        with pytest.raises(ValueError, match="img"):
            ops.page_flatten(bad)
    assert [ops.clean_kq(k) for k in (0, 0.2, 0.5, 1, 0.001, 0.002)] == [0, 51, 128, 256, 0, 1]
    assert ops.CLEAN_STATS == M.STATS and ops.CLEAN_CELLS == M.CELLS and M.kq_of(0.2) == 51


def test_library_refuses_before_any_launch():
    raw = lib.raw()

    def err():
        return raw.dvd_last_error().decode()
    assert raw.dvd_page_clean_workspace_bytes(0, 5, 16) == lib.E_CLEAN_SHAPE and "sides 1..16384" in err()
    assert raw.dvd_page_clean_workspace_bytes(5, 5, 5) == lib.E_CLEAN_PARAM and "cell = 5" in err()
    # three pieces, each rounded up to 256 bytes: the cell maxima and the background [3,hc,wc] and the gray plane [h,w]
    assert raw.dvd_page_clean_workspace_bytes(100, 70, 16) == 2 * 256 + 7168 and raw.dvd_page_clean_workspace_bytes(1, 1, 64) == 3 * 256


def test_library_argument_codes():
    """Every refusal is decided on the host: null pointers, shapes, parameters, misaligned counts and shared bytes."""
    raw = lib.raw()
    buf = (C.c_ubyte * 8192)()
    base = (C.addressof(buf) + 255) // 256 * 256
    img, out, bg, ws = base, base + 1024, base + 2048, base + 4096

    def err():
        return raw.dvd_last_error().decode()
    assert raw.dvd_page_background(None, 8, 8, 16, 2, 2, 1, bg, ws, None) == -1 and "null" in err()
    assert raw.dvd_page_background(img, 0, 8, 16, 2, 2, 1, bg, ws, None) == lib.E_CLEAN_SHAPE
    assert raw.dvd_page_background(img, 8, 8, 16, 9, 2, 1, bg, ws, None) == lib.E_CLEAN_PARAM and "close = 9" in err()
    assert raw.dvd_page_background(img, 8, 8, 16, 2, 2, 1, bg, img, None) == -1 and "share" in err()
    assert raw.dvd_page_flatten_rgb8(img, 8, 8, bg, 16, 0, out, None, None, None) == lib.E_CLEAN_PARAM and "white = 0" in err()
    assert raw.dvd_page_flatten_rgb8(img, 8, 8, bg, 16, 255, img + 3, None, None, None) == -1 and "share" in err()
    assert raw.dvd_page_flatten_rgb8(img, 8, 8, bg, 16, 255, out, None, ws + 4, None) == -1 and "misaligned" in err()
    assert raw.dvd_page_flatten_rgb8(img, 8, 8, None, 16, 255, out, None, None, None) == -1 and "null" in err()
    assert raw.dvd_page_binarize_u8(img, 2, 8, 8, 15, 51, out, None, None) == -1 and "channels = 2" in err()
    assert raw.dvd_page_binarize_u8(img, 3, 8, 8, 64, 51, out, None, None) == lib.E_CLEAN_PARAM and "radius = 64" in err()
    assert raw.dvd_page_binarize_u8(img, 3, 8, 8, 15, 257, out, None, None) == lib.E_CLEAN_PARAM
    assert raw.dvd_page_binarize_u8(img, 3, 8, 16385, 15, 51, out, None, None) == lib.E_CLEAN_SHAPE
    assert raw.dvd_page_binarize_u8(img, 1, 8, 8, 15, 51, img + 63, None, None) == -1 and "share" in err()
    clean = (img, 8, 8, 16, 2, 2, 1, 255)
    assert raw.dvd_page_clean_rgb8(*clean, 0, 0, 15, 51, out, bg, None, ws, None) == -1 and "neither" in err()
    assert raw.dvd_page_clean_rgb8(*clean, 1, 1, 15, 51, out, None, None, ws, None) == -1 and "null" in err()
    assert raw.dvd_page_clean_rgb8(*clean, 1, 0, 15, 51, None, None, None, ws, None) == -1 and "null" in err()
    assert raw.dvd_page_clean_rgb8(*clean, 1, 1, 0, 51, out, bg, None, ws, None) == lib.E_CLEAN_PARAM
    assert raw.dvd_page_clean_rgb8(*clean, 1, 0, 0, 51, out, None, None, out + 8, None) == -1 and "share" in err()


def test_exports_are_bound_and_declared():
    names = ("dvd_page_background", "dvd_page_flatten_rgb8", "dvd_page_binarize_u8", "dvd_page_clean_workspace_bytes", "dvd_page_clean_rgb8")
    header = open(os.path.join(ROOT, "include", "dvd_hip.h")).read()
    for name in names:
        assert name in lib.SIGNATURES and hasattr(lib.raw(), name) and f"{name}(" in header
    assert "dvd_page_clean_workspace_bytes" in lib.NON_STATUS and lib.RESTYPES["dvd_page_clean_workspace_bytes"] is C.c_long
    assert (lib.E_CLEAN_SHAPE, lib.E_CLEAN_PARAM, lib.CLEAN_STATS) == (-61, -62, 3)
    for text in ("#define DVD_E_CLEAN_SHAPE (-61)", "#define DVD_E_CLEAN_PARAM (-62)", "#define DVD_CLEAN_STATS 3"):
        assert text in header


def test_parse_clean():
    assert ops.parse_clean("flatten") == (True, False) and ops.parse_clean("binarize") == (False, True)
    assert ops.parse_clean("flatten,binarize") == ops.parse_clean(" binarize , flatten ") == (True, True)
    for bad in ("", "flat", "flatten,flatten", "flatten;binarize", None, 3, "flatten,", ("flatten",)):
        with pytest.raises(ValueError, match="clean"):
            ops.parse_clean(bad)


# ---- the command-line tools on a stand-in for ops --------------------------------------------------------------------------------
class _Page:
    """What the tools need of a device tensor."""
    def __init__(self, a):
        self.a = np.ascontiguousarray(a)
        self.shape = self.a.shape

    def __getitem__(self, key):
        return _Page(self.a[key])

    def expand(self, *shape):
        return _Page(np.broadcast_to(self.a, shape))

    def contiguous(self):
        return _Page(self.a)


def _fake_ops(written):
    fake = types.SimpleNamespace(CLEAN_STATS=ops.CLEAN_STATS, CLEAN_CELLS=ops.CLEAN_CELLS, clean_kq=ops.clean_kq)
    fake.decode_image = lambda path, **kw: (_Page(np.load(path)), "hip")

    def page_clean(img, flatten=True, binarize=False, return_stats=False, k=0.2, **kw):
        out, stats = M.clean(img.a, flatten, binarize, kq=ops.clean_kq(k), **kw)
        return (_Page(out), stats) if return_stats else _Page(out)
    fake.page_clean = page_clean

    def to_file(img, path, **kw):
        written[os.path.basename(path)] = (img.a.copy(), kw)
        open(path, "wb").write(b"file")
        return 4
    fake.png_encode_to_file = fake.jpeg_encode_to_file = to_file
    return fake


def test_clean_pages_manifest(tmp_path, monkeypatch):
    from dvd_amd import clean_pages
    written = {}
    monkeypatch.setattr(clean_pages, "ops", _fake_ops(written))
    monkeypatch.setattr(clean_pages, "IMAGE_SUFFIXES", (".npy",))
    pages = tmp_path / "pages"
    pages.mkdir()
    imgs = {"b": X.noise(33, 31, 4), "a 1": X.text_page(97, 61)["page"]}
    for stem, img in imgs.items():
        np.save(pages / f"{stem}.npy", img)
    (pages / "notes.txt").write_text("not a page")
    lines = []
    man = clean_pages.clean_pages(str(pages), str(tmp_path / "out"), binarize=True, cell=8, radius=7, k=0.3, log=lines.append)
    assert json.loads((tmp_path / "out" / "manifest.json").read_text()) == man
    assert man["parameters"] == dict(flatten=True, binarize=True, cell=8, close=2, smooth=2, neutral=True, white=255, radius=7, k=0.3,
                                     kq=77, format="png")
    assert [d["stem"] for d in man["pages"]] == ["a 1", "b"] and sorted(os.listdir(tmp_path / "out")) == ["a 1.png", "b.png", "manifest.json"]
    for d in man["pages"]:
        img = imgs[d["stem"]]
        want, stats = M.clean(img, True, True, cell=8, radius=7, kq=77)
        assert tuple(d) == clean_pages.MANIFEST_KEYS and d["size"] == list(img.shape[:2]) and d["page"] == d["stem"] + ".png"
        assert {k: d[k] for k in M.STATS} == stats and d["bytes"] == 4
        got, _ = written[d["page"]]
        assert got.shape == img.shape and all(np.array_equal(got[..., c], want) for c in range(3))   # the plane repeated into RGB
    assert len(lines) == 2 and all("ink" in ln for ln in lines)
    with pytest.raises(ValueError, match="nothing to do"):
        clean_pages.clean_pages(str(pages), str(tmp_path / "o2"), flatten=False, binarize=False)
    with pytest.raises(ValueError, match="format"):
        clean_pages.clean_pages(str(pages), str(tmp_path / "o2"), fmt="tiff")
    with pytest.raises(ValueError, match="cell"):
        clean_pages.clean_pages(str(pages), str(tmp_path / "o2"), cell=5)
    assert not (tmp_path / "o2").exists()                         # a bad request creates nothing


def test_tools_accept_the_clean_flag_only_when_given(capsys):
    """--clean is optional: a bad value is a usage error before any file is opened."""
    from dvd_amd import apply_map, render_pages
    for tool, argv in ((apply_map, ["m.npy", "i.png", "o.png"]), (render_pages, ["maps", "img", "out"])):
        with pytest.raises(SystemExit) as e:
            tool.main(argv + ["--clean", "flat"])
        assert e.value.code == 2 and "--clean" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        apply_map.main(["m.npy", "i.png", "o.txt", "--points", "p.txt", "--clean", "flatten"])
    assert "--clean" in capsys.readouterr().err


def test_render_pages_cleans_after_the_unwarp(tmp_path):
    """render_pages(clean=...) on a stand-in device: the page is cleaned after the unwarp, the manifest names the stages and gains
    the three counts; without `clean` neither the manifest nor the log changes."""
    from PIL import Image
    from dvd_amd import render_pages
    import sized_fixtures as Z
    import sized_model as ZM

    class Backend:
        def size(self, path):
            with Image.open(path) as im:
                return im.size[1], im.size[0]

        def load(self, path):
            return np.asarray(Image.open(path).convert("RGB"))

        def render(self, flows, photos, sizes, max_radius):
            got = [ZM.unwarp(f, p, s, max_radius=max_radius) for f, p, s in zip(flows, photos, sizes)]
            return [g[0] for g in got], [g[1] for g in got]

        def write(self, page, path, fmt, quality):
            Image.fromarray(page).save(path)

        def shape(self, photo):
            return int(photo.shape[0]), int(photo.shape[1])

        def clean(self, page, flatten, binarize):
            out, counts = M.clean(page, flatten, binarize)
            return (np.repeat(out[:, :, None], 3, axis=2) if binarize else out), counts

    maps, photos = tmp_path / "pred_flow", tmp_path / "img"
    maps.mkdir()
    photos.mkdir()
    flow, src = Z.smooth_flow(8, seed=7), X.text_page(97, 61)["page"]
    np.save(maps / "flow_a.npy", flow)
    Image.fromarray(src).save(photos / "a.png")
    plain_log, clean_log = [], []
    plain = render_pages.render_pages(str(maps), str(photos), str(tmp_path / "plain"), "x0.5", log=plain_log.append, backend=Backend())
    man = render_pages.render_pages(str(maps), str(photos), str(tmp_path / "out"), "x0.5", log=clean_log.append, backend=Backend(),
                                    clean="flatten,binarize")
    assert "clean" not in plain and tuple(plain["documents"][0]) == render_pages.MANIFEST_KEYS and len(plain_log) == 1
    page, _ = ZM.unwarp(flow, src, (49, 31))
    want, stats = M.clean(page, True, True)
    doc = man["documents"][0]
    assert man["clean"] == "flatten,binarize" and tuple(doc) == render_pages.MANIFEST_KEYS + M.STATS and {k: doc[k] for k in M.STATS} == stats
    assert json.loads((tmp_path / "out" / "manifest.json").read_text()) == man
    got = np.asarray(Image.open(tmp_path / "out" / "a.png"))
    assert all(np.array_equal(got[..., c], want) for c in range(3))
    assert clean_log[0] == plain_log[0] and len(clean_log) == 2 and f"ink {stats['ink']}" in clean_log[1]
    with pytest.raises(ValueError, match="clean"):
        render_pages.render_pages(str(maps), str(photos), str(tmp_path / "bad"), "x0.5", backend=Backend(), clean="flat")
    assert not (tmp_path / "bad").exists()
