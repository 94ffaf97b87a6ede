"""Synthetic documents on the CPU: tests/synth_model.py - the definition - against float64 references, the
sanitised restatement synth_host_check.cpp against the model byte for byte, the map family, and what the library, ops and the
command line refuse without a device."""
import json
import os
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mapinv_model as M  # noqa: E402
import synth_model as Y  # noqa: E402
import synth_fixtures as X  # noqa: E402
from host_check import build_host_check  # noqa: E402
from mapinv_fixtures import AFFINE, CASES, F, SCALE, affine_inverse, model as inv_model, photograph  # noqa: E402

from dvd_amd import synth_docs as S  # noqa: E402


def _window_full(fwd):
    cov = Y.covered_of(fwd)
    return sum(Y._shift(cov, dy, dx, False).astype(int) for dy in (-1, 0, 1) for dx in (-1, 0, 1)) == 9


# ---- the filter --------------------------------------------------------------------------------------------------------------------
def test_tent_sums_to_256_r_squared_at_every_offset():
    """For an integer half-width the sampled tent's weights add up to exactly 256 r^2 whatever the sub-pixel offset, so
    W = 65536 rx^2 ry^2 is the exact weight sum and the division rounds the exact mean."""
    for r in range(1, 9):
        s = 256 * 20 + np.arange(256)
        cols, wgt = Y.tent_taps(s, r, 1000)
        assert wgt.shape == (256, 2 * r) and (wgt >= 0).all() and (wgt.sum(axis=1) == 256 * r * r).all(), r
        assert ((wgt * cols).sum(axis=1) * 256 == s * wgt.sum(axis=1)).all()              # and its centroid is the position
    flat = np.full((9, 7, 3), 201, np.uint8)                                               # replicated edges keep a flat scan flat
    sx, sy = np.array([0, 5, 256 * 6, 700]), np.array([0, 256 * 8, 3, 900])
    for r in (1, 3, 8):
        assert (Y.sample(flat, sx, sy, np.full(4, r), np.full(4, 9 - r)) == 201).all()


def test_radius_one_is_q8_bilinear():
    scan = photograph(12, 10, seed=2)
    rng = np.random.default_rng(0)
    sx, sy = rng.integers(0, 256 * 9 + 1, 300), rng.integers(0, 256 * 11 + 1, 300)
    got = Y.sample(scan, sx, sy, np.ones(300, int), np.ones(300, int))
    want = X.bilinear64(scan, sx / 256.0, sy / 256.0)
    assert np.abs(got - want).max() <= 0.5 + 1e-9                                          # the exact mean, rounded once


def test_definition_details():
    """The choices the issue leaves open, as DESIGN 4.15 states them."""
    inv = np.uint32(M.INVALID).view(F)
    fwd = np.full((3, 5, 2), inv, F)
    fwd[1, 1:4] = [[0, 0], [1.5, 0], [4, 0]]                                                # one row of three covered pixels
    sx, sy, cov = Y.scan_positions(fwd, 3, 5)
    assert cov.sum() == 3 and sx[1, 1:4].tolist() == [0, 384, 1024]
    radii, (xx, xy, yx, yy), _ = Y.footprint(fwd, 3, 5, detail=True)
    assert xx[1, 1:4].tolist() == [768, 1024, 1280] and (xy[cov] == 0).all()                   # one-sided doubled, central, one-sided
    assert radii[1, 1:4, 0].tolist() == [1, 2, 2] and radii[1, 1:4, 1].tolist() == [1, 1, 1]   # 1.5 -> 1 (a half down), 2, 2.5 -> 2
    assert (radii[~cov] == 0).all()
    assert Y.radius_of(np.array([769, 512 * 8 + 256, 512 * 9, 0]), np.array([0, 0, 0, 0])).tolist() == [2, 8, 8, 1]
    assert Y.scan_q8(np.array([np.nan, -5, np.inf, 1e9], F), F(1), 4).tolist() == [0, 0, 768, 768]   # clamped; a NaN is 0
    # coverage is fwd's first component's bits; the soft edge counts the centre
    photo = Y.render(np.full((3, 5, 3), 90, np.uint8), fwd, (0, 0, 0))
    assert photo[1, 2].tolist() == [(90 * 3 + 4) // 9] * 3 and photo[1, 1].tolist() == [(90 * 2 + 4) // 9] * 3 and (photo[0] == 0).all()
    # shading: all four zero is none, whatever a_ref; l0 = 1 alone is the identity on a covered pixel
    scan, f = X.page_scan(37, 29), X.fwd_of("smooth_37x29_g4_s3")
    plain = Y.render(scan, f, (9, 9, 9))
    assert np.array_equal(Y.render(scan, f, (9, 9, 9), dict(l0=0, lgx=0, lgy=0, k=0, a_ref=5)), plain)
    assert np.array_equal(Y.render(scan, f, (9, 9, 9), dict(l0=1, lgx=0, lgy=0, k=0, a_ref=1)), plain)
    dark = Y.render(scan, f, (9, 9, 9), dict(l0=0.5, lgx=0, lgy=0, k=0, a_ref=1))
    full = _window_full(f)
    assert np.abs(dark[full].astype(int) * 2 - plain[full]).max() <= 1
    assert Y.render(scan, f, (9, 9, 9), dict(l0=5, lgx=0, lgy=0, k=0, a_ref=1))[full].min() >= min(255, 2 * plain[full].min())   # Lq caps at 2


def test_identity_is_the_scan_shrunk_about_the_centre():
    """flow = 0, a scan of the photograph's size, no shading: the photograph is the scan shrunk by 0.987 about the centre.
    Against the float64 bilinear evaluation at the exact position, wherever the 3 x 3 window is covered, the difference is at
    most one level: half a level of the final rounding plus the Q8 position - off by at most 1/512 px per axis, plus fwd's own
    f32 error of about 1e-4 px - times the scan's slope.  With neighbouring texels at most 96 levels apart that is
    0.5 + 2 * 96 * (1 / 512 + 1e-4) = 0.9; the scans here keep to that slope."""
    fwd, (h, w) = X.fwd_of("identity_64x48"), (64, 48)
    assert set(np.unique(Y.footprint(fwd, h, w))) == {0, 1}
    py, px = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    u, v = ((2 * px / (w - 1) - 1) / SCALE + 1) / 2 * (w - 1), ((2 * py / (h - 1) - 1) / SCALE + 1) / 2 * (h - 1)
    full = _window_full(fwd)
    assert full.sum() > 0.8 * h * w
    soft_page = (X.page_scan(h, w).astype(int) * 96 // 255 + 80).astype(np.uint8)          # the text page at 96 levels of contrast
    for scan in (X.smooth_scan(h, w), soft_page):
        step = max(np.abs(np.diff(scan.astype(int), axis=0)).max(), np.abs(np.diff(scan.astype(int), axis=1)).max())
        assert step <= 96
        worst = np.abs(Y.render(scan, fwd, (0, 0, 0)).astype(np.float64) - X.bilinear64(scan, u, v))[full].max()
        print("identity: worst", worst, "largest step", step)
        assert worst <= 1.0


@pytest.mark.parametrize("mult", [1, 3])
@pytest.mark.parametrize("case", ["affine_s8", "affine_s1"])
def test_affine_against_the_analytic_inverse(case, mult):
    """The affine fixture has an exact inverse and a constant Jacobian: the model against the same tent in float64 at that
    position, with the radii the Jacobian gives, on a smooth scan.  The bar is the difference measured here plus
    one level for the Q8 positions."""
    flow, h, w, step = CASES[case]
    fwd = inv_model(case)["fwd"]
    hs, ws = h * mult, w * mult
    scan = X.smooth_scan(hs, ws)
    u, v, _ = affine_inverse(h, w)
    a0, a1, a2, b0, b1, b2 = AFFINE
    jac = np.linalg.inv(np.array([[SCALE * (1 + a1), SCALE * a2 * (w - 1) / (h - 1)], [SCALE * b1 * (h - 1) / (w - 1), SCALE * (1 + b2)]]))
    kx, ky = (ws - 1) / (w - 1), (hs - 1) / (h - 1)
    rx = int(np.clip(np.ceil(np.abs(jac[0]).max() * kx - 0.5), 1, 8))
    ry = int(np.clip(np.ceil(np.abs(jac[1]).max() * ky - 0.5), 1, 8))
    assert (rx, ry) == (mult, mult)
    inside = _window_full(fwd) & (u >= 0) & (u <= w - 1) & (v >= 0) & (v <= h - 1)
    assert inside.sum() > 0.7 * h * w
    radii = Y.footprint(fwd, hs, ws)
    assert (radii[inside] == [rx, ry]).all()
    at = np.nonzero(inside)
    worst = np.abs(Y.render(scan, fwd, (0, 0, 0))[at].astype(np.float64) - X.tent64(scan, (u * kx)[at], (v * ky)[at], rx, ry)).max()
    print(case, mult, "worst", worst, "measured", X.AFFINE_MEASURED[mult])
    assert worst <= X.AFFINE_MEASURED[mult] + 1.0


def test_cycle_returns_the_scan():
    """unwarp(flow, render(scan, flow)) against the scan - the truth - over the page pixels at least 2 px inside, as the mean
    absolute difference in levels.  Two bilinear resamplings blur a text page of this size, which is most of the figure; the
    bar, 1.5 x the value recorded from this model, guards the fixture.  The finer mesh inverts no worse."""
    got = {}
    for case in X.CYCLE_MEASURED:
        flow, h, w, step = CASES[case]
        scan = X.page_scan(h, w)
        photo = Y.render(scan, inv_model(case)["fwd"], (128, 128, 128))
        got[case] = X.cycle_difference(scan, X.unwarp_model(flow, photo))
        print(case, "cycle", got[case], "recorded", X.CYCLE_MEASURED[case])
        assert got[case] <= X.CYCLE_BAR * X.CYCLE_MEASURED[case]
    assert got["smooth_64x48_g9_s1"] <= got["smooth_64x48_g9_s8"] and got["smooth_96x80_g16_s1"] <= got["smooth_96x80_g16_s8"]


# ---- the sanitised CPU restatement ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("synth_host_check")
    exe = build_host_check("synth", tmp)

    def run(scan, fwd, background, shading, sizes=None):
        hs, ws, h, w = sizes if sizes else (*scan.shape[:2], *fwd.shape[:2])
        plane = not isinstance(background, tuple)
        color = 0 if plane else background[0] | background[1] << 8 | background[2] << 16
        prm = shading or Y.NO_SHADING
        head = struct.pack("<5iI5f", hs, ws, h, w, int(plane), color, *(prm[k] for k in ("l0", "lgx", "lgy", "k", "a_ref")))
        data = head + np.ascontiguousarray(scan, np.uint8).tobytes() + np.ascontiguousarray(fwd, F).tobytes() + \
            (np.ascontiguousarray(background, np.uint8).tobytes() if plane else b"")
        (tmp / "in.bin").write_bytes(data)
        out = tmp / "out.bin"
        if out.exists():
            out.unlink()
        p = subprocess.run([str(exe), str(tmp / "in.bin"), str(out)], capture_output=True, text=True)
        assert p.returncode == 0 and p.stderr == "", (p.returncode, p.stderr[-2000:])      # a status, never a sanitizer report
        return int(p.stdout), (out.read_bytes() if out.exists() else None)
    return run


@pytest.mark.parametrize("name", list(X.RENDER_CASES))
def test_host_check_equals_the_model(host_check, name):
    c = X.render_case(name)
    h, w = c["fwd"].shape[:2]
    status, out = host_check(c["scan"], c["fwd"], c["background"], c["shading"])
    assert status == 0 and len(out) == 5 * h * w
    assert np.array_equal(np.frombuffer(out, np.uint8, 3 * h * w).reshape(h, w, 3), c["photo"])               # byte for byte
    assert np.array_equal(np.frombuffer(out, np.uint8, 2 * h * w, 3 * h * w).reshape(h, w, 2), c["radii"])


def test_cases_cover_what_they_are_named_for():
    covered = lambda name: X.render_case(name)["radii"][..., 0] > 0                           # noqa: E731
    for name in ("smooth_37x29", "smooth_96x80", "edge_33x31", "magnify"):
        r = X.render_case(name)["radii"]
        assert covered(name).sum() > 100 and (r[covered(name)] == 1).all(), name
    r = X.render_case("minify_3")["radii"][covered("minify_3")]
    assert r.max() < Y.MAX_RADIUS and len(np.unique(r[r > 1])) >= 2                              # mixed radii, none at the cap
    assert (X.render_case("minify_10")["radii"][covered("minify_10")] == Y.MAX_RADIUS).all()
    assert set(np.unique(X.render_case("folded")["radii"][..., 0])) == set(range(9))
    for name in ("uncovered", "thin_1x40", "tall_40x1"):
        c = X.render_case(name)
        assert not covered(name).any() and np.array_equal(c["photo"], np.broadcast_to(np.asarray(c["background"], np.uint8), c["photo"].shape))
    assert covered("hand_1x40").sum() == covered("hand_40x1").sum() == 37
    a, b = X.render_case("smooth_96x80")["photo"], X.render_case("smooth_96x80_shaded")["photo"]
    assert not np.array_equal(a, b)


def test_host_check_refuses_with_a_status(host_check):
    scan, fwd = np.zeros((4, 4, 3), np.uint8), np.zeros((5, 5, 2), F)
    for sizes in ((0, 4, 5, 5), (4, 16385, 5, 5), (4, 4, 0, 5), (4, 4, 5, 16385), (-1, 4, 5, 5)):
        assert host_check(scan, fwd, (0, 0, 0), None, sizes) == (-57, None)
    for bad in (dict(l0=np.nan), dict(lgx=np.inf), dict(k=-np.inf), dict(a_ref=np.nan), dict(l0=1.0, a_ref=0.0), dict(k=0.5, a_ref=-1.0)):
        assert host_check(scan, fwd, (0, 0, 0), dict(Y.NO_SHADING, **bad)) == (-58, None)
    status, out = host_check(scan, fwd, (0, 0, 0), dict(Y.NO_SHADING, a_ref=0.0))              # no shading: a_ref is not read
    assert status == 0 and len(out) == 125


# ---- the library's and the wrappers' refusals: before any launch, so they run here ------------------------------------------------
def test_entry_points_refuse_before_any_launch():
    import ctypes as C
    from dvd_amd import lib
    raw = lib.raw()
    prm = lib.SynthParams(0, 0, 0, 0, 1)
    for hs, ws, h, w in ((0, 4, 5, 5), (4, 16385, 5, 5), (4, 4, 0, 5), (4, 4, 5, 16385)):
        assert raw.dvd_synth_render_rgb8(None, hs, ws, None, h, w, None, 0, C.byref(prm), None, None) == -57
        assert b"synth_render_rgb8" in raw.dvd_last_error() and b"sides" in raw.dvd_last_error()
        assert raw.dvd_synth_footprint(None, h, w, hs, ws, None, None) == -57
    assert raw.dvd_synth_render_rgb8(None, 4, 4, None, 5, 5, None, 0, C.byref(prm), None, None) == -1 and b"null" in raw.dvd_last_error()
    assert raw.dvd_synth_footprint(None, 5, 5, 4, 4, None, None) == -1 and b"null" in raw.dvd_last_error()
    buf = (C.c_char * 512)()
    base = (C.addressof(buf) + 63) & ~63                                                      # host memory: never dereferenced
    for bad in (lib.SynthParams(float("nan"), 0, 0, 0, 1), lib.SynthParams(1, float("inf"), 0, 0, 1), lib.SynthParams(1, 0, 0, 0, 0),
                lib.SynthParams(0, 0, 0, 0, float("nan"))):
        assert raw.dvd_synth_render_rgb8(base, 4, 4, base + 64, 5, 5, None, 0, C.byref(bad), base + 256, None) == -58
        assert b"a_ref" in raw.dvd_last_error()
    assert raw.dvd_synth_render_rgb8(base, 4, 4, base + 68, 5, 5, None, 0, C.byref(prm), base + 256, None) == -1      # fwd off 8 bytes
    assert b"misaligned" in raw.dvd_last_error()
    assert raw.dvd_synth_render_rgb8(base, 4, 4, base + 64, 5, 8, None, 0, C.byref(prm), base + 257, None) == -1      # w % 4 == 0: dwords
    assert raw.dvd_synth_render_rgb8(base, 4, 4, base + 64, 5, 8, None, 0, C.byref(prm), base, None) == -1 and b"out must not" in raw.dvd_last_error()
    assert raw.dvd_synth_footprint(base + 4, 5, 5, 4, 4, base + 256, None) == -1
    assert (lib.E_SYNTH_SHAPE, lib.E_SYNTH_PARAM) == (-57, -58)


def test_ops_refuse_bad_arguments_and_host_tensors():
    from dvd_amd import lib, ops
    scan, fwd, flow = torch.zeros(6, 5, 3, dtype=torch.uint8), torch.zeros(5, 7, 2), torch.zeros(2, 8, 8)
    for call in (lambda: ops.synth_render(scan, fwd), lambda: ops.synth_footprint((6, 5), fwd), lambda: ops.synth_document(scan, flow, 5, 7)):
        with pytest.raises(lib.DvdError, match="on the device"):                             # host tensors: no CPU path
            call()
    for bad in ("scan", np.zeros((6, 5, 3), np.uint8)):
        with pytest.raises(ValueError, match="synth_render: scan_u8 must be a"):
            ops.synth_render(bad, fwd)
    for bad in ((6,), (6, 5.0), "6x5", (True, 5)):
        with pytest.raises(ValueError, match="synth_footprint: scan_hw"):
            ops.synth_footprint(bad, fwd)
    with pytest.raises(ValueError, match="synth_footprint: the sides"):
        ops.synth_footprint((0, 5), fwd)
    for bad in (dict(l0=float("nan")), dict(k="1"), dict(gamma=1), dict(l0=True), dict(a_ref=0.0), dict(lgx=1e39), [1, 0, 0, 0]):
        with pytest.raises(ValueError, match="shading"):
            ops.synth_shading(bad)
    assert ops.synth_shading(None) == dict(l0=0.0, lgx=0.0, lgy=0.0, k=0.0, a_ref=1.0)
    assert ops.synth_shading(dict(k=-0.5)) == dict(l0=1.0, lgx=0.0, lgy=0.0, k=-0.5, a_ref=None)
    assert ops.SYNTH_MAX_RADIUS == Y.MAX_RADIUS and ops.SYNTH_SHADING == ("l0", "lgx", "lgy", "k", "a_ref")


# ---- the map family ----------------------------------------------------------------------------------------------------------------
def test_maps_are_keyed():
    key = S.document_key(7, "a.png")
    assert key == (7, __import__("zlib").crc32(b"a.png"))
    for kind in S.KINDS:
        a, b = S.make_map(key, 16, kind, 3), S.make_map(key, 16, kind, 3)
        assert a.dtype == F and a.shape == (2, 16, 16) and a.tobytes() == b.tobytes()
        others = [S.make_map(S.document_key(7, "b.png"), 16, kind, 3), S.make_map(S.document_key(8, "a.png"), 16, kind, 3),
                  S.make_map(key, 16, kind, 3, attempt=1), S.make_map(key, 16, kind, 2)]
        assert all(o.tobytes() != a.tobytes() for o in others)
    for bad in (dict(g=1), dict(kind="fold"), dict(strength=0), dict(strength=6), dict(margin=0.5), dict(g=2.0)):
        with pytest.raises(ValueError, match="make_map"):
            S.make_map(key, **{**dict(g=16, kind="tilt", strength=3), **bad})


@pytest.mark.parametrize("kind", S.KINDS)
def test_maps_keep_the_margin(kind):
    """Every sampled position lies at least `margin` of the side inside the frame: at the grid's nodes in float64 on the f32
    map - between them the positions are bilinear, a convex combination - and so at every pixel of the f32 pipeline."""
    for strength in range(1, 6):
        for n, margin in ((0, 0.04), (1, 0.1)):
            flow = S.make_map(S.document_key(n, kind), 9, kind, strength, margin)
            t = np.linspace(0, 1, 9)
            q = (np.stack(np.meshgrid(t, t, indexing="xy")) + flow.astype(np.float64)) * 2 - 1                 # [-1, 1] before the scale
            pos = (q * SCALE + 1) / 2
            assert pos.min() >= margin and pos.max() <= 1 - margin, (strength, pos.min(), pos.max())
            x, y = M.positions(flow, 40, 30, SCALE)
            assert x.min() >= margin * 29 - 1e-3 and x.max() <= (1 - margin) * 29 + 1e-3 and y.min() >= margin * 39 - 1e-3 and \
                y.max() <= (1 - margin) * 39 + 1e-3


@pytest.mark.parametrize("kind", S.KINDS)
def test_accepted_maps_do_not_fold(kind):
    seen = []
    for n in range(20):
        accept = lambda flow: M.invert(flow, 64, 48, 8, SCALE)[1]                              # noqa: E731
        flow, stats, record = S.draw_accepted(S.document_key(n, f"doc_{n}"), accept, 9, kind, 5)
        assert all(stats[k] == 0 for k in S.ACCEPT_ZERO) and stats["covered"] > 0.3 * 64 * 48
        assert M.invert(flow, 64, 48, 1, SCALE)[1]["fold_px"] == 0                              # nor under the finest mesh
        seen.append(record)
    assert all(r["attempts"] >= 1 and r["strength"] == 5 / 2 ** r["halvings"] for r in seen)


def test_rejected_maps_are_redrawn_then_weakened():
    calls = []

    def accept(flow):
        calls.append(flow)
        return {k: int(len(calls) <= S.MAX_ATTEMPTS + 2) for k in S.ACCEPT_ZERO}
    key = S.document_key(0, "x")
    flow, stats, record = S.draw_accepted(key, accept, 8, "wave", 4)
    assert record == {"attempts": S.MAX_ATTEMPTS + 3, "halvings": 1, "strength": 2.0}
    assert flow.tobytes() == S.make_map(key, 8, "wave", 2.0, attempt=S.MAX_ATTEMPTS + 2).tobytes()
    assert len({c.tobytes() for c in calls}) == len(calls)


def test_procedural_page_is_keyed_and_looks_like_text():
    key = S.document_key(1, "page_00000")
    a = S.procedural_page(key, 64, 48)
    assert a.dtype == np.uint8 and a.shape == (64, 48, 3) and np.array_equal(a, S.procedural_page(key, 64, 48))
    assert not np.array_equal(a, S.procedural_page(S.document_key(1, "page_00001"), 64, 48))
    gray = a.astype(int).sum(axis=2)
    assert (gray > 3 * 225).mean() > 0.4 and (gray < 3 * 100).mean() > 0.03                     # mostly paper, some ink
    assert (a[:5] == a[0, 0]).all() and (a[:, :4] == a[0, 0]).all()                            # margins
    with pytest.raises(ValueError, match="procedural_page"):
        S.procedural_page(key, 4, 48)


# ---- the command line --------------------------------------------------------------------------------------------------------------
def test_cli_refuses_bad_arguments(tmp_path, capsys):
    (tmp_path / "scans").mkdir()
    out = str(tmp_path / "out")
    for argv, text in ((["-", out, "--size", "64"], "--size must be HxW"), (["-", out, "--size", "4x64"], "sides 8..16384"),
                       (["-", out, "--size", "64x48", "--procedural", "2", "--kinds", "tilt,fold"], "--kinds"),
                       (["-", out, "--size", "64x48", "--procedural", "2", "--strength", "6"], "--strength must be an integer 1..5"),
                       (["-", out, "--size", "64x48", "--procedural", "2", "--g", "1"], "--g must be"),
                       (["-", out, "--size", "64x48", "--procedural", "2", "--quality", "0"], "--quality"),
                       (["-", out, "--size", "64x48", "--procedural", "2", "--step", "0"], "--step"),
                       (["-", out, "--size", "64x48", "--procedural", "2", "--shading", "1,2,3"], "--shading must be four"),
                       (["-", out, "--size", "64x48", "--procedural", "2", "--shading", "1,nan,0,0"], "--shading must be four"),
                       (["-", out, "--size", "64x48", "--procedural", "2", "--background", "1,2,300"], "--background R,G,B"),
                       (["-", out, "--size", "64x48", "--procedural", "2", "--background", str(tmp_path / "none.png")], "--background must be"),
                       (["-", out, "--size", "64x48", "--procedural", "-1"], "--procedural"),
                       (["-", out, "--size", "64x48"], "SCANS_DIR must be"),
                       ([str(tmp_path / "scans"), out, "--size", "64x48"], "holds no image file"),
                       ([str(tmp_path / "scans"), out, "--size", "64x48", "--procedural", "2"], "--procedural draws its own pages"),
                       (["-", out, "--size", "64x48", "--procedural", "2", "--format", "gif"], "invalid choice")):
        with pytest.raises(SystemExit) as e:
            S.main(argv)
        assert e.value.code == 2 and text in capsys.readouterr().err, argv
    assert not os.path.exists(out)                                                             # refused before anything is written
    assert S.parse_background("noise") == ("noise", None) and S.parse_background("1,2,3") == ("color", (1, 2, 3))
    assert S.parse_shading("") is None and S.parse_shading("1,0.2,0,-0.5") == dict(l0=1.0, lgx=0.2, lgy=0.0, k=-0.5)


class ModelBackend:
    """write_dataset's device, played by the NumPy models: what the manifest and the file layout need, without a GPU."""

    def upload(self, array):
        return np.ascontiguousarray(array)

    def document(self, scan, flow, h, w, step, background, shading):
        fwd, stats = M.invert(flow, h, w, step, SCALE)[:2]
        prm = None if shading is None else dict(dict(l0=1.0, lgx=0.0, lgy=0.0, k=0.0), **shading, a_ref=scan.shape[0] * scan.shape[1] / max(stats["covered"], 1))
        return Y.render(scan, fwd, background, prm), fwd, stats

    def at_cap(self, scan_hw, fwd):
        return int((Y.footprint(fwd, *scan_hw).max(axis=2) == Y.MAX_RADIUS).sum())

    def write_image(self, img, path, fmt="png", quality=90):
        from PIL import Image
        Image.fromarray(img).save(path, quality=quality) if fmt == "jpeg" else Image.fromarray(img).save(path)

    def write_flo(self, flow, h, w, path):
        from dvd_amd import ops
        x, y = M.positions(flow, h, w, 1.0)
        ops.flo_write(np.stack([x - np.arange(w, dtype=F)[None, :], y - np.arange(h, dtype=F)[:, None]], axis=-1).astype(F), path)


def test_dataset_layout_and_manifest_schema(tmp_path):
    from PIL import Image
    from dvd_amd import evaluation
    scans = tmp_path / "scans"
    scans.mkdir()
    for name, size in (("b_scan.png", (90, 70)), ("a_scan.jpg", (64, 48))):
        Image.fromarray(X.page_scan(*size)).save(scans / name)
    lines = []
    man = S.write_dataset(str(scans), str(tmp_path / "out"), (64, 48), g=9, kinds=("curl", "mixed"), strength=2, seed=3, fmt="png",
                          shading=dict(k=-0.4), background="noise", log=lines.append, backend=ModelBackend())
    assert json.loads((tmp_path / "out" / "manifest.json").read_text()) == man and len(lines) == 2
    assert set(man) == {"seed", "format", "quality", "scale", "margin", "shading", "background", "documents"}
    assert [d["stem"] for d in man["documents"]] == ["a_scan", "b_scan"] and [d["kind"] for d in man["documents"]] == ["curl", "mixed"]
    for d in man["documents"]:
        assert tuple(d) == S.MANIFEST_KEYS
        assert d["key"] == list(S.document_key(3, d["stem"])) and d["strength_asked"] == 2 and d["attempts"] >= 1 and d["halvings"] >= 0
        assert d["strength"] == 2 / 2 ** d["halvings"] and d["size"] == [64, 48] and d["g"] == 9 and d["step"] == 8
        assert set(d["stats"]) == {"covered", "fold_px", "flipped_tris", "degenerate_tris", "skipped_tris", "tris"}
        assert all(d["stats"][k] == 0 for k in S.ACCEPT_ZERO) and 0 <= d["cap_share"] <= 1
        for k in ("image", "scan", "map", "flo"):
            assert (tmp_path / "out" / d[k]).is_file()
        flow = np.load(tmp_path / "out" / d["map"])
        assert flow.dtype == F and flow.shape == (2, 9, 9)
        assert flow.tobytes() == S.make_map(tuple(d["key"]), 9, d["kind"], d["strength"], attempt=d["attempts"] - 1).tobytes()
        # the names the document loop looks for
        photo = str(tmp_path / "out" / d["image"])
        assert evaluation.find_gt_map(str(tmp_path / "out" / "map"), photo) == str(tmp_path / "out" / "map" / (d["stem"] + ".flo"))
        assert evaluation.find_gt(str(tmp_path / "out" / "scan"), photo) == str(tmp_path / "out" / d["scan"])
        assert np.asarray(Image.open(photo)).shape == (64, 48, 3)
    assert man["documents"][1]["scan_size"] == [90, 70]
    assert sorted(os.listdir(tmp_path / "out" / "img")) == ["a_scan.png", "b_scan.png"]
