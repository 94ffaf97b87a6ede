"""The map inverse without a GPU: the NumPy model against what it has to deliver (no fold on smooth maps, the
coverage of exact rational arithmetic, second-order convergence, an analytic inverse, the smallest id on folds, hostile maps), the
sanitised CPU restatement against the model byte for byte, the library's refusals, settings.inverse_outputs from the launcher to
the document loop, the table's text, the .flo file and apply_map --points."""
import os
import struct
import subprocess
import sys
import types
from fractions import Fraction

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mapinv_model as M  # noqa: E402
from host_check import build_host_check  # noqa: E402

from mapinv_fixtures import CASES, F, OVERLAYS, SCALE, SMOOTH, affine_inverse, model, photograph, points  # noqa: E402

SMOOTH_NAMES = [f"smooth_{h}x{w}_g{g}_s{step}" for h, w, g, step, _ in SMOOTH]
# measured on the model (printed by the tests below); the bars are 4 x these
AFFINE_WORST = {"affine_s8": 0.00184, "affine_s1": 0.00179}       # pixels of the page, against the float64 analytic inverse
CYCLE_MEAN = {8: 0.0950, 4: 0.0247, 2: 0.0062, 1: 0.0012}          # 64 x 48, g = 9: cycle_mean per step


# ---- the definition -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SMOOTH_NAMES)
def test_smooth_maps_do_not_fold(name):
    m = model(name)
    s, count = m["stats"], m["detail"][3]
    print(name, s, f"covered {s['covered'] / count.size:.3f}")
    assert s["fold_px"] == 0 and s["flipped_tris"] == s["degenerate_tris"] == s["skipped_tris"] == 0
    assert count.max() == 1                                          # the top-left rule: no pixel is covered twice
    assert s["covered"] == int((count == 1).sum()) and 0.85 < s["covered"] / count.size < 0.97
    assert np.array_equal(M.covered_of(m["fwd"]), count == 1)


def _fraction_cover(lat, h, w):
    """The pixel centres inside some triangle of the mesh, by exact rational arithmetic and the stated tie rule."""
    R, C = len(lat["rows"]), len(lat["cols"])
    P = [[(Fraction(int(lat["qx"][r, c]), 256), Fraction(int(lat["qy"][r, c]), 256)) for c in range(C)] for r in range(R)]
    inside = np.zeros((h, w), int)
    for r in range(R - 1):
        for c in range(C - 1):
            a, b, cc, d = P[r][c], P[r][c + 1], P[r + 1][c], P[r + 1][c + 1]
            for tri in ((a, b, cc), (cc, b, d)):
                area = (tri[1][0] - tri[0][0]) * (tri[2][1] - tri[0][1]) - (tri[1][1] - tri[0][1]) * (tri[2][0] - tri[0][0])
                assert area > 0
                xs, ys = [p[0] for p in tri], [p[1] for p in tri]
                for y in range(max(int(min(ys)) - 1, 0), min(int(max(ys)) + 2, h)):
                    for x in range(max(int(min(xs)) - 1, 0), min(int(max(xs)) + 2, w)):
                        ok = True
                        for k in range(3):
                            p, q = tri[k], tri[(k + 1) % 3]
                            e = (q[0] - p[0]) * (y - p[1]) - (q[1] - p[1]) * (x - p[0])
                            # on the edge: it counts when the edge runs upward, or is horizontal and runs to the right
                            ok = ok and (e > 0 or (e == 0 and (q[1] < p[1] or (q[1] == p[1] and q[0] > p[0]))))
                        inside[y, x] += ok
    return inside


@pytest.mark.parametrize("name", SMOOTH_NAMES[:2])
def test_coverage_equals_an_exact_rational_count(name):
    _, h, w, _ = CASES[name]
    m = model(name)
    assert np.array_equal(_fraction_cover(m["detail"][0], h, w), m["detail"][3])


def test_cycle_error_converges_at_second_order():
    got = {step: model(f"smooth_64x48_g9_s{step}")["cycle"]["cycle_mean"] for step in (8, 4, 2, 1)}
    print("cycle_mean per step:", got)
    assert got[8] / got[4] >= 3 and got[4] / got[2] >= 3          # triangle interpolation of a smooth map: a factor 4
    assert got[1] <= got[2]                                        # at step 1 the Q8 quantisation (1/256 px) is the floor
    for step, want in CYCLE_MEAN.items():
        assert abs(got[step] - want) < 1e-4


@pytest.mark.parametrize("name", ["affine_s8", "affine_s1"])
def test_affine_map_against_its_analytic_inverse(name):
    _, h, w, _ = CASES[name]
    fwd = model(name)["fwd"]
    u, v, norm = affine_inverse(h, w)
    cov = M.covered_of(fwd)
    worst = float(np.maximum(np.abs(fwd[..., 0] - u), np.abs(fwd[..., 1] - v))[cov].max())
    bar = 4 * AFFINE_WORST[name]
    print(name, "worst", worst, "bar", bar, "quantisation bound", 2.0 ** -7 * norm)
    assert cov.sum() > 0.9 * h * w and worst <= bar < 2.0 ** -7 * norm


def _all_covering(t, h, w):
    """Per pixel the sorted ids of every rasterised triangle that covers it, by brute force over the whole image."""
    py, px = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    ids = [[[] for _ in range(w)] for _ in range(h)]
    for k in np.flatnonzero(t["kind"] <= 1):
        inside, _ = M.covers(t, k, px, py)
        for y, x in zip(*np.nonzero(inside)):
            ids[y][x].append(int(k))
    return ids


@pytest.mark.parametrize("name", ["folded", "far"])
def test_on_a_fold_the_smallest_id_wins(name):
    _, h, w, _ = CASES[name]
    m = model(name)
    _, t, win, count = m["detail"]
    assert m["stats"]["flipped_tris"] > 0 and m["stats"]["fold_px"] > 0
    ids = _all_covering(t, h, w)
    folds = 0
    for y in range(h):
        for x in range(w):
            assert len(ids[y][x]) == count[y, x]
            assert win[y, x] == (min(ids[y][x]) if ids[y][x] else M.INVALID)
            folds += len(ids[y][x]) >= 2
    assert folds == m["stats"]["fold_px"]


def test_collapsed_map_is_all_degenerate():
    m = model("collapsed")
    s = m["stats"]
    assert s["degenerate_tris"] == s["tris"] == 96 and s["covered"] == s["fold_px"] == s["flipped_tris"] == s["skipped_tris"] == 0
    assert (m["fwd"].view(np.uint32) == M.INVALID).all()
    assert np.isnan(m["cycle"]["cycle_mean"]) and m["cycle"]["n"] == 0
    lat = m["detail"][0]
    assert len(set(lat["qx"].reshape(-1).tolist())) == 1 and len(set(lat["qy"].reshape(-1).tolist())) == 1


@pytest.mark.parametrize("name", ["nan", "inf", "huge", "far"])
def test_hostile_maps_are_skipped_not_followed(name):
    _, h, w, step = CASES[name]
    m = model(name)
    lat, t, win, _ = m["detail"]
    ok = lat["valid"]
    # a triangle is skipped for an invalid vertex: cells touching one lose both triangles but for the corner the other half owns
    cell_bad = ~(ok[:-1, :-1] & ok[:-1, 1:] & ok[1:, :-1])                       # (a, b, c)
    cell_bad2 = ~(ok[1:, :-1] & ok[:-1, 1:] & ok[1:, 1:])                        # (c, b, d)
    by_vertex = int(cell_bad.sum() + cell_bad2.sum())
    box = t["box"]
    held = np.clip(box[:, 1] - box[:, 0] + 1, 0, None) * np.clip(box[:, 3] - box[:, 2] + 1, 0, None)
    bad_vertex = np.stack([cell_bad.reshape(-1), cell_bad2.reshape(-1)], axis=1).reshape(-1)
    by_box = int((~bad_vertex & (t["area"] != 0) & (held > M.budget(step))).sum())
    print(name, m["stats"], "by vertex", by_vertex, "by box", by_box)
    assert m["stats"]["skipped_tris"] == by_vertex + by_box > 0
    assert (by_vertex > 0) == (name != "far") and (by_box > 0) == (name == "far")
    assert (t["kind"] == 3).sum() == by_vertex + by_box and not np.isin(win[win != M.INVALID], np.flatnonzero(t["kind"] >= 2)).any()
    live = t["kind"] <= 1
    assert (held[live] <= M.budget(step)).all()                                    # the work of a triangle is bounded
    assert np.isfinite(m["fwd"][M.covered_of(m["fwd"])]).all()


def test_definition_details():
    assert M.lattice_axis(17, 8).tolist() == [0, 8, 16] and M.lattice_axis(18, 8).tolist() == [0, 8, 16, 17]
    assert M.lattice_axis(1, 3).tolist() == [0] and M.lattice_axis(5, 1).tolist() == [0, 1, 2, 3, 4]
    assert M.budget(1) == 1024 and M.budget(4) == 1024 and M.budget(8) == 4096
    # two triangles that share an edge through pixel centres: every centre on it belongs to exactly one
    lat = {"rows": np.array([0, 4]), "cols": np.array([0, 4]), "valid": np.ones((2, 2), bool),
           "qx": np.array([[256, 5 * 256], [256, 5 * 256]]), "qy": np.array([[256, 256], [5 * 256, 5 * 256]])}
    t = M.triangles(lat, 8, 8, 4)
    win, cnt = M.rasterise(t, 8, 8)
    assert cnt[1:5, 1:5].tolist() == [[1] * 4] * 4 and cnt.sum() == 16      # the top and left border in, the bottom and right out
    assert win[1, 1] == 0 and win[4, 1] == 0 and win[1, 4] == 0 and win[4, 4] == 1 and win[2, 3] == 0 and win[3, 3] == 1   # diagonal: lower id's left edge
    fwd = M.resolve(t, win)
    assert fwd[1, 1].tolist() == [0, 0] and fwd[3, 2].tolist() == [1, 2] and fwd[4, 4].tolist() == [3, 3]
    # a mirrored mesh: every triangle flipped, the same coverage
    lat["qx"] = lat["qx"][:, ::-1].copy()
    t = M.triangles(lat, 8, 8, 4)
    assert (t["kind"] == 1).all() and (t["area"] > 0).all()
    _, cnt2 = M.rasterise(t, 8, 8)
    assert cnt2.sum() == 16 and cnt2.max() == 1
    # the f64 sum's order is the kernels', its value the exact one to rounding
    v = np.random.default_rng(3).random(300000)
    assert abs(M.ordered_sum(v) - float(np.sum(v))) < 1e-7 and M.ordered_sum(np.zeros(0)) == 0.0


def test_overlay_and_points_model():
    name = "smooth_37x29_g4_s3"
    _, h, w, _ = CASES[name]
    fwd = model(name)["fwd"]
    src = photograph(h, w)
    cov = M.covered_of(fwd)
    thin = M.mesh_overlay(src, fwd, lines=5)
    changed = (thin != src).any(axis=2)
    assert changed.any() and not changed[~cov].any()
    red, green = (thin == (255, 0, 0)).all(axis=2), (thin == (0, 255, 0)).all(axis=2)
    assert green[cov & ~np.pad(cov, 1)[2:, 1:-1]].all() and 0 < (red & ~green).sum() < cov.sum() / 2
    wide = M.mesh_overlay(src, fwd, lines=5, thickness=3, dim=True)
    assert ((wide == (0, 255, 0)).all(axis=2) >= green).all() and (wide == (0, 255, 0)).all(axis=2).sum() > green.sum()
    far = ~cov & ~(wide != src >> 1).any(axis=2)
    assert far.any() and np.array_equal(wide[far], src[far] >> 1)
    pts = points(h, w)
    got = M.transfer_points(fwd, pts).view(np.uint32)
    assert (got[2] == M.INVALID).all() and (got[3] == M.INVALID).all()            # NaN, inf
    outside = (pts[:, 0] < 0) | (pts[:, 0] > w - 1) | (pts[:, 1] < 0) | (pts[:, 1] > h - 1)
    assert (got[outside] == M.INVALID).all() and (got[~outside & np.isfinite(pts).all(axis=1)] != M.INVALID).any()
    back = M.map_points(CASES[name][0], pts, h, w).view(np.uint32)
    assert (back[2] == M.INVALID).all() and (back[5:] != M.INVALID).all()
    # a covered pixel centre transfers to fwd itself
    y, x = np.argwhere(cov)[len(np.argwhere(cov)) // 2]
    assert np.array_equal(M.transfer_points(fwd, np.array([[x, y]], F))[0], fwd[y, x])


# ---- the sanitised CPU restatement ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("mapinv_host_check")
    exe = build_host_check("mapinv", tmp)

    def run(flow, h, w, step, src, photo_pts, page_pts, lines=17, thickness=1, dim=False, color=0x0000ff, outline=0x00ff00, g=None):
        flow = np.ascontiguousarray(flow, F)
        head = struct.pack("<9i2If", flow.shape[-1] if g is None else g, h, w, step, lines, thickness, int(dim), len(photo_pts), len(page_pts),
                           color, outline, SCALE)
        data = head + flow.tobytes() + np.ascontiguousarray(photo_pts, F).tobytes() + np.ascontiguousarray(page_pts, F).tobytes() + \
            np.ascontiguousarray(src, np.uint8).tobytes()
        (tmp / "in.bin").write_bytes(data)
        out = tmp / "out.bin"
        if out.exists():
            out.unlink()
        p = subprocess.run([str(exe), str(tmp / "in.bin"), str(out)], capture_output=True, text=True)
        assert p.returncode == 0 and p.stderr == "", (p.returncode, p.stderr[-2000:])      # a status, never a sanitizer report
        return int(p.stdout), (out.read_bytes() if out.exists() else None)
    return run


def _rgb(c):
    return c[0] | c[1] << 8 | c[2] << 16


@pytest.mark.parametrize("name", list(CASES))
def test_host_check_equals_the_model(host_check, name):
    flow, h, w, step = CASES[name]
    m = model(name)
    lat = m["detail"][0]
    src, pts = photograph(h, w), points(h, w)
    for k, ov in enumerate(OVERLAYS if name in ("smooth_37x29_g4_s3", "folded", "nan") else OVERLAYS[:1]):
        color, outline = ov.get("color", (255, 0, 0)), ov.get("outline_color", (0, 255, 0))
        status, out = host_check(flow, h, w, step, src, pts, pts, ov["lines"], ov["thickness"], ov["dim"], _rgb(color), _rgb(outline))
        assert status == 0
        nv, n, at = lat["qx"].size, h * w, 0
        verts = np.frombuffer(out, np.int32, 2 * nv, at).reshape(-1, 2)
        at += 8 * nv
        valid = np.frombuffer(out, np.uint8, nv, at)
        at += nv
        fwd = np.frombuffer(out, np.uint32, 2 * n, at).reshape(h, w, 2)
        at += 8 * n
        stats = np.frombuffer(out, np.uint64, 6, at)
        at += 48
        cyc = np.frombuffer(out, np.uint64, 3, at)
        at += 24
        picture = np.frombuffer(out, np.uint8, 3 * n, at).reshape(h, w, 3)
        at += 3 * n
        to_page = np.frombuffer(out, np.uint32, 2 * len(pts), at).reshape(-1, 2)
        at += 8 * len(pts)
        to_photo = np.frombuffer(out, np.uint32, 2 * len(pts), at).reshape(-1, 2)
        assert at + 8 * len(pts) == len(out)
        assert np.array_equal(verts[:, 0], lat["qx"].reshape(-1)) and np.array_equal(verts[:, 1], lat["qy"].reshape(-1))
        assert np.array_equal(valid != 0, lat["valid"].reshape(-1))
        assert np.array_equal(fwd, m["fwd"].view(np.uint32))                                        # bit for bit
        assert stats.tolist() == [m["stats"][k] for k in ("covered", "fold_px", "flipped_tris", "degenerate_tris", "skipped_tris", "tris")]
        c = m["cycle"]
        assert int(cyc[0]) == c["n"] and cyc[1:2].view(np.float64)[0] == c["sum"]
        assert cyc[2:3].view(np.uint32)[:1].view(F)[0] == (F(c["cycle_max"]) if c["n"] else F(0))
        assert np.array_equal(picture, M.mesh_overlay(src, m["fwd"], ov["lines"], ov["thickness"], color, outline, ov["dim"])), k
        assert np.array_equal(to_page, M.transfer_points(m["fwd"], pts).view(np.uint32))
        assert np.array_equal(to_photo, M.map_points(flow, pts, h, w, SCALE, pos=m["pos"]).view(np.uint32))


def test_host_check_refuses_with_a_status(host_check):
    flow, src, none = np.zeros((2, 4, 4), F), np.zeros((5, 5, 3), np.uint8), np.zeros((0, 2), F)
    for h, w in ((0, 5), (5, 0), (16385, 5), (5, 16385), (-1, 5)):
        assert host_check(flow, h, w, 8, src, none, none) == (-53, None)
    for g in (1, 0, 8193):
        assert host_check(flow, 5, 5, 8, src, none, none, g=g) == (-53, None)
    for step in (0, -8, 16385):
        assert host_check(flow, 5, 5, step, src, none, none) == (-54, None)
    for lines, thickness in ((1, 1), (0, 1), (17, 0), (17, 4)):
        assert host_check(flow, 5, 5, 8, src, none, none, lines, thickness) == (-55, None)
    status, out = host_check(flow, 5, 5, 8, src, none, none)
    assert status == 0 and len(out) == 4 * 8 + 4 + 25 * 8 + 48 + 24 + 75


# ---- the library's own refusals: before any launch, so they run here -------------------------------------------------------------
def test_entry_points_refuse_before_any_launch():
    import ctypes as C
    from dvd_amd import lib
    raw, s = lib.raw(), C.c_float(SCALE)
    for h, w in ((0, 5), (5, 16385), (-1, 5)):
        assert raw.dvd_map_invert_workspace_bytes(h, w, 8) == -53
        assert raw.dvd_map_invert(None, 8, h, w, 8, s, None, None, None, None) == -53 and b"map_invert" in raw.dvd_last_error()
        assert raw.dvd_map_cycle_error(None, 8, None, h, w, s, None, None, None) == -53
        assert raw.dvd_mesh_overlay_rgb8(None, None, h, w, 17, 1, 0, 0, 0, None, None) == -53
        assert raw.dvd_transfer_points(None, h, w, None, 1, None, None) == -53
        assert raw.dvd_map_points(None, 8, h, w, s, None, 1, None, None) == -53
    for g in (1, 8193):
        assert raw.dvd_map_invert(None, g, 5, 5, 8, s, None, None, None, None) == -53
        assert raw.dvd_map_points(None, g, 5, 5, s, None, 1, None, None) == -53
    for step in (0, -1, 16385):
        assert raw.dvd_map_invert_workspace_bytes(5, 5, step) == -54
        assert raw.dvd_map_invert(None, 8, 5, 5, step, s, None, None, None, None) == -54 and b"step" in raw.dvd_last_error()
    for lines, thickness in ((1, 1), (17, 0), (17, 4)):
        assert raw.dvd_mesh_overlay_rgb8(None, None, 5, 5, lines, thickness, 0, 0, 0, None, None) == -55 and b"lines" in raw.dvd_last_error()
    assert raw.dvd_transfer_points(None, 5, 5, None, -1, None, None) == -56 and raw.dvd_map_points(None, 8, 5, 5, s, None, -1, None, None) == -56
    for call in (lambda: raw.dvd_map_invert(None, 8, 5, 5, 8, s, None, None, None, None),
                 lambda: raw.dvd_map_cycle_error(None, 8, None, 5, 5, s, None, None, None),
                 lambda: raw.dvd_mesh_overlay_rgb8(None, None, 5, 5, 17, 1, 0, 0, 0, None, None),
                 lambda: raw.dvd_transfer_points(None, 5, 5, None, 1, None, None),
                 lambda: raw.dvd_map_points(None, 8, 5, 5, s, None, 1, None, None)):
        assert call() == -1 and b"null" in raw.dvd_last_error()
    assert raw.dvd_transfer_points(None, 5, 5, None, 0, None, None) == 0                          # no point: nothing to do
    assert raw.dvd_map_invert_workspace_bytes(64, 48, 8) % 256 == 0 and raw.dvd_map_invert_workspace_bytes(64, 48, 1) > raw.dvd_map_invert_workspace_bytes(64, 48, 8)
    assert "dvd_map_invert_workspace_bytes" in lib.NON_STATUS and lib.RESTYPES["dvd_map_invert_workspace_bytes"] is C.c_long
    assert (lib.E_INV_SHAPE, lib.E_INV_STEP, lib.E_INV_LINES, lib.E_INV_POINTS) == (-53, -54, -55, -56)


def test_ops_refuse_bad_arguments_and_host_tensors(tmp_path):
    from dvd_amd import ops
    flow, fwd, pts, src = torch.zeros(2, 8, 8), torch.zeros(5, 7, 2), torch.zeros(3, 2), torch.zeros(5, 7, 3, dtype=torch.uint8)
    for call, name in ((lambda: ops.map_invert(flow, 5, 7), "map_invert"), (lambda: ops.map_cycle_error(flow, fwd), "map_cycle_error"),
                       (lambda: ops.mesh_overlay(src, fwd), "mesh_overlay"), (lambda: ops.transfer_points(fwd, pts), "transfer_points"),
                       (lambda: ops.map_points(flow, pts, 5, 7), "map_points"), (lambda: ops.coverage_mask(fwd), "coverage_mask"),
                       (lambda: ops.mesh_overlay_to_file(src, fwd, str(tmp_path / "never.png")), "mesh_overlay")):
        with pytest.raises(ValueError, match=f"{name}: .* on the device"):                       # host tensors: no CPU path
            call()
    with pytest.raises(ValueError, match="mesh_overlay_to_file: huffman"):
        ops.mesh_overlay_to_file(src, fwd, str(tmp_path / "never.png"), huffman="best")
    with pytest.raises(ValueError, match="inverse_displacement"):
        ops.inverse_write_flo(np.zeros((5, 7, 3), F), str(tmp_path / "never.flo"))
    assert list(tmp_path.iterdir()) == []
    assert ops.INV_STATS == ("covered", "fold_px", "flipped_tris", "degenerate_tris", "skipped_tris", "tris") and ops.MAP_INVALID == -1


# ---- .flo -----------------------------------------------------------------------------------------------------------------------
def test_inverse_flo_round_trips_with_unknown_at_uncovered_pixels(tmp_path):
    from dvd_amd import ops
    name = "smooth_37x29_g4_s3"
    _, h, w, _ = CASES[name]
    fwd = model(name)["fwd"]
    path = str(tmp_path / "inv.flo")
    assert ops.inverse_write_flo(torch.from_numpy(fwd.copy()), path) == 12 + 8 * h * w
    back = ops.flow_read_flo(path)
    cov = M.covered_of(fwd)
    assert np.array_equal(back.view(np.uint32), M.inverse_displacement(fwd).view(np.uint32))
    assert (back[~cov] == F(1e10)).all() and (~cov).any() and np.abs(back[cov]).max() < 8
    py, px = np.nonzero(cov)
    assert np.array_equal(back[py, px, 0], fwd[py, px, 0] - px.astype(F)) and np.array_equal(back[py, px, 1], fwd[py, px, 1] - py.astype(F))
    assert (np.abs(back[~cov]) > 1e9).all()                       # what map_errors treats as unknown ground truth


# ---- settings.inverse_outputs ---------------------------------------------------------------------------------------------------
def _settings(**attrs):
    import admin.settings as ws
    s = ws.Settings()
    s.name, s.seed = "pytest_mapinv", 5
    for k, v in attrs.items():
        setattr(s, k, v)
    return s


LOG = types.SimpleNamespace(info=lambda *a: None)


def _exploding_loader():
    raise AssertionError("the loader was read")
    yield                                                                          # pragma: no cover


def test_inverse_outputs_parsing():
    from dvd_amd import evaluation
    assert evaluation.INVERSE_OUTPUTS == ("mesh", "flo", "mask")
    def read(settings):
        return evaluation.RoundOptions.from_settings(settings).inverse_outputs
    assert read(_settings()) == () and read(_settings(inverse_outputs="")) == ()
    assert read(_settings(inverse_outputs="mask")) == ("mask",)
    assert read(_settings(inverse_outputs="mask, mesh")) == ("mesh", "mask")
    assert read(_settings(inverse_outputs="flo,mask,mesh")) == ("mesh", "flo", "mask")


def test_a_bad_inverse_outputs_is_refused_before_the_loader_is_read(tmp_path, monkeypatch):
    from dvd_amd import evaluation
    monkeypatch.chdir(tmp_path)
    for value in ("png", "mesh,mesh", "mesh,", ",", " ", "MESH", None, True, 3, ("mesh",), ["mesh"]):
        with pytest.raises(ValueError, match="settings.inverse_outputs"):
            evaluation.run_evaluation_docunet(_settings(inverse_outputs=value), LOG, _exploding_loader(), None, torch.nn.Linear(1, 1), None)
    assert list(tmp_path.iterdir()) == []


def test_no_new_env_switch():
    from dvd_amd import run_options
    assert not any("inverse" in str(row) for row in run_options.TABLE)


class _OpsSpy:
    """dvd_amd.ops with every entry of the map inverse recorded and answered on the host by the model."""

    def __init__(self, real):
        self._real, self.calls = real, []

    def map_invert(self, flow, h, w, step=8, scale=0.987):
        self.calls.append(("map_invert", h, w, step))
        fwd, stats = M.invert(flow.numpy(), h, w, step, scale)
        return torch.from_numpy(fwd), stats

    def map_cycle_error(self, flow, fwd, scale=0.987):
        self.calls.append(("map_cycle_error",))
        c = M.cycle_error(flow.numpy(), fwd.numpy(), scale)
        return {k: c[k] for k in ("cycle_mean", "cycle_max", "n")}

    def mesh_overlay_to_file(self, src, fwd, path, huffman="fixed", **kw):
        self.calls.append(("mesh_overlay_to_file", tuple(src.shape), src.dtype, os.path.basename(path), huffman))
        open(path, "wb").close()

    def coverage_mask(self, fwd):
        self.calls.append(("coverage_mask",))
        return "MASK"

    def png_encode_to_file(self, img, path, huffman="fixed"):
        self.calls.append(("png_encode_to_file", img, os.path.basename(path)))
        open(path, "wb").close()

    def inverse_write_flo(self, fwd, path):
        self.calls.append(("inverse_write_flo", os.path.basename(path)))
        return self._real.inverse_write_flo(fwd, path)

    def __getattr__(self, name):
        if name.startswith(("map_", "mesh_", "transfer_", "inverse_")):
            raise AssertionError(f"ops.{name} was called")
        return getattr(self._real, name)


H, W = 40, 30


def _loop(monkeypatch, tmp_path, **attrs):
    """run_evaluation_docunet on stand-ins for everything but the new code: one batch of two documents, maps of G = 9."""
    from dvd_amd import evaluation
    from mapinv_fixtures import smooth
    monkeypatch.chdir(tmp_path)
    spy = _OpsSpy(evaluation.ops)
    monkeypatch.setattr(evaluation, "ops", spy)
    batch = [{"path": "dir/a_1 copy.jpg", "src_u8": torch.zeros(H, W, 3, dtype=torch.uint8)},
             {"path": "synthetic_00001", "source_vis": torch.full((3, H, W), 300.0)}]
    flow = torch.from_numpy(np.stack([smooth(9, 0.03), smooth(9, 0.02)]))
    outs = [torch.zeros(H, W, 3, dtype=torch.uint8)] * 2
    monkeypatch.setattr(evaluation, "batches_of", lambda loader, n: iter([batch]))
    monkeypatch.setattr(evaluation, "adopt_reference_items", lambda *a, **k: None)
    monkeypatch.setattr(evaluation, "prepare_conditioning", lambda *a, **k: None)
    monkeypatch.setattr(evaluation, "sample_batch", lambda *a, **k: flow)
    monkeypatch.setattr(evaluation, "unwarp_tail", lambda *a, **k: outs)
    monkeypatch.setattr(evaluation.th.cuda, "synchronize", lambda: None)
    s = _settings(**attrs)
    s.env.visualize, s.env.eval_dataset_name = False, "synthetic"
    lines = []
    results = evaluation.run_evaluation_docunet(s, types.SimpleNamespace(info=lines.append), None, None, torch.nn.Linear(1, 1), None)
    assert [p for p, _ in results] == [d["path"] for d in batch]
    return s, spy, lines, flow.numpy()


def test_absent_attribute_calls_nothing_new(monkeypatch, tmp_path):
    for attrs in ({}, {"inverse_outputs": ""}):
        s, spy, lines, _ = _loop(monkeypatch, tmp_path, **attrs)
        assert spy.calls == [] and lines == [] and not hasattr(s, "map_inverse")
        run = tmp_path / "vis_hp" / "synthetic" / "pytest_mapinv"
        assert list(run.iterdir()) == []


def test_set_attribute_inverts_logs_and_writes_per_document(monkeypatch, tmp_path):
    from dvd_amd import evaluation
    s, spy, lines, flow = _loop(monkeypatch, tmp_path, inverse_outputs="mask,mesh,flo")
    per_doc = ["map_invert", "map_cycle_error", "mesh_overlay_to_file", "inverse_write_flo", "coverage_mask", "png_encode_to_file"]
    assert [c[0] for c in spy.calls] == per_doc * 2
    assert spy.calls[0] == ("map_invert", H, W, 8)
    assert spy.calls[2] == ("mesh_overlay_to_file", (H, W, 3), torch.uint8, "mesh_a_1 copy.png", "fixed")
    assert spy.calls[8][1:3] == ((H, W, 3), torch.uint8) and spy.calls[11][1:] == ("MASK", "mask_synthetic_00001.png")
    run = tmp_path / "vis_hp" / "synthetic" / "pytest_mapinv"
    assert sorted(f.name for f in (run / "pred_flow").iterdir()) == sorted(
        f"{kind}_{stem}.{ext}" for stem in ("a_1 copy", "synthetic_00001") for kind, ext in (("mesh", "png"), ("inv", "flo"), ("mask", "png")))
    assert [p for p, _ in s.map_inverse] == ["dir/a_1 copy.jpg", "synthetic_00001"]
    for j, (path, score) in enumerate(s.map_inverse):
        fwd, stats = M.invert(flow[j], H, W, 8)
        c = M.cycle_error(flow[j], fwd)
        assert score["covered"] == stats["covered"] > 0 and score["fold_px"] == 0 and score["fold"] == 0.0 and score["tris"] == stats["tris"]
        assert score["cycle_mean"] == c["cycle_mean"] == score["cycle"] and score["cycle_max"] == c["cycle_max"]
        assert lines[j] == (f"{path} map_inverse covered {stats['covered']} fold_px 0 flipped 0 skipped 0 "
                            f"cycle_mean {c['cycle_mean']:.6f} cycle_max {c['cycle_max']:.6f}")
        assert np.array_equal(evaluation.ops.flow_read_flo(str(run / "pred_flow" / f"inv_{('a_1 copy', 'synthetic_00001')[j]}.flo")),
                              M.inverse_displacement(fwd))
    text = (run / "map_inverse.txt").read_text().splitlines()
    assert text[0] == "path " + " ".join(evaluation.MAP_INVERSE_COLUMNS) and len(text) == 3
    assert text[1].startswith(f"dir/a_1 copy.jpg {s.map_inverse[0][1]['covered']} 0 0 0 0 ")
    assert [ln.split()[:3] for ln in lines[2:]] == [["mean", "map_inverse", k] for k in ("fold", "cycle_mean", "cycle_max")]
    assert lines[2] == "mean map_inverse fold 0.000000 over 2 of 2 documents"
    s2, spy2, lines2, _ = _loop(monkeypatch, tmp_path, inverse_outputs="mask")
    assert [c[0] for c in spy2.calls] == ["map_invert", "map_cycle_error", "coverage_mask", "png_encode_to_file"] * 2 and len(lines2) == 5


# ---- the launcher -----------------------------------------------------------------------------------------------------------------
def _fake_launch(monkeypatch, R, seen):
    def run(settings):
        seen.append((settings.name, getattr(settings, "inverse_outputs", None), hasattr(settings, "map_inverse")))
        settings.ms_ssim = [("a", 0.5 + settings.corruption_number / 100), ("b", 0.7)]
        if getattr(settings, "inverse_outputs", None) and settings.corruption_number != 1:
            settings.map_inverse = [("a", {"fold": 0.0, "cycle": 0.25, "covered": 10}), ("b", {"fold": 0.5, "cycle": float("nan"), "covered": 0})]
    monkeypatch.setattr(R, "importlib", types.SimpleNamespace(import_module=lambda name: types.SimpleNamespace(run=run)))
    monkeypatch.setattr(R, "shutil", types.SimpleNamespace(copyfile=lambda *a: None))


def test_table_gains_the_columns_only_under_the_flag(tmp_path, monkeypatch):
    import run_sampling as R
    monkeypatch.chdir(tmp_path)
    seen = []
    _fake_launch(monkeypatch, R, seen)
    table = tmp_path / "vis_hp" / "synthetic" / "exp" / "corruption_table.txt"
    R.run_sampling("dvd", "val_TDiff", 3, "exp", corruption=True)
    plain = table.read_text()
    assert plain.splitlines()[0] == "no kind severity ms_ssim" and all(v is None for _, v, _ in seen)      # the attribute stays absent
    R.run_sampling("dvd", "val_TDiff", 3, "exp", corruption=True, inverse_outputs="")
    assert table.read_text() == plain
    seen.clear()
    R.run_sampling("dvd", "val_TDiff", 3, "exp", corruption=True, inverse_outputs="mesh")
    scored = table.read_text().splitlines()
    assert all(v == "mesh" and not had for _, v, had in seen)                     # a round never sees the scores of the one before
    assert scored[0] == "no kind severity ms_ssim fold cycle"
    assert scored[1] == "0 gaussian_noise 5 0.600000 0.250000 0.250000" and scored[2] == "1 shot_noise 5 0.605000 - -"
    assert [r.rsplit(" ", 2)[0] for r in scored] == plain.splitlines()            # the rest is the old table
    R.run_sampling("dvd", "val_TDiff", 3, "exp", severity=3, corruption_number=10, keyed_noise=True, gt_map_dir=str(tmp_path),
                   inverse_outputs="mesh,flo")
    assert table.read_text().splitlines()[0] == "no kind severity ms_ssim map_dev epe pck5 ause_epe fold cycle"
    monkeypatch.setattr(sys, "argv", ["run_sampling.py", "--train_module", "dvd", "--train_name", "val_TDiff", "--name", "cli",
                                      "--inverse_outputs", "mask,flo"])
    seen.clear()
    R.main()
    assert seen == [("cli", "mask,flo", False)]


# ---- apply_map --points ---------------------------------------------------------------------------------------------------------
def test_apply_map_carries_points(tmp_path, monkeypatch):
    from PIL import Image
    from dvd_amd import apply_map as A
    name = "smooth_37x29_g4_s3"
    flow, h, w, step = CASES[name]
    np.save(tmp_path / "m.npy", flow)
    Image.fromarray(photograph(h, w)).save(tmp_path / "in.png")
    pts = points(h, w)[4:]
    np.savetxt(tmp_path / "pts.txt", pts, fmt="%.6f")
    seen = []

    def carry(flow_, pts_, h_, w_, to, step_):
        seen.append((flow_.shape, pts_.dtype, h_, w_, to, step_))
        got = M.transfer_points(M.invert(flow_[0], h_, w_, step_)[0], pts_) if to == "page" else M.map_points(flow_[0], pts_, h_, w_)
        got = got.copy()
        got[got.view(np.uint32) == M.INVALID] = np.nan
        return got
    monkeypatch.setattr(A, "carry_points", carry)
    args = [str(tmp_path / "m.npy"), str(tmp_path / "in.png"), str(tmp_path / "out.txt"), "--points", str(tmp_path / "pts.txt")]
    A.main(args + ["--step", str(step)])
    A.main(args[:2] + [str(tmp_path / "photo.txt")] + args[3:] + ["--to", "photo"])
    assert seen == [((1, 2, 4, 4), np.float32, h, w, "page", step), ((1, 2, 4, 4), np.float32, h, w, "photo", 8)]
    read = np.loadtxt(tmp_path / "pts.txt", dtype=np.float64, ndmin=2).astype(F)
    page = np.loadtxt(tmp_path / "out.txt", ndmin=2)
    want = M.transfer_points(model(name)["fwd"], read)
    ok = want.view(np.uint32)[:, 0] != M.INVALID
    assert page.shape == (len(pts), 2) and ok.any() and (~ok).any()
    assert np.isnan(page[~ok]).all() and np.abs(page[ok] - want[ok]).max() <= 5.1e-5          # four decimals
    photo = np.loadtxt(tmp_path / "photo.txt", ndmin=2)
    assert np.abs(photo - M.map_points(flow, read, h, w)).max() <= 5.1e-5
    for bad in ("1 2 3\n4 5 6\n", "1 x\n"):
        (tmp_path / "bad.txt").write_text(bad)
        with pytest.raises(ValueError, match="bad.txt"):
            A.load_points(str(tmp_path / "bad.txt"))
    with pytest.raises(ValueError, match="--to"):
        A.apply_points(str(tmp_path / "m.npy"), "none.png", "never.txt", str(tmp_path / "pts.txt"), to="scan")
    with pytest.raises(ValueError, match="--step"):
        A.apply_points(str(tmp_path / "m.npy"), "none.png", "never.txt", str(tmp_path / "pts.txt"), step=0)
    with pytest.raises(SystemExit):
        A.main(args + ["--to", "scan"])
    assert not os.path.exists("never.txt")
