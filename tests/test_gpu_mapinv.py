"""The map inverse on the device: the kernels of mapinv.hip against tests/mapinv_model.py - the forward map, the
counts, the cycle numbers, the mesh picture and the points bit for bit, in buffers with guard rows - and one run of the document
loop with settings.inverse_outputs."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mapinv_model as M  # noqa: E402

from mapinv_fixtures import (CASES, F, OVERLAYS, SCALE, SMOOTH, interior_points, model, photograph, points,  # noqa: E402
                             round_trip_bound, smooth)

pytestmark = pytest.mark.gpu
GUARD = 3                      # rows on either side of an output, pre-filled


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t):
    return t.contiguous().view(torch.int32).cpu().numpy().view(np.uint32)


def _guarded(shape, dtype):
    """(the whole buffer, its middle as the output tensor): GUARD rows of the pattern before and after."""
    fill = 0x5a if dtype == torch.uint8 else float(np.frombuffer(b"\x5a\x5a\x5a\x5a", F)[0])
    whole = torch.full((shape[0] + 2 * GUARD, *shape[1:]), fill, dtype=dtype, device="cuda")
    return whole, whole[GUARD:GUARD + shape[0]]


def _guards_untouched(whole, rows):
    raw = whole.contiguous().view(torch.uint8).cpu().numpy().reshape(whole.shape[0], -1)
    return (raw[:GUARD] == 0x5a).all() and (raw[GUARD + rows:] == 0x5a).all()


def _check_case(flow, h, w, step, m, overlays):
    from dvd_amd import ops
    dflow = _dev(flow)
    whole, out = _guarded((h, w, 2), torch.float32)
    fwd, stats = ops.map_invert(dflow, h, w, step=step, out=out)
    assert fwd is out and _guards_untouched(whole, h)
    assert np.array_equal(_bits(fwd), m["fwd"].view(np.uint32))                                     # bit for bit
    assert stats == m["stats"]
    c, want = ops.map_cycle_error(dflow, fwd), m["cycle"]
    assert c["n"] == want["n"]
    if want["n"]:
        assert c["cycle_mean"] == want["cycle_mean"] and c["cycle_max"] == want["cycle_max"]       # the same order: the same bits
    else:
        assert np.isnan(c["cycle_mean"]) and np.isnan(c["cycle_max"])
    src = photograph(h, w)
    dsrc = _dev(src)
    for ov in overlays:
        whole, out = _guarded((h, w, 3), torch.uint8)
        pic = ops.mesh_overlay(dsrc, fwd, out=out, **ov)
        assert _guards_untouched(whole, h) and np.array_equal(pic.cpu().numpy(), M.mesh_overlay(src, m["fwd"], **ov)), ov
    assert np.array_equal(dsrc.cpu().numpy(), src)
    pts = points(h, w)
    dpts = _dev(pts)
    whole, out = _guarded((len(pts), 2), torch.float32)
    assert np.array_equal(_bits(ops.transfer_points(fwd, dpts, out=out)), M.transfer_points(m["fwd"], pts).view(np.uint32))
    assert _guards_untouched(whole, len(pts))
    whole, out = _guarded((len(pts), 2), torch.float32)
    assert np.array_equal(_bits(ops.map_points(dflow, dpts, h, w, out=out)), M.map_points(flow, pts, h, w, SCALE, pos=m["pos"]).view(np.uint32))
    assert _guards_untouched(whole, len(pts))
    return fwd


@pytest.mark.parametrize("name", list(CASES))
def test_kernels_equal_the_model(name):
    flow, h, w, step = CASES[name]
    _check_case(flow, h, w, step, model(name), OVERLAYS if name in ("smooth_37x29_g4_s3", "folded", "nan") else OVERLAYS[:1])


@pytest.mark.parametrize("name", ["smooth_37x29_g4_s3", "smooth_96x80_g16_s8", "inf", "huge"])
def test_lattice_is_the_unwarp_grid(name):
    """The mesh's vertices are the positions the unwarp tail samples: dvd_unwarp_grid at the lattice pixels, un-normalised and
    quantised as stated."""
    from dvd_amd import ops
    flow, h, w, step = CASES[name]
    _, _, verts, valid = ops.map_invert(_dev(flow), h, w, step=step, lattice=True)
    grid = ops.unwarp_grid(_dev(flow), h, w, SCALE).cpu().numpy()[0]
    rows, cols = M.lattice_axis(h, step), M.lattice_axis(w, step)
    with np.errstate(all="ignore"):
        x = (((grid[0] + F(1)) * F(0.5)) * F(w - 1)).astype(F)[rows][:, cols]
        y = (((grid[1] + F(1)) * F(0.5)) * F(h - 1)).astype(F)[rows][:, cols]
    qx, qy, ok = M.quantise(x, y)
    verts = verts.cpu().numpy()
    assert np.array_equal(valid.cpu().numpy() != 0, ok) and np.array_equal(verts[..., 0], qx) and np.array_equal(verts[..., 1], qy)
    lat = model(name)["detail"][0]
    assert np.array_equal(lat["qx"], qx) and np.array_equal(lat["valid"], ok)                  # and the model's grid is the kernel's
    assert ok.all() == (name.startswith("smooth"))


@pytest.mark.parametrize("step", [8, 1])
def test_many_workgroups(step):
    """701 x 500 from G = 64: hundreds of workgroups in every pass, more block partials than one finalize round; twice."""
    from dvd_amd import ops
    h, w = 701, 500
    flow = smooth(64, 0.03)
    fwd_m, stats_m, _ = M.invert(flow, h, w, step, SCALE, detail=True)
    pos = M.positions(flow, h, w, SCALE)
    m = {"fwd": fwd_m, "stats": stats_m, "pos": pos, "cycle": M.cycle_error(flow, fwd_m, SCALE, pos=pos)}
    assert stats_m["fold_px"] == 0 and stats_m["covered"] > 0.9 * h * w
    fwd = _check_case(flow, h, w, step, m, OVERLAYS[:1])
    again, stats = ops.map_invert(_dev(flow), h, w, step=step)
    assert np.array_equal(_bits(again), _bits(fwd)) and stats == stats_m                      # two runs: identical bytes
    assert ops.map_cycle_error(_dev(flow), again) == ops.map_cycle_error(_dev(flow), fwd)


def test_two_runs_of_a_folded_map_are_identical():
    """Where triangles overlap the atomics arrive in any order; the minimum does not care."""
    from dvd_amd import ops
    flow, h, w, step = CASES["folded"]
    runs = [ops.map_invert(_dev(flow), h, w, step=step) for _ in range(3)]
    for fwd, stats in runs[1:]:
        assert np.array_equal(_bits(fwd), _bits(runs[0][0])) and stats == runs[0][1]
    src = _dev(photograph(h, w))
    assert torch.equal(ops.mesh_overlay(src, runs[0][0]), ops.mesh_overlay(src, runs[1][0]))


@pytest.mark.parametrize("name", [f"smooth_{h}x{w}_g{g}_s{step}" for h, w, g, step, _ in SMOOTH])
def test_points_come_back(name):
    """Page -> photograph -> page returns an interior point within the bound that follows from the case's cycle error."""
    from dvd_amd import ops
    flow, h, w, step = CASES[name]
    m = model(name)
    pts = interior_points(h, w)
    fwd, _ = ops.map_invert(_dev(flow), h, w, step=step)
    back = ops.transfer_points(fwd, ops.map_points(_dev(flow), _dev(pts), h, w)).cpu().numpy()
    assert (back.view(np.uint32) != M.INVALID).all()
    bound = round_trip_bound(m["pos"], m["cycle"]["cycle_max"])
    worst = float(np.abs(back - pts).max())
    print(name, "worst", worst, "bound", bound, "cycle_max", m["cycle"]["cycle_max"])
    assert worst <= bound
    want = M.transfer_points(m["fwd"], M.map_points(flow, pts, h, w, SCALE, pos=m["pos"]))
    assert np.array_equal(back.view(np.uint32), want.view(np.uint32))


def test_ops_refuse_what_the_kernels_cannot_take():
    from dvd_amd import ops
    flow, fwd = torch.zeros(2, 8, 8, device="cuda"), torch.zeros(5, 7, 2, device="cuda")
    src, pts = torch.zeros(5, 7, 3, dtype=torch.uint8, device="cuda"), torch.zeros(3, 2, device="cuda")
    for bad in (dict(step=0), dict(step=2.0), dict(step=True), dict(scale=float("nan")), dict(scale="1"), dict(out=torch.zeros(5, 7, 2)),
                dict(out=torch.zeros(5, 8, 2, device="cuda"))):
        with pytest.raises(ValueError, match="map_invert"):
            ops.map_invert(flow, 5, 7, **bad)
    for h, w in ((0, 7), (5, 16385), (5.0, 7)):
        with pytest.raises(ValueError, match="map_invert"):
            ops.map_invert(flow, h, w)
        with pytest.raises(ValueError, match="map_points"):
            ops.map_points(flow, pts, h, w)
    for bad in (torch.zeros(3, 8, 8, device="cuda"), torch.zeros(2, 8, 9, device="cuda"), torch.zeros(2, 1, 1, device="cuda"),
                torch.zeros(2, 8, 8, dtype=torch.float16, device="cuda")):
        with pytest.raises(ValueError, match="map_invert"):
            ops.map_invert(bad, 5, 7)
        with pytest.raises(ValueError, match="map_cycle_error"):
            ops.map_cycle_error(bad, fwd)
    for bad in (dict(lines=1), dict(lines=2.5), dict(thickness=0), dict(thickness=4), dict(color=(256, 0, 0)), dict(outline_color=(0, 0)),
                dict(color="red"), dict(out=src)):
        with pytest.raises(ValueError, match="mesh_overlay"):
            ops.mesh_overlay(src, fwd, **bad)
    with pytest.raises(ValueError, match="mesh_overlay"):
        ops.mesh_overlay(src[:4], fwd)
    for bad in (torch.zeros(3, 3, device="cuda"), torch.zeros(6, device="cuda"), torch.zeros(3, 2, dtype=torch.float64, device="cuda"), pts.cpu()):
        with pytest.raises(ValueError, match="transfer_points"):
            ops.transfer_points(fwd, bad)
        with pytest.raises(ValueError, match="map_points"):
            ops.map_points(flow, bad, 5, 7)
    assert tuple(ops.transfer_points(fwd, torch.zeros(0, 2, device="cuda")).shape) == (0, 2)


# ---- end to end ---------------------------------------------------------------------------------------------------------------
PATHS = ["synthetic_00000", "synthetic_00001"]
SIZE = (96, 80)


def _launcher(monkeypatch, tmp_path):
    import types
    import admin.settings as ws
    import run_sampling as R
    monkeypatch.chdir(tmp_path)
    made = []

    class Small(ws.Settings):
        def __init__(self):
            super().__init__()
            self.env.grid_size, self.env.diffusion_steps = 16, 2
            self.env.num_synthetic_docs, self.env.batch_docs, self.env.full_res = 2, 2, SIZE
            self.env.visualize, self.env.use_prestage_nets = True, True
            self.env.eval_dataset_name = "synthetic"
            made.append(self)
    monkeypatch.setattr(R, "ws_settings", types.SimpleNamespace(Settings=Small))
    monkeypatch.setattr(R, "shutil", types.SimpleNamespace(copyfile=lambda *a: None))
    return R, made


def test_run_writes_the_inverse_and_a_run_without_the_attribute_does_not(tmp_path, monkeypatch):
    """G = 16, 2 steps, synthetic weights, two synthetic image documents, keyed noise (so that two runs sample the same maps)."""
    from PIL import Image
    from dvd_amd import evaluation, ops
    R, made = _launcher(monkeypatch, tmp_path)
    R.run_sampling("dvd", "val_TDiff", 77, "with", keyed_noise=True, inverse_outputs="mesh,flo,mask")
    R.run_sampling("dvd", "val_TDiff", 77, "without", keyed_noise=True)
    with_, without = made
    assert with_.inverse_outputs == "mesh,flo,mask" and not hasattr(without, "inverse_outputs") and not hasattr(without, "map_inverse")
    root = tmp_path / "vis_hp" / "synthetic"
    assert sorted(f.name for f in (root / "with" / "pred_flow").iterdir()) == sorted(
        f"{kind}_{p}.{ext}" for p in PATHS for kind, ext in (("mesh", "png"), ("inv", "flo"), ("mask", "png")))
    assert [f.name for f in root.glob("without/**/*") if f.name.startswith(("mesh_", "inv_", "mask_", "map_inverse"))] == []
    text = (root / "with" / "map_inverse.txt").read_text().splitlines()
    assert text[0] == "path " + " ".join(evaluation.MAP_INVERSE_COLUMNS) and [ln.split()[0] for ln in text[1:]] == PATHS
    assert [p for p, _ in with_.map_inverse] == PATHS
    h, w = SIZE
    for i, p in enumerate(PATHS):
        flow = with_.map_ref[p].cuda()                                                           # the map the sampler returned
        fwd, stats = ops.map_invert(flow, h, w)
        score = with_.map_inverse[i][1]
        assert score["covered"] == stats["covered"] > 0 and score["fold_px"] == stats["fold_px"] and score["tris"] == stats["tris"] == 2 * 12 * 10
        assert score["cycle_mean"] == ops.map_cycle_error(flow, fwd)["cycle_mean"]
        src = _dev(next(evaluation.synthetic_documents(with_, [i]))["image_u8"])
        mesh = np.asarray(Image.open(root / "with" / "pred_flow" / f"mesh_{p}.png"))
        assert mesh.shape == (h, w, 3) and np.array_equal(mesh, ops.mesh_overlay(src, fwd).cpu().numpy())
        covered = M.covered_of(fwd.cpu().numpy())
        mask = np.asarray(Image.open(root / "with" / "pred_flow" / f"mask_{p}.png"))
        assert mask.shape == (h, w, 3) and np.array_equal(mask, np.repeat((covered * 255).astype(np.uint8)[..., None], 3, axis=2))
        assert np.array_equal(ops.flow_read_flo(str(root / "with" / "pred_flow" / f"inv_{p}.flo")), M.inverse_displacement(fwd.cpu().numpy()))
        assert (root / "without" / "dewarped_pred" / f"warped_{p}.png").read_bytes() == \
            (root / "with" / "dewarped_pred" / f"warped_{p}.png").read_bytes()


def test_apply_map_carries_points_on_the_device(tmp_path):
    from PIL import Image
    from dvd_amd import apply_map
    flow, h, w, step = CASES["smooth_64x48_g9_s8"]
    np.save(tmp_path / "m.npy", flow)
    Image.fromarray(photograph(h, w)).save(tmp_path / "in.png")
    pts = interior_points(h, w, n=20)
    np.savetxt(tmp_path / "page.txt", pts, fmt="%.6f")
    apply_map.main([str(tmp_path / "m.npy"), str(tmp_path / "in.png"), str(tmp_path / "photo.txt"), "--points", str(tmp_path / "page.txt"),
                    "--to", "photo"])
    apply_map.main([str(tmp_path / "m.npy"), str(tmp_path / "in.png"), str(tmp_path / "back.txt"), "--points", str(tmp_path / "photo.txt")])
    back = np.loadtxt(tmp_path / "back.txt", ndmin=2)
    m = model("smooth_64x48_g9_s8")
    assert np.isfinite(back).all() and np.abs(back - pts).max() <= round_trip_bound(m["pos"], m["cycle"]["cycle_max"]) + 2e-4
