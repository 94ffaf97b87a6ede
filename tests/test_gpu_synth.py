"""Synthetic documents on the device: the kernels of synth.hip against tests/synth_model.py - whole buffers,
byte for byte, between guard rows, inputs untouched - and the dataset writer end to end: the maps it writes score exactly 0
against themselves, its photographs unwarp back to the scan, and the document loop scores every document against its map."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import synth_model as Y  # noqa: E402
import synth_fixtures as X  # noqa: E402
from mapinv_fixtures import CASES, F, SCALE, model as inv_model  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 3                      # rows on either side of an output, pre-filled


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()                  # a copy: the fixtures are read-only


def _guarded(shape):
    """(the whole buffer, its middle as the output tensor): GUARD rows of 0x5a before and after."""
    whole = torch.full((shape[0] + 2 * GUARD, *shape[1:]), 0x5a, dtype=torch.uint8, device="cuda")
    return whole, whole[GUARD:GUARD + shape[0]]


def _guards_untouched(whole, rows):
    raw = whole.cpu().numpy().reshape(whole.shape[0], -1)
    return (raw[:GUARD] == 0x5a).all() and (raw[GUARD + rows:] == 0x5a).all()


@pytest.mark.parametrize("name", list(X.RENDER_CASES))
def test_kernels_equal_the_model(name):
    from dvd_amd import ops
    c = X.render_case(name)
    h, w = c["fwd"].shape[:2]
    scan, fwd = _dev(c["scan"]), _dev(c["fwd"])
    bg = c["background"] if isinstance(c["background"], tuple) else _dev(c["background"])
    whole, out = _guarded((h, w, 3))
    photo = ops.synth_render(scan, fwd, background=bg, shading=c["shading"], out=out)
    assert photo is out and _guards_untouched(whole, h)
    assert np.array_equal(photo.cpu().numpy(), c["photo"])                                       # byte for byte
    whole, out = _guarded((h, w, 2))
    radii = ops.synth_footprint(c["scan"].shape[:2], fwd, out=out)
    assert radii is out and _guards_untouched(whole, h) and np.array_equal(radii.cpu().numpy(), c["radii"])
    assert np.array_equal(scan.cpu().numpy(), c["scan"]) and np.array_equal(fwd.cpu().numpy().view(np.uint32), c["fwd"].view(np.uint32))
    if torch.is_tensor(bg):
        assert np.array_equal(bg.cpu().numpy(), c["background"])
    assert torch.equal(ops.synth_render(scan, fwd, background=bg, shading=c["shading"]), photo)   # twice: the same bytes


def test_footprint_reports_the_cap():
    from dvd_amd import ops
    fwd = _dev(X.fwd_of("small_40x32"))
    covered = ops.coverage_mask(fwd)[..., 0] != 0
    assert (ops.synth_footprint((40, 32), fwd)[covered] == 1).all()                              # a scan of the photograph's size
    mixed = ops.synth_footprint((120, 96), fwd)[covered]
    assert int(mixed.max()) < ops.SYNTH_MAX_RADIUS and len(torch.unique(mixed[mixed > 1])) >= 2
    assert (ops.synth_footprint((400, 320), _dev(X.fwd_of("calm_40x32")))[ops.coverage_mask(_dev(X.fwd_of("calm_40x32")))[..., 0] != 0]
            == ops.SYNTH_MAX_RADIUS).all()


def test_shading_off_is_skipped_and_a_ref_defaults_to_the_covered_share():
    from dvd_amd import ops
    c = X.render_case("smooth_96x80_shaded")
    scan, fwd, bg = _dev(c["scan"]), _dev(c["fwd"]), _dev(c["background"])
    plain = ops.synth_render(scan, fwd, background=bg)
    assert np.array_equal(plain.cpu().numpy(), Y.render(c["scan"], c["fwd"], c["background"]))
    assert torch.equal(ops.synth_render(scan, fwd, background=bg, shading=dict(l0=0, lgx=0, lgy=0, k=0, a_ref=7.0)), plain)
    assert torch.equal(ops.synth_render(scan, fwd, background=bg, shading=dict(l0=1.0)), plain)   # L = 1: Lq = 65536, the identity
    assert np.array_equal(ops.synth_render(scan, fwd, background=bg, shading=X.SHADE).cpu().numpy(), c["photo"])     # a_ref counted from fwd


def test_refused_calls_answer_their_status_and_write_nothing():
    import ctypes as C
    from dvd_amd import lib, ops
    raw = lib.raw()
    scan, fwd = torch.zeros(6, 5, 3, dtype=torch.uint8, device="cuda"), torch.zeros(5, 8, 2, device="cuda")
    whole, out = _guarded((5, 8, 3))
    prm, p = lib.SynthParams(0, 0, 0, 0, 1), lib.ptr
    assert raw.dvd_synth_render_rgb8(p(scan), 0, 5, p(fwd), 5, 8, None, 0, C.byref(prm), p(out), None) == lib.E_SYNTH_SHAPE
    assert raw.dvd_synth_render_rgb8(p(scan), 6, 5, p(fwd), 5, 16385, None, 0, C.byref(prm), p(out), None) == lib.E_SYNTH_SHAPE
    bad = lib.SynthParams(1, float("nan"), 0, 0, 1)
    assert raw.dvd_synth_render_rgb8(p(scan), 6, 5, p(fwd), 5, 8, None, 0, C.byref(bad), p(out), None) == lib.E_SYNTH_PARAM
    assert raw.dvd_synth_render_rgb8(p(scan), 6, 5, None, 5, 8, None, 0, C.byref(prm), p(out), None) == -1
    assert raw.dvd_synth_render_rgb8(p(scan), 6, 5, p(fwd), 5, 8, None, 0, C.byref(prm), C.c_void_p(out.data_ptr() + 1), None) == -1
    assert raw.dvd_synth_footprint(p(fwd), 5, 8, 6, 0, p(out), None) == lib.E_SYNTH_SHAPE
    torch.cuda.synchronize()
    assert (whole == 0x5a).all()
    for call in (lambda: ops.synth_render(scan, fwd, background=(0, 0)), lambda: ops.synth_render(scan, fwd, background=(0, 0, 256)),
                 lambda: ops.synth_render(scan, fwd, background=torch.zeros(5, 7, 3, dtype=torch.uint8, device="cuda")),
                 lambda: ops.synth_render(scan, fwd, background=torch.zeros(5, 8, 3, device="cuda")),
                 lambda: ops.synth_render(scan, fwd, shading=dict(k=float("inf"))), lambda: ops.synth_render(scan, fwd, shading=dict(a_ref=-1.0)),
                 lambda: ops.synth_render(scan.float(), fwd), lambda: ops.synth_render(scan[:, :, :2], fwd),
                 lambda: ops.synth_render(scan, fwd[..., :1]), lambda: ops.synth_render(scan, fwd.double()),
                 lambda: ops.synth_render(scan, fwd, out=torch.zeros(5, 8, 3, dtype=torch.uint8)),
                 lambda: ops.synth_render(scan, fwd, out=torch.zeros(5, 9, 3, dtype=torch.uint8, device="cuda")),
                 lambda: ops.synth_render(scan, fwd, out=whole.view(-1)[1:121].view(5, 8, 3))):
        with pytest.raises(ValueError, match="synth_render"):
            call()
    for call in (lambda: ops.synth_render(scan.cpu(), fwd), lambda: ops.synth_render(scan, fwd.cpu()),
                 lambda: ops.synth_render(scan, fwd, background=torch.zeros(5, 8, 3, dtype=torch.uint8)),
                 lambda: ops.synth_footprint((6, 5), fwd.cpu()), lambda: ops.synth_document(scan, torch.zeros(2, 8, 8), 5, 8)):
        with pytest.raises(lib.DvdError, match="on the device"):
            call()
    for bad in (dict(step=0), dict(scale=float("nan")), dict(shading=dict(l0="1")), dict(background="white")):
        with pytest.raises(ValueError):
            ops.synth_document(scan, torch.zeros(2, 8, 8, device="cuda"), 5, 8, **bad)
    assert (whole == 0x5a).all()


@pytest.mark.parametrize("case", ["smooth_64x48_g9_s8", "smooth_96x80_g16_s1"])
def test_document_is_invert_then_render(case):
    from dvd_amd import ops
    flow, h, w, step = CASES[case]
    scan, dflow, bg = _dev(X.page_scan(h, w)), _dev(flow), _dev(X.background_plane(h, w))
    photo, fwd, stats = ops.synth_document(scan, dflow, h, w, step=step, background=bg, shading=X.SHADE)
    fwd2, stats2 = ops.map_invert(dflow, h, w, step=step)
    assert stats == stats2 == inv_model(case)["stats"] and torch.equal(fwd.view(torch.int32), fwd2.view(torch.int32))
    prm = dict(X.SHADE, a_ref=h * w / stats["covered"])
    assert torch.equal(photo, ops.synth_render(scan, fwd2, background=bg, shading=prm))
    assert np.array_equal(photo.cpu().numpy(), Y.render(X.page_scan(h, w), inv_model(case)["fwd"], X.background_plane(h, w),
                                                        dict(prm, a_ref=float(F(prm["a_ref"])))))
    plain, _, _ = ops.synth_document(scan, dflow, h, w, step=step)
    assert torch.equal(plain, ops.synth_render(scan, fwd2))
    # the round trip on the device: the photograph unwarped by its own map is the scan again, within the bar of the model
    page = ops.unwarp_u8(dflow, plain)
    diff = X.cycle_difference(X.page_scan(h, w), page.cpu().numpy())
    print(case, "cycle on the device", diff, "recorded on the model", X.CYCLE_MEASURED[case])
    assert diff <= X.CYCLE_BAR * X.CYCLE_MEASURED[case]


def test_many_workgroups_and_the_general_loop():
    """301 x 260 from a scan of 700 x 600: a hundred workgroups, dword stores, radii 2 and 3 beside each other."""
    from dvd_amd import ops
    import mapinv_model as M
    from mapinv_fixtures import smooth
    h, w, flow = 301, 260, smooth(64, 0.03)
    fwd = M.invert(flow, h, w, 8, SCALE)[0]
    scan = X.page_scan(700, 600)
    want = Y.render(scan, fwd, X.TRIPLE, dict(X.SHADE, a_ref=5.0))
    got = ops.synth_render(_dev(scan), _dev(fwd), background=X.TRIPLE, shading=dict(X.SHADE, a_ref=5.0))
    assert np.array_equal(got.cpu().numpy(), want)
    radii = ops.synth_footprint((700, 600), _dev(fwd)).cpu().numpy()
    assert np.array_equal(radii, Y.footprint(fwd, 700, 600)) and {2, 3} <= set(np.unique(radii))


# ---- end to end ---------------------------------------------------------------------------------------------------------------
def test_dataset_writer_end_to_end(tmp_path, monkeypatch, capsys):
    """Two procedural documents of 64 x 48 from G = 9 maps.  Each written .flo scored against its own .npy gives EPE exactly 0;
    each photograph, decoded and unwarped with its .npy, is the scan again within the cycle bar; and one run of the document
    loop over OUT/img with gt_map_dir = OUT/map (G = 16, 2 steps, synthetic weights) logs a finite map_score line per document
    and skips none."""
    import admin.settings as ws
    from dvd_amd import ops, synth_docs, val_TDiff
    monkeypatch.chdir(tmp_path)
    man = synth_docs.main(["-", "out", "--procedural", "2", "--size", "64x48", "--g", "9", "--format", "png", "--seed", "4",
                           "--kinds", "curl,mixed", "--background", "noise", "--shading", ""])
    assert json.loads((tmp_path / "out" / "manifest.json").read_text()) == man
    docs = man["documents"]
    assert [d["stem"] for d in docs] == ["page_00000", "page_00001"] and all(tuple(d) == synth_docs.MANIFEST_KEYS for d in docs)
    for d in docs:
        assert all(d["stats"][k] == 0 for k in synth_docs.ACCEPT_ZERO) and d["cap_share"] == 0.0
        flow = np.load(tmp_path / "out" / d["map"])
        assert flow.tobytes() == synth_docs.make_map(tuple(d["key"]), 9, d["kind"], d["strength"], attempt=d["attempts"] - 1).tobytes()
        field = _dev(ops.flow_read_flo(str(tmp_path / "out" / d["flo"])))
        score = ops.map_score(_dev(flow), field)
        assert score["epe"] == 0.0 and score["pck1"] == 1.0 and score["n_valid"] == 64 * 48
        scan = ops.pil_decode_rgb8(str(tmp_path / "out" / d["scan"]))
        assert np.array_equal(scan, synth_docs.procedural_page(tuple(d["key"]), 64, 48))
        photo = _dev(ops.pil_decode_rgb8(str(tmp_path / "out" / d["image"])))
        fwd, stats = ops.map_invert(_dev(flow), 64, 48)
        assert stats == d["stats"]
        bg = _dev(synth_docs.noise_background(tuple(d["key"]), 64, 48))
        assert torch.equal(photo, ops.synth_render(_dev(scan), fwd, background=bg))            # the file holds the render
        diff = X.cycle_difference(scan, ops.unwarp_u8(_dev(flow), photo).cpu().numpy())
        print(d["stem"], d["kind"], "cycle", diff, "bar", X.CYCLE_BAR * X.CYCLE_MEASURED["smooth_64x48_g9_s8"])
        assert diff <= X.CYCLE_BAR * X.CYCLE_MEASURED["smooth_64x48_g9_s8"]
    s = ws.Settings()
    s.env.grid_size, s.env.diffusion_steps, s.env.batch_docs = 16, 2, 2
    s.name, s.seed, s.severity, s.corruption_number = "pytest_synth_docs", 0, 0, 0
    s.env.eval_dataset_name, s.env.eval_dataset = "synthdocs", os.path.join("out", "img")
    s.env.use_prestage_nets, s.env.synthetic_weights_if_missing, s.env.visualize = True, True, True
    s.gt_map_dir = os.path.join("out", "map")
    torch.manual_seed(0)
    capsys.readouterr()
    got = val_TDiff.run(s)
    log = capsys.readouterr().out
    assert [os.path.basename(p) for p, _ in got] == ["page_00000.png", "page_00001.png"]
    assert "skipped: no ground-truth map" not in log
    assert [os.path.basename(p) for p, _ in s.map_score] == ["page_00000.png", "page_00001.png"]
    for (p, score), d in zip(s.map_score, docs):
        line = next(ln for ln in log.splitlines() if ln.startswith(f"{p} map_score epe "))
        assert np.isfinite(float(line.split()[3])) and np.isfinite(score["epe"]) and score["n_valid"] == 64 * 48
