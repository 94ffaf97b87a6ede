"""Flow pictures and .flo files without a GPU: the NumPy model against goldens of the real reference, the
sanitised CPU restatement against the model byte for byte, the .flo layout, the up-sampled field against torch and float64,
settings.flow_outputs from the launcher to the document loop, and apply_map's argument check."""
import os
import struct
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flowviz_model as M  # noqa: E402
from host_check import build_host_check  # noqa: E402

from flowviz_fixtures import (CASES, F, MEASURED_ULP, SHARE_BAR, UPSAMPLE_SHAPES, coarse_maps, golden,  # noqa: E402
                              odd_field)


# ---- the definition -------------------------------------------------------------------------------------------------------------
def test_wheel_is_the_published_one():
    w = M.WHEEL
    assert w.shape == (55, 3) and sum(M.WHEEL_SEGMENTS) == 55
    starts = np.cumsum((0,) + M.WHEEL_SEGMENTS[:-1])
    primaries = [(255, 0, 0), (255, 255, 0), (0, 255, 0), (0, 255, 255), (0, 0, 255), (255, 0, 255)]
    assert [tuple(w[s]) for s in starts] == primaries
    assert tuple(w[14]) == (255, 255 * 14 // 15, 0) and tuple(w[54]) == (255, 0, 255 - 255 * 5 // 6)
    from datasets.utils import flow_viz
    assert np.array_equal(flow_viz.make_colorwheel(), w.astype(np.float64)) and flow_viz.make_colorwheel().dtype == np.float64


def test_model_against_the_reference_goldens():
    differ = total = 0
    for name in CASES:
        field, image, clip, bgr = golden(name)
        got = M.flow_to_image(field, clip, bgr)
        d = np.abs(got.astype(np.int32) - image.astype(np.int32))
        assert d.max() <= 1, (name, int(d.max()))
        if name == "anchors":
            assert np.array_equal(got, image)
        differ, total = differ + int((d > 0).sum()), total + d.size
    print(f"bytes that differ from the reference: {differ} of {total} = {differ / total:.2e}")
    assert differ / total <= SHARE_BAR, (differ, total)
    field, image, _, _ = golden("sides")
    rad = np.sqrt((field.astype(np.float64) ** 2).sum(-1)) / (np.sqrt(24 ** 2 + 32 ** 2) + 1e-5)
    assert (rad > 1).mean() > 0.1 and (rad < 1).mean() > 0.1 and np.abs(rad - 1).min() >= 1e-4


def test_exact_anchors():
    """(0, 0) is white; a displacement along an axis or a diagonal has a = k / 4 exactly, whatever its length, and lands on the
    colour the definition gives for fk = (a + 1) / 2 * 54 at that angle."""
    assert M.flow_to_image(np.zeros((3, 5, 2), F)).tolist() == np.full((3, 5, 3), 255).tolist()
    assert (M.flow_to_image(np.zeros((3, 5, 2), F), norm="max") == 255).all()
    dirs = {(1, 0): 0.0, (1, 1): 0.25, (0, 1): 0.5, (-1, 1): 0.75, (-1, 0): 1.0, (-1, -1): -0.75, (0, -1): -0.5, (1, -1): -0.25}
    for (x, y), want in dirs.items():
        for m in (1e-30, 0.37, 1.0, 3.0, 1e30):
            assert float(M.turn_of(F(m) * F(y), F(m) * F(x))) == want, (x, y, m)
    assert float(M.turn_of(F(-0.0), F(-1))) == -1.0 and float(M.turn_of(F(0.0), F(-1))) == 1.0     # numpy's arctan2(-+0, -1) = -+pi
    assert float(M.turn_of(F(-0.0), F(-0.0))) == -1.0 and float(M.turn_of(F(0.0), F(0.0))) == 0.0
    # the colours on those angles inside the unit radius, from the definition in exact rationals
    from fractions import Fraction as Q
    h, w, m = 6, 10, 2.0
    rad_max = float(M.diag_rad_max(h, w))
    for (x, y), a in dirs.items():
        field = np.zeros((h, w, 2), F)
        field[2, 3] = (-m * x, -m * y)                      # a = atan2(-v, -u) / pi
        fk = (Q(a) + 1) / 2 * 54
        k0 = int(fk)
        f = fk - k0
        length = m * (2 ** 0.5 if x and y else 1.0)
        for ch in range(3):
            col = ((1 - f) * int(M.WHEEL[k0, ch]) + f * int(M.WHEEL[(k0 + 1) % 55, ch])) / 255
            want = 255 * (1 - length / rad_max * (1 - float(col)))
            assert col == 1 or abs(want - round(want)) > 1e-3      # no byte boundary (a full channel is 255 exactly)
            assert int(M.flow_to_image(field)[2, 3, ch]) == int(want), (x, y, ch)


def test_angle_is_accurate():
    """turn_of against float64 arctan2 / pi: the polynomial's 6e-9, five roundings of at most half an ulp of 1/4 (1.5e-8) on
    the way to the octant and at most two of half an ulp of 1 (6e-8) in placing it: below 2^-23."""
    rng = np.random.default_rng(3)
    y, x = rng.normal(size=200000).astype(F), rng.normal(size=200000).astype(F)
    err = np.abs(M.turn_of(y, x).astype(np.float64) - np.arctan2(y.astype(np.float64), x.astype(np.float64)) / np.pi)
    print(f"largest angle error {err.max():.3e} turns/2")
    assert err.max() < 2.0 ** -23


def test_non_finite_pixels_clip_and_bgr():
    f = odd_field(9, 11)
    img = M.flow_to_image(f)
    assert img.reshape(-1, 3)[[1, 3, 5]].tolist() == [[0, 0, 0]] * 3 and img.reshape(-1, 3)[7].tolist() == [255, 255, 255]
    assert np.array_equal(M.flow_to_image(f, convert_to_bgr=True), img[..., ::-1])
    clipped = np.where(np.isfinite(f), np.clip(f, 0, 3.0), f)                               # [0, clip]: negatives become 0
    assert np.array_equal(M.flow_to_image(f, 3.0), M.flow_to_image(clipped.astype(F)))
    assert float(M.radius_max(f)) == float(np.sqrt((f[np.isfinite(f).all(-1)] ** 2).sum(-1, dtype=F)).max())
    assert float(M.radius_max(np.full((2, 2, 2), np.nan, F))) == 0.0


# ---- the sanitised CPU restatement ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("flowviz_host_check")
    exe = build_host_check("flowviz", tmp)

    def run(mode, head, body=None):
        (tmp / "in.bin").write_bytes(struct.pack("<i", mode) + head + (b"" if body is None else np.asarray(body, "<f4").tobytes()))
        out = tmp / "out.bin"
        if out.exists():
            out.unlink()
        p = subprocess.run([str(exe), str(tmp / "in.bin"), str(out)], capture_output=True, text=True)
        assert p.returncode == 0 and p.stderr == "", (p.returncode, p.stderr[-2000:])      # a status, never a sanitizer report
        return int(p.stdout), (out.read_bytes() if out.exists() else None)
    return run


def _pictures(run, fields, norm, clip, bgr):
    n, h, w = fields.shape[:3]
    status, out = run(0, struct.pack("<iiiiif", n, h, w, M.NORMS.index(norm), int(bgr), -1.0 if clip is None else clip), fields)
    assert status == 0
    img = np.frombuffer(out, np.uint8, n * h * w * 3).reshape(n, h, w, 3)
    return img, (np.frombuffer(out, F, n, img.size) if norm == "max" else None)


@pytest.mark.parametrize("norm", M.NORMS)
def test_host_check_equals_the_model_on_the_goldens(host_check, norm):
    for name in CASES:
        field, _, clip, bgr = golden(name)
        img, largest = _pictures(host_check, np.stack([field, field[::-1].copy()]), norm, clip, bgr)
        assert np.array_equal(img[0], M.flow_to_image(field, clip, bgr, norm)), name
        assert np.array_equal(img[1], M.flow_to_image(field[::-1], clip, bgr, norm)), name
        if norm == "max":
            assert largest[0] == M.radius_max(field, clip) == largest[1]


@pytest.mark.parametrize("h,w", [(1, 1), (1, 67), (67, 1), (33, 31)])
def test_host_check_equals_the_model_on_odd_sizes(host_check, h, w):
    f = odd_field(h, w)
    for norm in M.NORMS:
        for clip, bgr in ((None, False), (0.4 * max(h, w), True)):
            img, largest = _pictures(host_check, f[None], norm, clip, bgr)
            assert np.array_equal(img[0], M.flow_to_image(f, clip, bgr, norm)), (norm, clip)
            if norm == "max":
                assert largest[0] == M.radius_max(f, clip)
    status, out = host_check(1, struct.pack("<iiif", 1, h, w, -1.0), f)
    assert status == 0 and np.frombuffer(out, F)[0] == M.radius_max(f)


@pytest.mark.parametrize("g,h,w", UPSAMPLE_SHAPES + ((8, 33, 31),))
def test_host_check_upsamples_and_fuses_as_the_model(host_check, g, h, w):
    flow = coarse_maps(g)
    status, out = host_check(2, struct.pack("<iiii", 2, g, h, w), flow)
    want = np.stack([M.full_uv(m, h, w) for m in flow])
    assert status == 0 and np.array_equal(np.frombuffer(out, np.uint32), want.reshape(-1).view(np.uint32))
    for norm in M.NORMS:
        status, out = host_check(3, struct.pack("<iiiiii", 2, g, h, w, M.NORMS.index(norm), 0), flow)
        pics = np.stack([M.flow_picture(m, h, w, norm) for m in flow])
        assert status == 0 and np.array_equal(np.frombuffer(out, np.uint8, pics.size).reshape(pics.shape), pics), norm
        if norm == "max":
            assert np.frombuffer(out, F, 2, pics.size).tolist() == [float(M.radius_max(u)) for u in want]


def test_host_check_refuses_with_a_status(host_check):
    for n, h, w in ((1, 0, 5), (1, 5, 0), (1, 16385, 5), (1, 5, 16385), (65536, 5, 5), (-1, 5, 5)):
        assert host_check(0, struct.pack("<iiiiif", n, h, w, 0, 0, -1.0)) == (-50, None)
        assert host_check(1, struct.pack("<iiif", n, h, w, -1.0)) == (-50, None)
        assert host_check(2, struct.pack("<iiii", n, 8, h, w)) == (-50, None)
        assert host_check(3, struct.pack("<iiiiii", n, 8, h, w, 0, 0)) == (-50, None)
    for g in (1, 0, -3, 8193):
        assert host_check(2, struct.pack("<iiii", 1, g, 5, 5)) == (-50, None)
    assert host_check(0, struct.pack("<iiiiif", 1, 5, 5, 2, 0, -1.0)) == (-1, None)          # no such norm
    assert host_check(0, struct.pack("<iiiiif", 1, 5, 5, 0, 0, float("nan"))) == (-1, None)
    assert host_check(3, struct.pack("<iiiiii", 1, 8, 5, 5, -1, 0)) == (-1, None)
    status, out = host_check(0, struct.pack("<iiiiif", 0, 5, 5, 0, 0, -1.0))                  # an empty batch is no refusal
    assert status == 0 and out == b""


# ---- the library's own refusals: before any launch, so they run here -------------------------------------------------------------
def test_entry_points_refuse_before_any_launch():
    import ctypes as C
    from dvd_amd import lib, ops
    raw = lib.raw()
    for n, h, w in ((1, 0, 5), (1, 5, 16385), (65536, 5, 5), (-1, 5, 5)):
        assert raw.dvd_flow_to_image_rgb8(None, n, h, w, 0, C.c_float(-1), 0, None, None, None, None) == -50
        assert raw.dvd_flow_radius_max(None, n, h, w, C.c_float(-1), None, None, None) == -50
        assert raw.dvd_flow_full_uv(None, n, 8, h, w, None, None) == -50
        assert raw.dvd_flow_picture_rgb8(None, n, 8, h, w, 0, 0, None, None, None, None) == -50
        assert raw.dvd_flow_workspace_bytes(n, h, w) == -50
    assert raw.dvd_flow_full_uv(None, 1, 1, 5, 5, None, None) == -50 and raw.dvd_flow_picture_rgb8(None, 1, 8193, 5, 5, 0, 0, None, None, None, None) == -50
    assert raw.dvd_flow_to_image_rgb8(None, 1, 5, 5, 2, C.c_float(-1), 0, None, None, None, None) == -1
    assert raw.dvd_flow_to_image_rgb8(None, 1, 5, 5, 0, C.c_float(-1), 0, None, None, None, None) == -1 and b"null" in raw.dvd_last_error()
    assert raw.dvd_flow_to_image_rgb8(None, 0, 5, 5, 0, C.c_float(-1), 0, None, None, None, None) == 0
    assert raw.dvd_flow_workspace_bytes(3, 64, 64) == 3 * 4 and raw.dvd_flow_workspace_bytes(1, 65, 64) == 8
    assert "dvd_flow_workspace_bytes" in lib.NON_STATUS and lib.RESTYPES["dvd_flow_workspace_bytes"] is C.c_long
    assert lib.E_FLOW_SHAPE == -50 and ops.FLOW_NORMS == {"diag": 0, "max": 1}


def test_ops_refuse_bad_arguments_and_host_tensors():
    from dvd_amd import lib, ops
    field, flow = torch.zeros(5, 7, 2), torch.zeros(2, 8, 8)
    for bad in (dict(norm="median"), dict(norm=None), dict(clip_flow=-1.0), dict(clip_flow=float("nan")), dict(clip_flow="3")):
        with pytest.raises(ValueError, match="flow_to_image"):
            ops.flow_to_image(field, **bad)
    for bad in (torch.zeros(5, 7, 3), torch.zeros(5, 7), torch.zeros(5, 7, 2, dtype=torch.float64), torch.zeros(7, 5, 2).transpose(0, 1),
                torch.zeros(0, 7, 2), np.zeros((5, 7, 2), F)):
        with pytest.raises(ValueError, match="flow_to_image"):
            ops.flow_to_image(bad)
        with pytest.raises(ValueError, match="flow_radius_max"):
            ops.flow_radius_max(bad)
    for bad in (torch.zeros(3, 8, 8), torch.zeros(2, 8, 9), torch.zeros(2, 1, 1), torch.zeros(2, 8, 8, dtype=torch.float16)):
        with pytest.raises(ValueError, match="flow_full_uv"):
            ops.flow_full_uv(bad, 5, 5)
        with pytest.raises(ValueError, match="flow_picture"):
            ops.flow_picture(bad, 5, 5)
    for h, w in ((0, 5), (5, 16385), (5.0, 5), (True, 5)):
        with pytest.raises(ValueError, match="flow_full_uv"):
            ops.flow_full_uv(flow, h, w)
        with pytest.raises(ValueError, match="flow_picture"):
            ops.flow_picture(flow, h, w, norm="max")
    with pytest.raises(ValueError, match="flow_picture"):
        ops.flow_picture(flow, 5, 5, norm="both")
    with pytest.raises(ValueError, match="one map per file"):
        ops.flow_write_flo(torch.zeros(2, 2, 8, 8), 5, 5, "never.flo")
    with pytest.raises(ValueError, match="huffman"):
        ops.flow_picture_to_file(flow, 5, 5, "never.png", huffman="best")
    for call in (lambda: ops.flow_to_image(field), lambda: ops.flow_radius_max(field), lambda: ops.flow_full_uv(flow, 5, 5),
                 lambda: ops.flow_picture(flow, 5, 5), lambda: ops.flow_write_flo(flow, 5, 5, "never.flo")):
        with pytest.raises(lib.DvdError, match="device tensor"):                                # host tensors: no CPU path
            call()
    assert not os.path.exists("never.flo") and not os.path.exists("never.png")


# ---- .flo -----------------------------------------------------------------------------------------------------------------------
def test_flo_round_trips_to_the_bit(tmp_path):
    from dvd_amd import ops
    field = odd_field(7, 5)
    field[0, 0] = (-0.0, np.float32(1e-42))
    path = str(tmp_path / "a.flo")
    assert ops.flo_write(field, path) == 12 + 7 * 5 * 8 == os.path.getsize(path)
    data = open(path, "rb").read()
    assert data[:12] == struct.pack("<fii", 202021.25, 5, 7) and data[:4] == b"PIEH" and data == M.flo_bytes(field)
    back = ops.flow_read_flo(path)
    assert back.dtype == np.float32 and back.shape == (7, 5, 2) and np.array_equal(back.view(np.uint32), field.view(np.uint32))
    for bad in (data[:11], b"PIEG" + data[4:], data[:-1], data + b"\0", struct.pack("<fii", 202021.25, 0, 7)):
        (tmp_path / "bad.flo").write_bytes(bad)
        with pytest.raises(ValueError, match="bad.flo"):
            ops.flow_read_flo(str(tmp_path / "bad.flo"))
    with pytest.raises(ValueError, match="flo_write"):
        ops.flo_write(field.astype(np.float64), path)


# ---- the up-sampled field -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g,h,w", UPSAMPLE_SHAPES)
def test_upsampled_field_against_torch_and_float64(g, h, w):
    worst = 0.0
    for m in coarse_maps(g):
        got = M.upsample(m, h, w)
        want = torch.nn.functional.interpolate(torch.from_numpy(m[None]), (h, w), mode="bilinear", align_corners=True)[0].numpy()
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))                       # measured: no element differs
        ulp = float(np.spacing(np.abs(m).max()))
        worst = max(worst, float(np.abs(got.astype(np.float64) - M.upsample64(m, h, w)).max()) / ulp)
    print(f"G = {g} -> {h} x {w}: {worst:.2f} ulp of the map's largest value against float64")
    assert worst <= 2 * MEASURED_ULP[(g, h, w)]


def test_fma32_is_one_rounding():
    """Against exact rationals, on operands chosen so that the float64 sum is itself inexact (where two roundings can differ)."""
    from fractions import Fraction as Q
    rng = np.random.default_rng(5)
    a, b = rng.normal(size=4000).astype(F), rng.normal(size=4000).astype(F)
    c = (-(a.astype(np.float64) * b.astype(np.float64)) * (1 + rng.normal(size=4000) * 1e-7) + rng.normal(size=4000) * 1e-9).astype(F)
    c[:1000] = rng.normal(size=1000).astype(F) * F(1e8)
    got = M.fma32(a, b, c)
    for i in range(0, 4000, 7):
        exact = Q(float(a[i])) * Q(float(b[i])) + Q(float(c[i]))
        lo = np.float32(float(exact))                        # float() of a Fraction rounds correctly to float64: a candidate
        cands = sorted({float(lo), float(np.nextafter(lo, F(np.inf))), float(np.nextafter(lo, F(-np.inf)))}, key=lambda v: abs(Q(v) - exact))
        assert abs(Q(float(got[i])) - exact) == abs(Q(cands[0]) - exact), i


# ---- settings.flow_outputs ------------------------------------------------------------------------------------------------------
def _settings(**attrs):
    import admin.settings as ws
    s = ws.Settings()
    s.name, s.seed = "pytest_flowviz", 5
    for k, v in attrs.items():
        setattr(s, k, v)
    return s


LOG = types.SimpleNamespace(info=lambda *a: None)


def _exploding_loader():
    raise AssertionError("the loader was read")
    yield                                                                          # pragma: no cover


def _flow_outputs_of(settings):
    from dvd_amd import evaluation
    return evaluation.RoundOptions.from_settings(settings).flow_outputs


def test_flow_outputs_parsing():
    from dvd_amd import evaluation
    assert evaluation.FLOW_OUTPUTS == ("png", "flo", "npy")
    assert _flow_outputs_of(_settings()) == () and _flow_outputs_of(_settings(flow_outputs="")) == ()
    assert _flow_outputs_of(_settings(flow_outputs="png")) == ("png",)
    assert _flow_outputs_of(_settings(flow_outputs="npy, png")) == ("png", "npy")
    assert _flow_outputs_of(_settings(flow_outputs="flo,npy,png")) == ("png", "flo", "npy")


def test_a_bad_flow_outputs_is_refused_before_the_loader_is_read(tmp_path, monkeypatch):
    from dvd_amd import evaluation
    monkeypatch.chdir(tmp_path)
    for value in ("jpg", "png,png", "png,", ",", " ", "PNG", None, True, 3, ("png",), ["png"]):
        with pytest.raises(ValueError, match="settings.flow_outputs"):
            evaluation.run_evaluation_docunet(_settings(flow_outputs=value), LOG, _exploding_loader(), None, torch.nn.Linear(1, 1), None)
    assert list(tmp_path.iterdir()) == []


class _OpsSpy:
    """dvd_amd.ops with every flow_* entry recorded (and answered on the host, where one is called)."""

    def __init__(self, real):
        self._real, self.calls = real, []

    def __getattr__(self, name):
        if name.startswith(("flow_", "flo_")):
            def record(*a, **k):
                self.calls.append(name)
                return (12, 1.5) if name == "flow_picture_to_file" else 12
            return record
        return getattr(self._real, name)


def _emit(monkeypatch, tmp_path, **attrs):
    from dvd_amd import evaluation
    from dvd_amd.run_options import RunOptions
    monkeypatch.chdir(tmp_path)
    spy = _OpsSpy(evaluation.ops)
    monkeypatch.setattr(evaluation, "ops", spy)
    s = _settings(**attrs)
    s.env.visualize = False
    lines, results = [], []
    batch = [{"path": "a.png"}, {"path": "dir/b_1 copy.jpg"}, {"path": "synthetic_00002"}]
    outs = [torch.zeros(6, 4, 3, dtype=torch.uint8)] * 3
    flow = torch.arange(3 * 2 * 8 * 8, dtype=torch.float32).reshape(3, 2, 8, 8)
    extra = {"flow": flow, "flow_outputs": _flow_outputs_of(s)} if _flow_outputs_of(s) else {}
    evaluation.emit(s, types.SimpleNamespace(info=lines.append), batch, outs, results, RunOptions.from_env(s.env), "cpu", **extra)
    assert [p for p, _ in results] == [d["path"] for d in batch]
    return spy, lines, flow


def test_absent_attribute_calls_nothing_new(monkeypatch, tmp_path):
    for attrs in ({}, {"flow_outputs": ""}):
        spy, lines, _ = _emit(monkeypatch, tmp_path, **attrs)
        assert spy.calls == [] and lines == [] and list(tmp_path.iterdir()) == []


def test_set_attribute_writes_per_document_under_the_page_stem(monkeypatch, tmp_path):
    spy, lines, flow = _emit(monkeypatch, tmp_path, flow_outputs="png,flo,npy")
    assert spy.calls == ["flow_picture_to_file", "flow_write_flo"] * 3
    assert lines == [f"{p} flow_rad_max 1.500000" for p in ("a.png", "dir/b_1 copy.jpg", "synthetic_00002")]
    out = tmp_path / "vis_hp" / "synthetic" / "pytest_flowviz" / "pred_flow"
    assert sorted(f.name for f in out.iterdir()) == ["flow_a.npy", "flow_b_1 copy.npy", "flow_synthetic_00002.npy"]
    assert np.array_equal(np.load(out / "flow_b_1 copy.npy"), flow[1].numpy())
    spy, lines, _ = _emit(monkeypatch, tmp_path, flow_outputs="flo")
    assert spy.calls == ["flow_write_flo"] * 3 and lines == []


def test_launcher_flag_reaches_settings(tmp_path, monkeypatch):
    import run_sampling as R
    monkeypatch.chdir(tmp_path)
    seen = []
    monkeypatch.setattr(R, "importlib", types.SimpleNamespace(import_module=lambda name: types.SimpleNamespace(
        run=lambda settings: seen.append((settings.name, getattr(settings, "flow_outputs", None))))))
    monkeypatch.setattr(R, "shutil", types.SimpleNamespace(copyfile=lambda *a: None))
    R.run_sampling("dvd", "val_TDiff", 3, "exp")
    R.run_sampling("dvd", "val_TDiff", 3, "exp", flow_outputs="")
    R.run_sampling("dvd", "val_TDiff", 3, "exp", flow_outputs="png,flo")
    assert seen == [("exp", None), ("exp", None), ("exp", "png,flo")]
    seen.clear()
    R.run_sampling("dvd", "val_TDiff", 3, "exp", severity=3, corruption_number=10, keyed_noise=True, flow_outputs="npy")
    assert seen == [("exp", "npy"), ("exp/c10_brightness_s3", "npy")]                          # every round under its own run name
    monkeypatch.setattr(sys, "argv", ["run_sampling.py", "--train_module", "dvd", "--train_name", "val_TDiff", "--name", "cli",
                                      "--flow_outputs", "png,npy"])
    seen.clear()
    R.main()
    assert seen == [("cli", "png,npy")]


# ---- apply_map ------------------------------------------------------------------------------------------------------------------
def test_apply_map_checks_its_arguments(tmp_path):
    from dvd_amd import apply_map as A
    for bad in (np.zeros((3, 8, 8), F), np.zeros((2, 8, 9), F), np.zeros((2, 1, 1), F), np.zeros((2, 8, 8), np.int32), np.zeros((8, 8), F)):
        np.save(tmp_path / "bad.npy", bad)
        with pytest.raises(ValueError, match="bad.npy"):
            A.load_map(str(tmp_path / "bad.npy"))
    np.save(tmp_path / "good.npy", np.ones((2, 8, 8), np.float64))
    m = A.load_map(str(tmp_path / "good.npy"))
    assert m.shape == (1, 2, 8, 8) and m.dtype == np.float32
    with pytest.raises(ValueError, match="--mode"):
        A.apply_map(str(tmp_path / "good.npy"), "none.png", str(tmp_path / "out.png"), mode="nearest")
    with pytest.raises(SystemExit):
        A.main(["only_a_map.npy"])
    with pytest.raises(SystemExit):
        A.main([str(tmp_path / "good.npy"), "in.png", "out.png", "--mode", "nearest"])
    assert not (tmp_path / "out.png").exists()
