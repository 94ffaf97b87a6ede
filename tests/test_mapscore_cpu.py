"""The map score without a GPU: the NumPy model against goldens of the real reference's metric modules, the
sanitised CPU restatement against the model, the selection against np.sort on hostile key sets, settings.gt_map_dir from the
launcher to the document loop, the ground-truth lookup, keep_hypotheses, and the table's text."""
import ctypes as C
import os
import struct
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flowviz_model as FV  # noqa: E402
import mapscore_model as M  # noqa: E402
from host_check import build_host_check  # noqa: E402

from mapscore_fixtures import (BARS, CASES, F, MEASURED, check_against_reference, document,  # noqa: E402
                               golden, golden_planes, key_sets, margins_hold)


# ---- the definition against the real reference ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_model_against_the_reference_goldens(name):
    planes, ref = golden_planes(name)
    assert margins_hold(planes)
    got = M.score(planes)
    detail = M.sparsification(planes["e"], planes["sigma"], detail=True)["detail"]
    want = [got["n_valid"] - hi for hi in M.ranks_desc(got["n_valid"])]
    for row, key in enumerate(("sparse", "opt")):                      # the reference's kept sets have N - hi pixels, and so have ours
        assert ref["subs"][row].tolist() == want == detail[key][2][:, 0].tolist(), key
    for k in ("epe", "epe_std"):
        print(f"{name} {k}: {abs(got[k] / float(ref['std' if k == 'epe_std' else k]) - 1):.2e} relative")
    check_against_reference(got, ref)
    assert all(BARS[k] == 4 * MEASURED[k] for k in BARS)


def test_goldens_cover_what_they_are_there_for():
    assert (~golden_planes("invalid")[0]["valid"]).sum() == 20 * 37                    # NaN, +-inf, 1e10 and -2e9 pixels
    planes, _ = golden_planes("still")
    ok = planes["valid"]
    e = planes["e"][ok].view(F)
    assert ((planes["m"][ok] == 0) & (e > 3)).sum() > 100                              # Fl where |gt| = 0: e / 0 = inf counts
    for name in CASES:
        pred, gt, sigma, _ = golden(name)
        assert pred.shape[0] <= 100 and pred.shape[1] <= 100 and pred.shape == gt.shape and sigma.shape == pred.shape[:2]


def test_definition_details():
    e = np.asarray([0.0, 1.0, 1.5, 3.0, 5.0, 7.0], F)
    planes = {"e": e.view(np.uint32), "sigma": np.zeros(6, np.uint32), "m": np.asarray([1, 1, 0, 100, 0, 1000], F), "valid": np.ones(6, bool)}
    got = M.score(planes, sparsify=False)
    assert (got["pck1"], got["pck3"], got["pck5"], got["n_valid"]) == (2 / 6, 4 / 6, 5 / 6, 6)
    assert got["fl"] == 1 / 6                                  # 5.0 over m = 0 counts; 7 / 1000 and 3.0 (not > 3) do not
    assert got["epe"] == 17.5 / 6 and got["epe_std"] == pytest.approx(np.std(e.astype(np.float64), ddof=1), rel=1e-12)
    assert M.ranks_desc(1) == [0] * 50 and M.ranks_desc(101)[:3] == [0, 2, 4] and M.ranks_desc(102)[1] == 3       # ceil
    assert int(M.fixed_of(F(1e9))) == 2 ** 35 and int(M.fixed_of(F(0.5))) == 2 ** 19 and 2 ** 28 * 2 ** 35 <= 2 ** 63
    one = M.score({"e": e[:1].view(np.uint32), "sigma": e[:1].view(np.uint32), "m": e[:1], "valid": np.ones(1, bool)})
    assert one["epe"] == 0.0 and np.isnan(one["epe_std"]) and one["AUSE"]["EPE"] == 0.0
    none = M.score({"e": np.full(3, M.INVALID), "sigma": np.full(3, M.INVALID), "m": np.zeros(3, F), "valid": np.zeros(3, bool)})
    assert none["n_valid"] == 0 and np.isnan(none["epe"]) and "AUSE" not in none
    # a perfect spread (sigma = e) is the oracle: AUSE 0; all ties (sigma constant) keep everything: a flat curve
    planes, _ = golden_planes("page")
    assert M.sparsification(planes["e"], planes["e"])["AUSE"] == {"EPE": 0.0, "PCK1": 0.0, "PCK5": 0.0}
    flat = M.sparsification(planes["e"], np.where(planes["valid"], np.uint32(0), M.INVALID))
    assert len(set(flat["sparse_curve"]["EPE"][:50].tolist())) == 1
    # a map against itself
    flow, _, hyps = document(33, 31)
    own = M.score(M.errors_of_maps(flow, FV.full_uv(flow, 33, 31), hyps, 33, 31))
    assert own["epe"] == 0.0 and own["epe_std"] == 0.0 and own["pck1"] == 1.0 and own["fl"] == 0.0 and own["n_valid"] == 1023


# ---- the sanitised CPU restatement ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("mapscore_host_check")
    exe = build_host_check("mapscore", tmp)

    def run(mode, head, *bodies):
        data = struct.pack("<i", mode) + head + b"".join(np.ascontiguousarray(b).tobytes() for b in bodies)
        (tmp / "in.bin").write_bytes(data)
        out = tmp / "out.bin"
        if out.exists():
            out.unlink()
        p = subprocess.run([str(exe), str(tmp / "in.bin"), str(out)], capture_output=True, text=True)
        assert p.returncode == 0 and p.stderr == "", (p.returncode, p.stderr[-2000:])      # a status, never a sanitizer report
        return int(p.stdout), (out.read_bytes() if out.exists() else None)
    return run


def _document(run, flow, gt, hyps, h, w):
    """mode 0 -> (e, sigma, counts, sum e, sum e^2, {key: (thresholds, bins)})."""
    flow, gt = np.asarray(flow, F), np.asarray(gt, F)
    g = 0 if flow.shape == (h, w, 2) else flow.shape[-1]
    gt_g = 0 if gt.shape == (h, w, 2) else gt.shape[-1]
    n_hyp = 1 if hyps is None else len(hyps)
    bodies = [flow, gt] + ([np.asarray(hyps, F)] if n_hyp >= 2 else [])
    status, out = run(0, struct.pack("<iiiii", g, gt_g, n_hyp, h, w), *bodies)
    assert status == 0
    n = h * w
    e, sigma = np.frombuffer(out, np.uint32, n), np.frombuffer(out, np.uint32, n, 4 * n)
    counts = np.frombuffer(out, np.uint64, 5, 8 * n)
    se, se2 = np.frombuffer(out, np.float64, 2, 8 * n + 40)
    rest, parts = 8 * n + 56, {}
    if counts[0]:
        for key in ("sparse", "opt"):
            parts[key] = (np.frombuffer(out, np.uint32, 50, rest), np.frombuffer(out, np.uint64, 204, rest + 200).reshape(51, 4))
            rest += 200 + 204 * 8
    assert rest == len(out)
    return e, sigma, counts, float(se), float(se2), parts


def _check_document(run, flow, gt, hyps, h, w):
    planes = M.errors_of_maps(flow, gt, hyps, h, w) if np.asarray(flow).shape != (h, w, 2) else M.errors(flow, gt)
    e, sigma, counts, se, se2, parts = _document(run, flow, gt, hyps, h, w)
    assert np.array_equal(e, planes["e"]) and np.array_equal(sigma, planes["sigma"])                 # bit for bit
    want, wse, wse2 = M.headline(planes)
    assert counts.tolist() == [want[k] for k in ("n_valid", "n1", "n3", "n5", "n_fl")]
    assert abs(se - wse) <= 1e-9 * wse and abs(se2 - wse2) <= 1e-9 * wse2
    if want["n_valid"]:
        detail = M.sparsification(planes["e"], planes["sigma"], detail=True)["detail"]
        for key in ("sparse", "opt"):
            assert np.array_equal(parts[key][0], detail[key][0]), key                                # the 50 order statistics
            assert np.array_equal(parts[key][1], detail[key][1]), key                                # the integer sums
    return want["n_valid"]


@pytest.mark.parametrize("name", CASES)
def test_host_check_equals_the_model_on_the_goldens(host_check, name):
    pred, gt, _, _ = golden(name)
    assert _check_document(host_check, pred, gt, None, *pred.shape[:2]) > 1000


@pytest.mark.parametrize("h,w", [(1, 1), (1, 67), (67, 1), (33, 31)])
def test_host_check_equals_the_model_on_odd_sizes(host_check, h, w):
    flow, gt, hyps = document(h, w)
    _check_document(host_check, flow, gt, hyps, h, w)
    _check_document(host_check, flow, gt, hyps[:2], h, w)
    _check_document(host_check, flow, gt, None, h, w)                                  # H = 1: sigma = 0, every key equal
    _check_document(host_check, flow, document(h, w, seed=5)[0], hyps, h, w)           # a coarse ground truth [2,g,g]
    _check_document(host_check, flow, np.full((h, w, 2), np.nan, F), hyps, h, w)       # no valid pixel


def _select(run, keys, ranks):
    return run(1, struct.pack("<ii", len(keys), len(ranks)), np.asarray(ranks, np.uint32), np.asarray(keys, np.uint32))


@pytest.mark.parametrize("name", sorted(key_sets()))
def test_selection_against_sort_on_hostile_keys(host_check, name):
    keys = key_sets()[name]
    n, order = len(keys), np.sort(keys)
    n_valid = int((keys != M.INVALID).sum())
    for ranks in ([0], [n - 1], [0, n - 1], sorted({0, n // 3, n // 2, n - 1}), [n // 2] * 50, list(np.linspace(0, n - 1, 50).astype(int)),
                  sorted(n_valid - 1 - hi for hi in M.ranks_desc(n_valid))):
        status, out = _select(host_check, keys, ranks)
        assert status == 0 and np.array_equal(np.frombuffer(out, np.uint32), order[ranks]), (name, ranks[:4])
    # and through the model's descending ranks, invalid keys skipped
    assert np.array_equal(M.select_desc(keys, M.ranks_desc(n_valid)), np.sort(keys[keys != M.INVALID])[::-1][M.ranks_desc(n_valid)])


def test_host_check_refusals(host_check):
    from dvd_amd import lib
    keys = key_sets()["few"]
    for ranks in ([17], [3, 2], list(range(17)) * 3):                                  # beyond n, decreasing, more than 50
        assert _select(host_check, keys, ranks) == (lib.E_MAP_RANKS, None)
    assert _select(host_check, keys, []) == (lib.E_MAP_RANKS, None)
    for head in ((1, 0, 1, 4, 4), (8193, 0, 1, 4, 4), (8, 1, 1, 4, 4), (8, 0, 0, 4, 4), (8, 0, 65, 4, 4), (8, 0, 1, 0, 4), (8, 0, 1, 4, 16385),
                 (0, 0, 2, 4, 4)):
        assert host_check(0, struct.pack("<iiiii", *head)) == (lib.E_MAP_SHAPE, None), head


# ---- the library and ops refuse before any launch ---------------------------------------------------------------------------------
def test_library_refuses_before_any_launch():
    from dvd_amd import lib
    raw = lib.raw()
    one = C.c_void_p(256)            # non-null and aligned; never dereferenced: every call below is refused
    assert lib.E_MAP_SHAPE == -51 and lib.E_MAP_RANKS == -52 and lib.E_FLOW_SHAPE == -50
    for g, gt_g, n_hyp, h, w in ((1, 0, 1, 4, 4), (8193, 0, 1, 4, 4), (8, 1, 1, 4, 4), (8, 8193, 1, 4, 4), (8, 0, 0, 4, 4), (8, 0, 65, 4, 4),
                                 (8, 0, 1, 0, 4), (8, 0, 1, 4, 0), (8, 0, 1, 16385, 4), (0, 0, 2, 4, 4)):
        assert raw.dvd_map_errors(one, g, one, gt_g, one, n_hyp, h, w, one, one, one, None) == lib.E_MAP_SHAPE
    assert raw.dvd_map_errors(None, 8, one, 0, None, 1, 4, 4, one, one, one, None) == -1
    assert raw.dvd_map_errors(one, 8, one, 0, None, 2, 4, 4, one, one, one, None) == -1                      # H = 2 without hypotheses
    assert raw.dvd_map_errors(one, 8, C.c_void_p(260), 0, None, 1, 4, 4, one, one, one, None) == -1          # a field is 8-byte aligned
    assert raw.dvd_map_errors(one, 8, one, 0, None, 1, 4, 4, one, one, C.c_void_p(64), None) == -1
    assert raw.dvd_map_metrics(one, 0, 4, one, None) == lib.E_MAP_SHAPE and raw.dvd_map_metrics(None, 4, 4, one, None) == -1
    ranks = (C.c_uint32 * 3)(0, 5, 9)
    assert raw.dvd_select_u32(one, 0, ranks, 3, one, one, None) == lib.E_MAP_SHAPE
    assert raw.dvd_select_u32(one, 2 ** 28 + 1, ranks, 3, one, one, None) == lib.E_MAP_SHAPE
    assert raw.dvd_select_u32(one, 9, ranks, 3, one, one, None) == lib.E_MAP_RANKS                            # a rank of n
    assert raw.dvd_select_u32(one, 10, (C.c_uint32 * 2)(5, 4), 2, one, one, None) == lib.E_MAP_RANKS
    assert raw.dvd_select_u32(one, 10, ranks, 0, one, one, None) == lib.E_MAP_RANKS
    assert raw.dvd_select_u32(one, 10, ranks, 51, one, one, None) == lib.E_MAP_RANKS
    assert raw.dvd_select_u32(one, 10, None, 3, one, one, None) == lib.E_MAP_RANKS
    assert raw.dvd_select_u32(None, 10, ranks, 3, one, one, None) == -1
    assert raw.dvd_sparsify_bins(one, one, 0, one, 50, one, one, None) == lib.E_MAP_SHAPE
    assert raw.dvd_sparsify_bins(one, one, 10, one, 51, one, one, None) == lib.E_MAP_RANKS
    assert raw.dvd_sparsify_bins(one, one, 10, None, 50, one, one, None) == -1
    assert raw.dvd_mapscore_workspace_bytes(0, 4) == lib.E_MAP_SHAPE and raw.dvd_mapscore_workspace_bytes(4, 16385) == lib.E_MAP_SHAPE
    small, page = raw.dvd_mapscore_workspace_bytes(1, 1), raw.dvd_mapscore_workspace_bytes(3508, 2480)
    assert small % 256 == 0 and page - small >= 2 * 4 * 3508 * 2480 and page - small < 2 * 4 * 3508 * 2480 + 7 * 8 * 8500 + 2048
    assert "dvd_mapscore_workspace_bytes" in lib.NON_STATUS and lib.RESTYPES["dvd_mapscore_workspace_bytes"] is C.c_long


def test_ops_refuse_before_any_launch(monkeypatch):
    from dvd_amd import lib, ops

    def fail(name, *args):
        raise AssertionError(f"{name} was launched")
    monkeypatch.setattr(lib, "call", fail)
    flow, gt, hyps = torch.zeros(2, 8, 8), torch.zeros(5, 7, 2), torch.zeros(3, 2, 8, 8)
    for fn in (ops.map_errors, ops.map_metrics, ops.map_score):
        with pytest.raises(ValueError, match="on the device"):
            fn(flow, gt, hyps)                                              # host tensors
        with pytest.raises(ValueError, match="on the device"):
            fn(flow.numpy(), gt)
    for fn in (ops.sparsification, lambda e, s: ops.select_kth_desc(e, [0])):
        with pytest.raises(ValueError, match="on the device"):
            fn(torch.zeros(10), torch.zeros(10))
    monkeypatch.setattr(ops, "_map_device", lambda *args: None)             # as if every tensor lived on the device: the shapes
    for a, b, c, size, match in ((torch.zeros(2, 8, 7), gt, None, None, "flow must be"), (torch.zeros(2, 1, 1), gt, None, None, "flow must be"),
                                 (flow, torch.zeros(5, 7, 3), None, None, "gt must be"), (flow, torch.zeros(2, 8, 8), None, (0, 5), "1..16384"),
                                 (flow, torch.zeros(2, 8, 8), None, (5, 16385), "1..16384"), (flow, torch.zeros(2, 8, 9), None, (5, 5), "coarse map"),
                                 (flow, gt, torch.zeros(3, 2, 9, 9), None, "hyps must be"), (flow, gt, torch.zeros(65, 2, 8, 8), None, "hyps must be"),
                                 (torch.zeros(5, 7, 2), gt, torch.zeros(3, 2, 8, 8), None, "without hyps"),
                                 (torch.zeros(5, 6, 2), gt, None, None, "like the ground truth"), (flow, gt, None, 5, "size must be")):
        with pytest.raises(ValueError, match=match):
            ops.map_score(a, b, c, size=size)
    assert ops.map_ranks(1023) == M.ranks_desc(1023) and ops.map_ranks(1) == [0] * 50
    assert ops.MAP_CURVES == M.METRICS and ops.MAP_NO_PIXELS == M.NO_PIXELS and ops.MAP_FIX_SCALE == float(M.FIX_SCALE)
    # the host part of sparsification is the model's, bit for bit
    planes, _ = golden_planes("anti")
    detail = M.sparsification(planes["e"], planes["sigma"], detail=True)
    for key, name in (("sparse", "sparse_curve"), ("opt", "opt_curve")):
        curve = ops._map_curves(detail["detail"][key][1].astype(np.int64).view(np.uint64))
        top = np.asarray(ops._map_curves(detail["detail"]["opt"][1])["EPE"]).max() + 1e-6
        assert np.array_equal(curve["EPE"] / top, detail[name]["EPE"])


def test_kernels_use_no_scratch(tmp_path):
    """hipcc's own report for gfx950 with the library's flags: 0 bytes of scratch in every kernel of mapscore.hip, and the LDS of
    the selection's histogram kernel is its [50][256] u32 table (with the slot table: below 64 KB), the largest of the file."""
    import re
    import shutil
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dvd_amd", "csrc", "mapscore.hip")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=on", "--cuda-device-only", "-c", src, "-o",
                        str(tmp_path / "m.o"), "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, check=True)
    use = re.findall(r"Function Name: (\S+).*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?LDS Size \[bytes/block\]: (\d+)", r.stderr, re.S)
    print(use)
    assert len(use) == 9 and all(int(scratch) == 0 for _, _, scratch, _ in use), use          # map_errors comes in four forms
    lds = {name: int(size) for name, _, _, size in use}
    hist, = (size for name, size in lds.items() if "select_hist" in name)
    assert 50 * 256 * 4 <= hist < 64 * 1024 and max(lds.values()) == hist


# ---- from the settings to the sampling loop ---------------------------------------------------------------------------------------
def _settings(**attrs):
    import admin.settings as ws
    s = ws.Settings()
    s.name, s.seed = "pytest_mapscore", 5
    for k, v in attrs.items():
        setattr(s, k, v)
    return s


LOG = types.SimpleNamespace(info=lambda *a: None)


def _exploding_loader():
    raise AssertionError("the loader was read")
    yield                                                                          # pragma: no cover


def test_a_bad_gt_map_dir_is_refused_before_the_loader_is_read(tmp_path, monkeypatch):
    from dvd_amd import evaluation
    monkeypatch.chdir(tmp_path)
    for value in (1, None, True, ["maps"], str(tmp_path / "missing"), b"maps"):
        with pytest.raises(ValueError, match="settings.gt_map_dir"):
            evaluation.run_evaluation_docunet(_settings(gt_map_dir=value), LOG, _exploding_loader(), None, torch.nn.Linear(1, 1), None)
    assert list(tmp_path.iterdir()) == []
    read = evaluation.RoundOptions.from_settings
    assert read(_settings()).gt_map_dir is None and read(_settings(gt_map_dir="")).gt_map_dir is None
    assert read(_settings(gt_map_dir=str(tmp_path))).gt_map_dir == str(tmp_path)


def test_no_new_env_switch():
    from dvd_amd import run_options
    assert not any("gt_map" in str(row) for row in run_options.TABLE)


def test_lookup_order(tmp_path):
    from dvd_amd import evaluation
    assert evaluation.gt_map_candidates("in/12_1 copy.png") == [
        "12_1 copy.flo", "flow_12_1 copy.flo", "12_1 copy.npy", "flow_12_1 copy.npy", "12.flo", "flow_12.flo", "12.npy", "flow_12.npy"]
    assert evaluation.gt_map_candidates("synthetic_00001") == ["synthetic_00001.flo", "flow_synthetic_00001.flo", "synthetic_00001.npy",
                                                               "flow_synthetic_00001.npy"]
    names = evaluation.gt_map_candidates("a/7_2.jpg")
    assert evaluation.find_gt_map(str(tmp_path), "a/7_2.jpg") is None
    for name in reversed(names):                                            # each earlier candidate wins over the later ones
        (tmp_path / name).write_bytes(b"")
        assert evaluation.find_gt_map(str(tmp_path), "a/7_2.jpg") == str(tmp_path / name)


class _Recorder:
    def __init__(self):
        self.calls = []

    def ddim_sample_loop(self, model, shape, **kw):
        self.calls.append(dict(kw, model=model, shape=shape))
        final = {"hypotheses": torch.ones(shape[0] * 2, *shape[1:])} if kw["sampling_kwargs"].get("keep_hypotheses") else {}
        return torch.zeros(shape), final


def test_hypotheses_come_back_only_when_asked_for():
    from dvd_amd import evaluation
    s, rec = _settings(), _Recorder()
    args = (s, LOG, rec, "MODEL", 4, torch.zeros(1, 3, 8, 8), 16, None, None, None, None, None, None)
    flow = evaluation.run_sample_lr_dewarping(*args)
    assert torch.is_tensor(flow) and set(rec.calls[0]["sampling_kwargs"]) == {"src_img"}
    flow, hyps = evaluation.run_sample_lr_dewarping(*args, keep_hypotheses=True)
    assert rec.calls[1]["sampling_kwargs"]["keep_hypotheses"] is True and tuple(hyps.shape) == (2, 2, 16, 16) and tuple(flow.shape) == (1, 2, 16, 16)
    with pytest.raises(TypeError):                                                                               # keyword only
        evaluation.run_sample_lr_dewarping(*args, None, None, None, None, True)
    batch = [{"path": p, "y512": torch.zeros(3, 8, 8), "mask_cat": torch.zeros(1, 8, 8), "mask_y512": torch.zeros(1, 16, 16),
              "line_msk": torch.zeros(1, 16, 16)} for p in ("a", "b")]
    s.env.grid_size = 16
    assert torch.is_tensor(evaluation.sample_batch(s, LOG, rec, "MODEL", batch, 16, "cpu"))
    assert set(rec.calls[-1]["sampling_kwargs"]) == {"src_img"}
    flow, hyps = evaluation.sample_batch(s, LOG, rec, "MODEL", batch, 16, "cpu", keep_hypotheses=True)
    assert tuple(hyps.shape) == (4, 2, 16, 16)


def test_final_keeps_its_keys_without_keep_hypotheses(monkeypatch):
    """The sampling loop on a stand-in engine: `final` gains "hypotheses" only under sampling_kwargs["keep_hypotheses"] = True."""
    from dvd_amd import gaussian_diffusion, script_util
    seen = []

    def sample(eng, tables, x_T, **kw):
        seen.append(kw)
        mean = torch.zeros(1, 2, 16, 16)
        return (mean, torch.ones(2, 2, 16, 16)) if kw.get("keep_hypotheses") else mean
    monkeypatch.setattr(gaussian_diffusion.sampler, "sample", sample)
    eng = types.SimpleNamespace(prepare=lambda *a: None, feat_nchw=lambda: "FEAT")
    model = types.SimpleNamespace(engine=lambda g, b, n: eng, parameters=lambda: iter([torch.zeros(1)]))
    d = script_util.create_gaussian_diffusion(steps=3, noise_schedule="cosine", predict_xstart=True, rescale_timesteps=True, timestep_respacing="")
    kw = {k: torch.zeros(1, 1, 4, 4) for k in ("y512", "mask_cat", "mask_y512", "line_msk")}
    for extra in ({}, {"keep_hypotheses": False}, {"keep_hypotheses": 1}):
        sample_, final = d.ddim_sample_loop(model, (1, 2, 16, 16), model_kwargs=dict(kw), time_variant=True, n_batch=2,
                                            sampling_kwargs=dict({"src_img": None}, **extra))
        assert set(final) == {"sample", "pred_xstart", "feat_dict"} and "keep_hypotheses" not in seen[-1] and torch.is_tensor(sample_)
    sample_, final = d.ddim_sample_loop(model, (1, 2, 16, 16), model_kwargs=dict(kw), time_variant=True, n_batch=2,
                                        sampling_kwargs={"src_img": None, "keep_hypotheses": True})
    assert set(final) == {"sample", "pred_xstart", "feat_dict", "hypotheses"} and tuple(final["hypotheses"].shape) == (2, 2, 16, 16)
    assert final["sample"] is sample_ and tuple(sample_.shape) == (1, 2, 16, 16)


def _read_flo(path):
    from dvd_amd import ops
    return ops.flow_read_flo(path)


class _ScoreStub:
    """ops.map_score on the host, by the model; ops.flow_read_flo as it is."""
    flow_read_flo = staticmethod(_read_flo)

    def __init__(self):
        self.calls = []

    def map_score(self, flow, gt, hyps=None, size=None):
        self.calls.append((tuple(gt.shape), None if hyps is None else tuple(hyps.shape), size))
        h, w = size if size else gt.shape[:2]
        return M.score(M.errors_of_maps(flow.numpy(), gt.numpy(), None if hyps is None else hyps.numpy(), h, w), sparsify=hyps is not None)


def test_documents_are_scored_logged_and_summarised(tmp_path, monkeypatch):
    from dvd_amd import evaluation, ops
    monkeypatch.chdir(tmp_path)
    stub = _ScoreStub()
    monkeypatch.setattr(evaluation, "ops", stub)
    maps = tmp_path / "maps"
    maps.mkdir()
    flow, _, hyps = document(20, 30, g=8, n_hyp=2)
    other = document(20, 30, g=8, seed=9)[0]
    ops.flo_write(FV.full_uv(flow, 20, 30), str(maps / "flow_a.flo"))                        # its own map: every error 0
    np.save(maps / "b.npy", other)
    lines = []
    log = types.SimpleNamespace(info=lines.append)
    s = _settings(gt_map_dir=str(maps), map_score=[])
    s.env.eval_dataset_name = "synthetic"
    batch = [{"path": p} for p in ("a", "b", "c")]
    outs = [torch.zeros(24, 36, 3, dtype=torch.uint8)] * 3
    t = torch.from_numpy
    evaluation.score_against_gt_maps(s, log, batch, t(np.stack([flow] * 3)), t(np.concatenate([hyps] * 3)), outs, str(maps))
    assert stub.calls == [((20, 30, 2), (2, 2, 8, 8), None), ((2, 8, 8), (2, 2, 8, 8), (24, 36))]     # .flo at its own size, .npy at the page's
    assert [p for p, _ in s.map_score] == ["a", "b"]
    a, b = s.map_score[0][1], s.map_score[1][1]
    assert a["epe"] == 0.0 and a["pck1"] == 1.0 and a["fl"] == 0.0 and b["epe"] > 0
    assert lines[0] == f"a map_score epe 0.000000 pck1 1.000000 pck5 1.000000 fl 0.000000 ause_epe {a['ause_epe']:.6f}"
    assert lines[1].startswith("b map_score epe ") and lines[2] == f"c map_score skipped: no ground-truth map in {maps}"
    lines.clear()
    evaluation.score_against_gt_maps(s, log, batch[:1], t(flow[None]), t(hyps[:1]), outs[:1], str(maps))           # H = 1
    assert lines[0] == "a map_score: one hypothesis, no spread: sparsification skipped" and lines[1].endswith("ause_epe -")
    assert stub.calls[-1][1] is None and "AUSE" not in s.map_score[-1][1]
    s.map_score.pop()
    os.makedirs("vis_hp/synthetic/pytest_mapscore")
    lines.clear()
    evaluation.write_score_sheet(s, log, evaluation.SCORE["map_score"], 3)
    text = (tmp_path / "vis_hp/synthetic/pytest_mapscore/map_score.txt").read_text().splitlines()
    assert text[0] == "path " + " ".join(evaluation.MAP_SCORE_COLUMNS) and text[1].startswith("a 0.000000 0.000000 1.000000") and len(text) == 3
    assert lines[0] == f"mean epe {b['epe'] / 2:.6f} over 2 of 3 documents" and [ln.split()[1] for ln in lines] == list(evaluation.MAP_SCORE_LOGGED)
    assert evaluation.map_score_means(s.map_score, ("epe", "pck5"))["pck5"] == (1.0 + b["pck5"]) / 2


# ---- the launcher -----------------------------------------------------------------------------------------------------------------
def _fake_launch(monkeypatch, R, seen):
    def run(settings):
        seen.append((settings.name, getattr(settings, "gt_map_dir", None)))
        settings.ms_ssim = [("a", 0.5 + settings.corruption_number / 100), ("b", 0.7)]
        if getattr(settings, "gt_map_dir", None) and settings.corruption_number != 1:
            settings.map_score = [("a", {"epe": 1.0, "pck5": 0.5, "ause_epe": 0.25}), ("b", {"epe": 2.0 + settings.corruption_number, "pck5": 1.0})]
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
    assert plain.splitlines()[0] == "no kind severity ms_ssim" and plain.splitlines()[1] == "0 gaussian_noise 5 0.600000"
    assert all(d is None for _, d in seen)                                                   # the attribute stays absent
    R.run_sampling("dvd", "val_TDiff", 3, "exp", corruption=True, gt_map_dir=str(tmp_path))
    scored = table.read_text().splitlines()
    assert seen[-1][1] == str(tmp_path)
    assert scored[0] == "no kind severity ms_ssim epe pck5 ause_epe"
    assert scored[1] == "0 gaussian_noise 5 0.600000 1.500000 0.750000 0.250000" and scored[2] == "1 shot_noise 5 0.605000 - - -"
    assert [r.rsplit(" ", 3)[0] for r in scored] == plain.splitlines()                       # the rest is the old table
    R.run_sampling("dvd", "val_TDiff", 3, "exp", severity=3, corruption_number=10, keyed_noise=True, gt_map_dir=str(tmp_path))
    assert table.read_text().splitlines()[0] == "no kind severity ms_ssim map_dev epe pck5 ause_epe"
    with pytest.raises(TypeError):
        R.run_sampling("dvd", "val_TDiff", 3, "exp", True, False, None, None, False, "", str(tmp_path))
