"""Local distortion without a GPU (definition: DESIGN.md 4.7; kernels: tests/test_gpu_sflow.py).  The integer model
(tests/sflow_model.py) is held to its own properties - the separable min-convolution equals the brute-force one, identical
planes give a zero field, pure shifts are recovered away from the border, messages and costs stay in 16 bits; the CPU
restatement of the kernels' arithmetic (dvd_amd/csrc/sflow_host_check.cpp on sflow_core.h), built under ASan/UBSan, is held to
the model byte for byte - descriptors, the top level's cost volume, the flow and LD - and must end with a status, never a
sanitizer report, on refused shapes; the argument checks and the env.gt_metrics setting need no GPU either."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import sflow_model as M
from host_check import build_host_check
from dvd_amd import lib, ops

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SMALL = dict(levels=2, w_top=3, w=2, iters_top=12, iters=6)
SHIFTS = {(37, 53): (2, -1), (48, 64): (-3, 2), (40, 44): (1, 3)}
EXPORTS = ("dvd_dsift_u8", "dvd_sflow_cost", "dvd_sflow_level_workspace_bytes", "dvd_sflow_level", "dvd_sflow_workspace_bytes",
           "dvd_sflow")


def last_error():
    return lib.raw().dvd_last_error().decode()


@pytest.fixture(scope="module")
def shift_cases():
    """(h, w) -> (A, B, the model's flow, the model's LD): computed once, shared and left unchanged"""
    out = {}
    for (h, w), (su, sv) in SHIFTS.items():
        a = M.page(h, w, h + w)
        b = M.shifted(a, su, sv)
        flow, ld = M.sift_flow(a, b, **SMALL)
        out[(h, w)] = (a, b, flow, ld)
    return out


# ---- 1. separable equals brute force ------------------------------------------------------------------------------------------
def test_separable_min_convolution_equals_brute_force():
    rng = np.random.default_rng(0)
    a = M.page(24, 30, 3)
    b = M.shifted(a, 1, -1)
    da, db = M.dsift(a), M.dsift(b)
    off = (rng.integers(-2, 3, (24, 30)), rng.integers(-2, 3, (24, 30)))
    p = M.params()
    fast = M.level(da, db, off, 2, 4, p)
    assert fast.shape == (2, 24, 30) and np.array_equal(fast, M.level_brute(da, db, off, 2, 4, p))


# ---- 2. the model's own properties (the 16-bit bounds are asserted inside the model on every call) ----------------------------
@pytest.mark.parametrize("size", list(SHIFTS))
def test_model_recovers_a_pure_shift(shift_cases, size):
    su, sv = SHIFTS[size]
    _, _, flow, ld = shift_cases[size]
    ok = (flow[0] == su) & (flow[1] == sv)
    print(f"{size} shift {(su, sv)}: exact at {ok.mean():.3f} of all pixels, LD {ld:.4f}")
    assert flow.dtype == np.int16 and ok[8:-8, 8:-8].all()
    assert abs(ld - float(np.hypot(su, sv))) < 0.35 * float(np.hypot(su, sv))       # a border band of mismatches, no more


@pytest.mark.parametrize("size", list(SHIFTS))
def test_model_gives_zero_on_identical_planes(shift_cases, size):
    a = shift_cases[size][0]
    flow, ld = M.sift_flow(a, a, **SMALL)
    assert not flow.any() and ld == 0.0


def test_model_pieces():
    img = M.page(13, 12, 1)
    d = M.dsift(img)
    assert d.shape == (13, 12, 128) and d.dtype == np.uint8 and d.max() > 0
    assert not M.dsift(np.full((14, 15), 77)).any()                              # no gradient: eps alone divides
    assert M.reduce2(np.full((7, 9), 200)).shape == (4, 5) and (M.reduce2(np.full((7, 9), 200)) == 200).all()
    s = np.array([0, 1, 3, 4, 8, 15, 16, (1 << 52) - 1, 1 << 52, 94906265 ** 2 - 1, 94906265 ** 2], np.int64)
    assert M.isqrt(s).tolist() == [0, 1, 1, 2, 2, 3, 4, 67108863, 67108864, 94906264, 94906265]
    assert M.ld_sum(np.stack([np.full((3, 5), 3), np.full((3, 5), -4)])) == 5.0
    lu, lv = M.labels(2)
    assert (lu[7], lv[7]) == (0, -1) and lu.size == 25


# ---- 3. the CPU restatement of the kernels' arithmetic, under AddressSanitizer and UBSan --------------------------------------
@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    return build_host_check("sflow", tmp_path_factory.mktemp("sflow_host"))


def _host_run(exe, a, b, tmp_path, **kw):
    """(status, descriptors of A, the top level's cost volume, flow, LD); a sanitizer report ends the program with another exit
    status and fails here"""
    p = M.params(**kw)
    h, w = a.shape
    head = np.array([h, w] + [p[k] for k in M.FIELDS], np.int32)
    (tmp_path / "in.bin").write_bytes(head.tobytes() + a.astype(np.uint8).tobytes() + b.astype(np.uint8).tobytes())
    r = subprocess.run([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    status, ht, wt, lt = (int(v) for v in r.stdout.split())
    if status:
        return status, None, None, None, None
    raw = (tmp_path / "out.bin").read_bytes()
    n0, n1, n2 = h * w * 128, ht * wt * lt * 2, 2 * h * w * 2
    assert len(raw) == n0 + n1 + n2 + 8
    return (0, np.frombuffer(raw, np.uint8, n0).reshape(h, w, 128), np.frombuffer(raw, np.uint16, ht * wt * lt, n0).reshape(ht, wt, lt),
            np.frombuffer(raw, np.int16, 2 * h * w, n0 + n1).reshape(2, h, w), float(np.frombuffer(raw, np.float64, 1, n0 + n1 + n2)[0]))


def _top_cost(a, b, **kw):
    p = M.params(**kw)
    ta, tb = M.pyramid(a, p["levels"])[-1], M.pyramid(b, p["levels"])[-1]
    zero = np.zeros(ta.shape, np.int64)
    return M.cost_volume(M.dsift(ta, p["eps"]), M.dsift(tb, p["eps"]), (zero, zero), p["w_top"], p["gamma"], p["T"])


def test_host_restatement_equals_the_model_under_sanitizers(host_check, tmp_path, shift_cases):
    cases = [(a, b, SMALL, flow, ld) for a, b, flow, ld in shift_cases.values()]
    odd = dict(levels=3, w_top=2, w=1, iters_top=5, iters=3)                   # 50 x 70 -> 25 x 35 -> 13 x 18: odd through ceil
    a = M.page(50, 70, 9)
    b = M.shifted(a, -2, 1)
    cases.append((a, b, odd) + M.sift_flow(a, b, **odd))
    flat = np.full((24, 26), 131)                                               # every descriptor 0, every label ties
    one = dict(levels=1, w_top=10, w=2, iters_top=2, iters=1)                   # the 21 x 21 label grid
    cases.append((flat, M.page(24, 26, 4), one) + M.sift_flow(flat, M.page(24, 26, 4), **one))
    for a, b, kw, want_flow, want_ld in cases:
        status, desc, cost, flow, ld = _host_run(host_check, a, b, tmp_path, **kw)
        assert status == 0
        assert np.array_equal(desc, M.dsift(a)), a.shape
        assert np.array_equal(cost, _top_cost(a, b, **kw)), a.shape
        assert np.array_equal(flow, want_flow), a.shape
        assert ld == want_ld, (a.shape, ld, want_ld)                           # the same additions in the same order


def test_host_restatement_refuses_bad_shapes_with_a_status(host_check, tmp_path):
    a = M.page(22, 30, 2)
    for kw in (dict(levels=2), dict(levels=0), dict(levels=7), dict(levels=1, w_top=11), dict(levels=1, w=0), dict(levels=1, d=32768),
               dict(levels=1, T=65535), dict(levels=1, eps=0), dict(levels=1, iters=0), dict(levels=1, alpha=-1)):
        assert _host_run(host_check, a, a, tmp_path, **kw)[0] == -1, kw          # levels=2: a top level of 11 x 15
    assert _host_run(host_check, a[:11], a[:11], tmp_path, levels=1)[0] == -1
    assert _host_run(host_check, a, a, tmp_path, levels=1, w_top=1, iters_top=1)[0] == 0


# ---- 4. argument checks and the setting ---------------------------------------------------------------------------------------
def test_exports_are_bound():
    for name in EXPORTS:
        assert name in lib.SIGNATURES and hasattr(lib.raw(), name)
    for name in ("dvd_sflow_level_workspace_bytes", "dvd_sflow_workspace_bytes"):
        assert name in lib.NON_STATUS and lib.RESTYPES[name] is C.c_long
    assert [f for f, _ in lib.SflowParams._fields_] == list(M.FIELDS) and C.sizeof(lib.SflowParams) == 40
    assert lib.SFLOW_DEFAULTS == M.DEFAULTS == ops.SFLOW_DEFAULTS
    text = open(os.path.join(ROOT, "include", "dvd_hip.h")).read()
    assert "#define DVD_SFLOW_MIN_TOP 12" in text and lib.SFLOW_MIN_TOP == 12


def test_workspace_formula():
    raw = lib.raw()
    pr = ops.sflow_params()
    got = raw.dvd_sflow_workspace_bytes(920, 650, C.byref(pr))
    dims = [(920, 650), (460, 325), (230, 163), (115, 82)]
    planes = 2 * sum(h * w for h, w in dims)
    level = max(18 * h * w * (441 if k == 3 else 25) + 8 * -(-h * w // 256) for k, (h, w) in enumerate(dims))
    want = planes + 2 * 128 * 920 * 650 + 3 * 4 * 920 * 650 + level
    assert want <= got <= want + 256 * 20 and 0.40e9 < got < 0.45e9, (got, want)       # each piece rounded up to 256 bytes
    assert raw.dvd_sflow_level_workspace_bytes(37, 53, 2) >= 18 * 37 * 53 * 25
    assert raw.dvd_sflow_level_workspace_bytes(37, 53, 11) == -1 and "sflow_level_workspace_bytes" in last_error()
    assert raw.dvd_sflow_level_workspace_bytes(0, 53, 2) == -1


def test_library_refuses_bad_arguments_before_any_launch():
    """Device pointers that are never dereferenced: nothing is launched."""
    raw = lib.raw()
    fake = C.c_void_p(1 << 20)
    good = ops.sflow_params()

    def changed(**kw):
        return lib.SflowParams(**dict(M.DEFAULTS, **kw))

    assert raw.dvd_sflow_workspace_bytes(89, 89, C.byref(good)) > 0                  # 89, 45, 23, 12
    assert raw.dvd_sflow_workspace_bytes(88, 650, C.byref(good)) == -1 and "top level below 12" in last_error()
    assert raw.dvd_sflow_workspace_bytes(8193, 650, C.byref(good)) == -1 and "8192" in last_error()
    assert raw.dvd_sflow_workspace_bytes(920, 650, None) == -1 and "null" in last_error()
    for kw, word in ((dict(levels=0), "levels"), (dict(levels=7), "levels"), (dict(w_top=11), "window"), (dict(w=0), "window"),
                     (dict(d=32768), "16-bit"), (dict(T=65400), "16-bit"), (dict(gamma=400), "16-bit"), (dict(eps=0), "eps"),
                     (dict(iters_top=0), "iterations"), (dict(alpha=65536), "alpha")):
        bad = changed(**kw)
        assert raw.dvd_sflow_workspace_bytes(920, 650, C.byref(bad)) == -1 and word in last_error(), kw
        assert raw.dvd_sflow(fake, fake, 1, 920, 650, C.byref(bad), fake, fake, fake, None) == -1 and word in last_error(), kw
        assert raw.dvd_sflow_cost(fake, fake, fake, 37, 53, 2, C.byref(bad), fake, None) == -1 and word in last_error(), kw
        assert raw.dvd_sflow_level(fake, fake, fake, 37, 53, 2, 3, C.byref(bad), fake, fake, None, None) == -1, kw
    assert raw.dvd_sflow(None, fake, 1, 920, 650, C.byref(good), fake, fake, fake, None) == -1 and "null" in last_error()
    assert raw.dvd_sflow(fake, fake, 0, 920, 650, C.byref(good), fake, fake, fake, None) == -1 and "batch" in last_error()
    assert raw.dvd_sflow(fake, fake, 1, 80, 650, C.byref(good), fake, fake, fake, None) == -1 and "below 12" in last_error()
    assert raw.dvd_sflow(fake, fake, 1, 920, 650, C.byref(good), C.c_void_p((1 << 20) + 64), fake, fake, None) == -1 and "aligned" in last_error()
    assert raw.dvd_dsift_u8(None, 1, 13, 12, 1 << 17, fake, None) == -1 and "null" in last_error()
    assert raw.dvd_dsift_u8(fake, 1, 0, 12, 1 << 17, fake, None) == -1 and "shape" in last_error()
    assert raw.dvd_dsift_u8(fake, 1, 13, 12, 0, fake, None) == -1 and "eps" in last_error()
    assert raw.dvd_dsift_u8(fake, 1, 13, 12, 1 << 17, C.c_void_p((1 << 20) + 8), None) == -1 and "aligned" in last_error()
    assert raw.dvd_sflow_cost(fake, fake, fake, 37, 53, 11, C.byref(good), fake, None) == -1 and "window" in last_error()
    assert raw.dvd_sflow_level(fake, fake, fake, 37, 53, 2, 0, C.byref(good), fake, fake, None, None) == -1 and "iterations" in last_error()


def test_ops_argument_checks_need_no_gpu():
    x = torch.zeros(1, 96, 96)
    for kw in (dict(levels=0), dict(levels=7), dict(w_top=11), dict(w=0), dict(d=32768), dict(T=65400), dict(eps=0), dict(iters=0),
               dict(alpha=-1), dict(levels=2.0), dict(w=True), dict(window=3)):
        with pytest.raises(ValueError, match="sift_flow"):
            ops.sift_flow(x, x, **kw)
        with pytest.raises(ValueError, match="ld_u8"):
            ops.ld_u8(torch.zeros(200, 200, 3, dtype=torch.uint8), torch.zeros(200, 200, 3, dtype=torch.uint8), **kw)
    with pytest.raises(ValueError, match="top level"):
        ops.sift_flow(torch.zeros(1, 88, 96), torch.zeros(1, 88, 96))
    with pytest.raises(ValueError, match="one shape"):
        ops.sift_flow(x, torch.zeros(1, 96, 97))
    with pytest.raises(ValueError, match="one shape"):
        ops.local_distortion(x[0], x[0])
    with pytest.raises(ValueError, match="top level"):
        ops.ld_u8(torch.zeros(300, 420, 3, dtype=torch.uint8), torch.zeros(352, 250, 3, dtype=torch.uint8), area=80 * 90)
    with pytest.raises(ValueError, match=r"expected \[H,W,3\]"):
        ops.ld_u8(torch.zeros(300, 420, dtype=torch.uint8), torch.zeros(352, 250, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="area"):
        ops.ld_u8(torch.zeros(300, 420, 3, dtype=torch.uint8), torch.zeros(352, 250, 3, dtype=torch.uint8), area=0)
    with pytest.raises(ValueError, match="metrics"):
        ops.gt_metrics_u8(torch.zeros(300, 420, 3, dtype=torch.uint8), torch.zeros(352, 250, 3, dtype=torch.uint8), ("psnr",))
    with pytest.raises(ValueError, match="dense_sift_u8"):
        ops.dense_sift_u8(torch.zeros(13, 12))
    with pytest.raises(ValueError, match="eps"):
        ops.dense_sift_u8(torch.zeros(1, 13, 12), eps=0)
    d = torch.zeros(37, 53, 128, dtype=torch.uint8)
    off = torch.zeros(2, 37, 53, dtype=torch.int16)
    with pytest.raises(ValueError, match="win"):
        ops.sflow_cost(d, d, off, 11)
    with pytest.raises(ValueError, match="off"):
        ops.sflow_cost(d, d, off[:, :36], 2)
    with pytest.raises(ValueError, match="iters"):
        ops.sflow_level(d, d, off, 2, 0)
    with pytest.raises(lib.DvdError, match="device tensor"):                 # good arguments on the host: there is no CPU path
        ops.sift_flow(x, x)
    assert ops.sflow_top_size(920, 650, 4) == (115, 82) and ops.sflow_top_size(50, 70, 3) == (13, 18)
    pr = ops.sflow_params()
    assert {f: getattr(pr, f) for f in M.FIELDS} == M.DEFAULTS


def test_gt_metrics_setting():
    """parse_gt_metrics itself (the run's check of env.gt_metrics: tests/test_run_options_cpu.py)."""
    import admin.settings as ws
    from dvd_amd.evaluation import parse_gt_metrics
    assert ws.Settings().env.gt_metrics == "ms_ssim"                         # the default: what a run scored before
    assert parse_gt_metrics("ms_ssim") == ("ms_ssim",)
    assert parse_gt_metrics("ms_ssim,ld") == parse_gt_metrics("ld, ms_ssim") == ("ms_ssim", "ld")
    assert parse_gt_metrics("ld") == ("ld",)
    for bad in ("", "ssim", "ms_ssim,ad", "ld,ld", "ms_ssim;ld", None, ("ld",)):
        with pytest.raises(ValueError, match="env.gt_metrics"):
            parse_gt_metrics(bad)
