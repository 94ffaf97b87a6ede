"""Aligned distortion without a GPU (definition: DESIGN.md 4.8; kernels: tests/test_gpu_adist.py).  The integer model
(tests/adist_model.py on tests/sflow_model.py) is held to the properties the metric must have - a global shift or scaling that
LD counts in full all but vanishes from AD, a local displacement that no global map explains stays, identical planes give zero,
a flat scan falls back to the plain mean; its pieces are held to hand-made cases; the CPU restatement of the kernels' arithmetic
(dvd_amd/csrc/adist_host_check.cpp on adist_core.h + sflow_core.h), built under ASan/UBSan, is held to the model byte for byte
and bit for bit, and must end with a status, never a sanitizer report, on refused shapes; the argument checks and the env.gt_ad
setting need no GPU either."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import adist_model as A
import sflow_model as M
from host_check import build_host_check
from dvd_amd import lib, ops

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SMALL = dict(levels=2, w_top=3, w=2, iters_top=12, iters=6)
SHIFTS = {(37, 53): (2, -1), (48, 64): (-3, 2), (40, 44): (1, 3)}
EXPORTS = ("dvd_ad_fit", "dvd_ad_align", "dvd_ad_weighted", "dvd_adist_workspace_bytes", "dvd_adist")


def last_error():
    return lib.raw().dvd_last_error().decode()


def _local(a):
    """rows 16..31 of B displaced by two pixels, the rest of B = A"""
    b = a.copy()
    b[16:32] = M.shifted(a, 2, 0)[16:32]
    return b


@pytest.fixture(scope="module")
def cases():
    """name -> (A, B, the model's result): computed once, shared and left unchanged"""
    out = {}
    for (h, w), (su, sv) in SHIFTS.items():
        a = M.page(h, w, h + w)
        out[f"shift{h}x{w}"] = (a, M.shifted(a, su, sv))
    a = M.page(48, 64, 112)
    out["scale"] = (a, A.scaled(a, 1.08, 0.94))
    out["scale+shift"] = (a, A.scaled(a, 1.06, 1.06, 2, -1))
    out["local"] = (a, _local(a))
    out["same"] = (a, a)
    out["flat"] = (np.full((48, 64), 131), a)
    return {k: (a, b, A.aligned_distortion(a, b, **SMALL)) for k, (a, b) in out.items()}


# ---- 1. the model's own properties --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [f"shift{h}x{w}" for h, w in SHIFTS] + ["scale", "scale+shift"])
def test_model_global_maps_leave_ad(cases, name):
    """Measured with this model (LD / AD): shifts 2.1904 / 0, 3.5240 / 0, 3.0476 / 0.0054; scale 1.08 x 0.94 1.4413 / 0.00037;
    scale 1.06 then shift (2, -1) 2.2275 / 0.1178."""
    r = cases[name][2]
    print(f"{name}: LD {r['ld']:.6f} AD {r['ad']:.6f} coef/65536 {(r['coef'] / 65536).round(4).tolist()}")
    assert r["ld"] > 1.0 and 0.0 <= r["ad"] < r["ld"] / 4


def test_model_keeps_a_local_distortion(cases):
    """Measured: LD 0.6250, AD 0.9078 - the displaced band holds more gradient than the mean, and no global map removes it."""
    r = cases["local"][2]
    print(f"local: LD {r['ld']:.6f} AD {r['ad']:.6f}")
    assert r["ld"] > 0.5 and r["ad"] >= r["ld"] / 2


@pytest.mark.parametrize("size", list(SHIFTS))
def test_model_fit_recovers_the_shift(cases, size):
    su, sv = SHIFTS[size]
    ax, bx, ay, by = cases["shift%dx%d" % size][2]["coef"] / 65536.0
    print(f"{size} shift {(su, sv)}: a = ({ax:.4f}, {ay:.4f}), b = ({bx:.5f}, {by:.5f})")
    assert abs(ax - su) < 0.2 and abs(ay - sv) < 0.2 and abs(bx) < 0.03 and abs(by) < 0.03


def test_model_identical_planes_and_flat_scan(cases):
    a, _, r = cases["same"]
    assert not r["coef"].any() and not r["sums"].any() and np.array_equal(r["aligned"], a) and r["ad"] == 0.0 and r["ld"] == 0.0
    flat, _, r = cases["flat"]
    print(f"flat scan: AD {r['ad']!r}, pass 2's LD {r['ld2']!r}")
    assert not A.weights(flat).any() and r["flow2"].any()
    assert r["ad"] == r["ld2"] == M.ld_sum(r["flow2"])                  # the fallback, bit for bit


# ---- 2. pieces ----------------------------------------------------------------------------------------------------------------
def _flow(fu, fv):
    return np.stack([np.asarray(fu), np.asarray(fv)]).astype(np.int16)


def wide_strip():
    """2 x 8192, f_u = 630 sign(X): Sxu = 2 * 630 * 8192^2 / 2 leaves 32 bits"""
    X = 2 * np.arange(8192) - 8191
    return _flow(np.broadcast_to(630 * np.sign(X), (2, 8192)), np.zeros((2, 8192)))


def test_fit_pieces():
    h, w = 9, 14
    sums, coef = A.fit(_flow(np.full((h, w), 3), np.full((h, w), -2)))
    assert sums.tolist() == [3 * h * w, 0, -2 * h * w, 0] and coef.tolist() == [3 * 65536, 0, -2 * 65536, 0]
    X, Y = 2 * np.arange(w) - (w - 1), 2 * np.arange(h) - (h - 1)
    sums, coef = A.fit(_flow(np.broadcast_to(X, (h, w)), np.broadcast_to(-3 * Y[:, None], (h, w))))       # f_u = X/2 * 2, f_v = Y/2 * -6
    assert coef.tolist() == [0, 2 * 65536, 0, -6 * 65536] and sums[1] == h * w * (w * w - 1) // 3
    sums, coef = A.fit(wide_strip())
    assert sums.tolist() == [0, 2 * 630 * 8192 * 8192 // 2, 0, 0] and sums[1] > 1 << 32 and sums.dtype == np.int64
    assert coef.tolist() == [0, int(np.rint(2 * sums[1] / (2 * 8192 * (8192 ** 2 - 1) // 3) * 65536)), 0, 0] and coef[1] == 15120
    rng = np.random.default_rng(1)
    for shape in ((1, 7), (7, 1)):                                          # a one-pixel axis: Sxx or Syy = 0
        f = rng.integers(-94, 95, (2,) + shape)
        sums, coef = A.fit(f)
        k = 3 if shape[0] == 1 else 1
        assert coef[k] == 0 and sums[k] == 0 and coef[4 - k] != 0 and coef.dtype == np.int32
    _, coef = A.fit(_flow([[-32767, 32767]], [[0, 0]]))                      # bx = 65534 in Q16 leaves int32: saturated
    assert coef.tolist() == [0, (1 << 31) - 1, 0, 0]


def test_align_pieces():
    b = M.page(13, 12, 1)
    assert np.array_equal(A.align(b, [0, 0, 0, 0]), b)
    got = A.align(b, [32768, 0, -32768, 0])                                  # half a pixel right, half a pixel up
    ys, xs = np.clip(np.arange(13) - 1, 0, 12), np.clip(np.arange(12) + 1, 0, 11)
    up, here = b[ys], b
    want = (up[:, np.arange(12)] + up[:, xs] + here[:, np.arange(12)] + here[:, xs]) * 16384
    want[0] = (b[0][np.arange(12)] + b[0][xs]) * 32768                       # row 0 clamps to cy = 0: no vertical fraction
    want[:, 11] = np.where(np.arange(13) == 0, b[0, 11] * 65536, (up[:, 11] + here[:, 11]) * 32768)      # column 11 clamps
    assert np.array_equal(got, (want + 32768) >> 16)
    assert np.array_equal(A.align(b, [1 << 30, 0, -(1 << 30), 0]), np.full((13, 12), b[0, 11]))      # everything clamps
    assert np.array_equal(A.align(b, [-(1 << 30), 0, 1 << 30, 0]), np.full((13, 12), b[12, 0]))
    wide = A.align(b, [0, 65536, 0, -65536 // 2])                            # q_x = x + X/2: columns spread, rows squeezed
    assert wide.min() >= 0 and wide.max() <= 255 and np.array_equal(wide[:, 0], wide[:, 1])
    g = A.weights(np.broadcast_to(((np.arange(23) // 2) % 2) * 255, (20, 23)))
    assert g[:, 1:-1].min() == 255 and A.weights(np.array([[0, 255], [255, 0]])).max() == 360


def test_ad_sum_against_a_plain_sum():
    rng = np.random.default_rng(2)
    for shape in ((37, 53), (300, 300)):
        g = rng.integers(0, 361, shape)
        f = rng.integers(-94, 95, (2,) + shape)
        plain = float((g * np.hypot(f[0], f[1])).sum() / g.sum())
        assert abs(A.ad_sum(g, f) - plain) <= 1e-12 * plain
        assert A.ad_sum(np.zeros(shape, np.int64), f) == M.ld_sum(f)
    assert A.ad_sum(np.full((3, 5), 7), _flow(np.full((3, 5), 3), np.full((3, 5), -4))) == 5.0


# ---- 3. the CPU restatement of the kernels' arithmetic, under AddressSanitizer and UBSan --------------------------------------
@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    return build_host_check("adist", tmp_path_factory.mktemp("adist_host"))


def _run(exe, tmp_path, payload, *mode):
    """(status, the output file's bytes); a sanitizer report ends the program with another exit status and fails here"""
    (tmp_path / "in.bin").write_bytes(payload)
    r = subprocess.run([str(exe), *mode, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    status = int(r.stdout.split()[0])
    return status, ((tmp_path / "out.bin").read_bytes() if status == 0 else None)


def _host_chain(exe, a, b, tmp_path, **kw):
    p = M.params(**kw)
    h, w = a.shape
    head = np.array([h, w] + [p[k] for k in M.FIELDS], np.int32)
    status, raw = _run(exe, tmp_path, head.tobytes() + a.astype(np.uint8).tobytes() + b.astype(np.uint8).tobytes())
    if status:
        return status, None
    nf = 2 * h * w * 2
    assert len(raw) == nf + 32 + 16 + h * w + nf + 24
    at = [0, nf, nf + 32, nf + 48, nf + 48 + h * w, 2 * nf + 48 + h * w]
    ld, ld2, ad = np.frombuffer(raw, np.float64, 3, at[5])
    return 0, dict(flow1=np.frombuffer(raw, np.int16, 2 * h * w, at[0]).reshape(2, h, w), sums=np.frombuffer(raw, np.int64, 4, at[1]),
                   coef=np.frombuffer(raw, np.int32, 4, at[2]), aligned=np.frombuffer(raw, np.uint8, h * w, at[3]).reshape(h, w),
                   flow2=np.frombuffer(raw, np.int16, 2 * h * w, at[4]).reshape(2, h, w), ld=float(ld), ld2=float(ld2), ad=float(ad))


def test_host_restatement_equals_the_model_under_sanitizers(host_check, tmp_path, cases):
    for name in ("shift37x53", "shift40x44", "scale+shift", "local", "same", "flat"):
        a, b, want = cases[name]
        status, got = _host_chain(host_check, a, b, tmp_path, **SMALL)
        assert status == 0
        for key in ("flow1", "sums", "coef", "aligned", "flow2"):
            assert np.array_equal(got[key], want[key]), (name, key)
        assert (got["ld"], got["ld2"], got["ad"]) == (want["ld"], want["ld2"], want["ad"]), name      # the same additions in the same order


def test_host_restatement_stages_equal_the_model(host_check, tmp_path):
    rng = np.random.default_rng(3)
    flows = [rng.integers(-94, 95, (2, 37, 53)), rng.integers(-94, 95, (2, 1, 7)), rng.integers(-94, 95, (2, 7, 1)), wide_strip(),
             _flow([[-32767, 32767]], [[0, 0]]), _flow(np.full((3, 4), -32768), np.full((3, 4), -32768))]
    for f in flows:
        _, h, w = f.shape
        status, raw = _run(host_check, tmp_path, np.array([h, w], np.int32).tobytes() + f.astype(np.int16).tobytes(), "fit")
        sums, coef = A.fit(f)
        assert status == 0 and np.array_equal(np.frombuffer(raw, np.int64, 4), sums) and np.array_equal(np.frombuffer(raw, np.int32, 4, 32), coef), (h, w)
    for h, w in ((13, 12), (37, 53), (1, 9)):
        b = M.page(h, w, 5) if h > 12 else rng.integers(0, 256, (h, w))
        for coef in ALIGN_COEFS:
            status, raw = _run(host_check, tmp_path, np.array([h, w] + list(coef), np.int32).tobytes() + b.astype(np.uint8).tobytes(), "align")
            assert status == 0 and np.array_equal(np.frombuffer(raw, np.uint8).reshape(h, w), A.align(b, coef)), (h, w, coef)


ALIGN_COEFS = ((0, 0, 0, 0), (32768, 0, -32768, 0), (-70000, -5000, 12345, -3000), (4321, 6000, -99999, 2500),
               (1 << 30, 0, -(1 << 30), 0), (-(1 << 31) + 1, (1 << 31) - 1, (1 << 31) - 1, -(1 << 31) + 1))


def test_host_restatement_refuses_bad_shapes_with_a_status(host_check, tmp_path):
    a = M.page(22, 30, 2)
    for kw in (dict(levels=2), dict(levels=0), dict(levels=7), dict(levels=1, w_top=11), dict(levels=1, d=32768), dict(levels=1, eps=0)):
        assert _host_chain(host_check, a, a, tmp_path, **kw)[0] == -1, kw          # levels=2: a top level of 11 x 15
    assert _host_chain(host_check, a[:11], a[:11], tmp_path, levels=1)[0] == -1
    assert _host_chain(host_check, a, a, tmp_path, levels=1, w_top=1, iters_top=1)[0] == 0
    for h, w in ((0, 5), (5, 0), (8193, 1), (-1, 4)):
        assert _run(host_check, tmp_path, np.array([h, w], np.int32).tobytes(), "fit")[0] == -1
        assert _run(host_check, tmp_path, np.array([h, w, 0, 0, 0, 0], np.int32).tobytes(), "align")[0] == -1


# ---- 4. argument checks and the setting ---------------------------------------------------------------------------------------
def test_exports_are_bound():
    for name in EXPORTS:
        assert name in lib.SIGNATURES and hasattr(lib.raw(), name)
    assert "dvd_adist_workspace_bytes" in lib.NON_STATUS and lib.RESTYPES["dvd_adist_workspace_bytes"] is C.c_long


def test_workspace_formula():
    raw = lib.raw()
    pr = ops.sflow_params()
    got, chain = raw.dvd_adist_workspace_bytes(920, 650, C.byref(pr)), raw.dvd_sflow_workspace_bytes(920, 650, C.byref(pr))
    hw, blocks = 920 * 650, -(-920 * 650 // 256)
    want = chain + 4 * hw + 2 * 4 * hw + 32 * blocks + 32 + 16 + 8            # ONE chain workspace, B', two flows, the partials
    assert want <= got <= want + 256 * 8, (got, want)
    assert raw.dvd_adist_workspace_bytes(88, 650, C.byref(pr)) == -1 and "top level below 12" in last_error()
    assert raw.dvd_adist_workspace_bytes(920, 650, None) == -1 and "null" in last_error()


def test_library_refuses_bad_arguments_before_any_launch():
    """Device pointers that are never dereferenced: nothing is launched."""
    raw = lib.raw()
    fake, odd = C.c_void_p(1 << 20), C.c_void_p((1 << 20) + 2)
    good = ops.sflow_params()
    none7 = [None] * 5

    def adist(a=fake, b=fake, n=1, h=920, w=650, pr=good, work=fake, ld=fake, ad=fake, extra=none7):
        return raw.dvd_adist(a, b, n, h, w, C.byref(pr) if pr is not None else None, work, ld, ad, *extra, None)

    for kw in (dict(a=None), dict(b=None), dict(pr=None), dict(work=None), dict(ld=None), dict(ad=None)):
        assert adist(**kw) == -1 and "adist: null" in last_error(), kw
    for n in (0, -1, 65536):
        assert adist(n=n) == -1 and "batch" in last_error()
    assert adist(h=80) == -1 and "below 12" in last_error()
    assert adist(w=8193) == -1 and "8192" in last_error()
    assert adist(h=0) == -1
    assert adist(work=C.c_void_p((1 << 20) + 64)) == -1 and "256-byte aligned" in last_error()
    assert adist(ad=odd) == -1 and "misaligned" in last_error()
    assert adist(extra=[None, odd, None, None, None]) == -1 and "misaligned" in last_error()
    for kw, word in ((dict(levels=0), "levels"), (dict(w_top=11), "window"), (dict(d=32768), "16-bit"), (dict(eps=0), "eps"),
                     (dict(iters_top=0), "iterations")):
        bad = lib.SflowParams(**dict(M.DEFAULTS, **kw))
        assert adist(pr=bad) == -1 and word in last_error(), kw
        assert raw.dvd_adist_workspace_bytes(920, 650, C.byref(bad)) == -1 and word in last_error(), kw
    assert raw.dvd_ad_fit(None, 1, 37, 53, fake, fake, fake, None) == -1 and "ad_fit: null" in last_error()
    assert raw.dvd_ad_fit(fake, 1, 37, 53, None, fake, fake, None) == -1 and "null" in last_error()
    assert raw.dvd_ad_fit(fake, 0, 37, 53, fake, fake, fake, None) == -1 and "batch" in last_error()
    assert raw.dvd_ad_fit(fake, 1, 0, 53, fake, fake, fake, None) == -1 and "shape" in last_error()
    assert raw.dvd_ad_fit(fake, 1, 37, 8193, fake, fake, fake, None) == -1 and "8192" in last_error()
    assert raw.dvd_ad_fit(fake, 1, 37, 53, odd, fake, fake, None) == -1 and "misaligned" in last_error()
    assert raw.dvd_ad_align(fake, None, 1, 37, 53, fake, None) == -1 and "ad_align: null" in last_error()
    assert raw.dvd_ad_align(fake, fake, 1, 37, 0, fake, None) == -1 and "shape" in last_error()
    assert raw.dvd_ad_align(fake, fake, 65536, 37, 53, fake, None) == -1 and "batch" in last_error()
    assert raw.dvd_ad_align(fake, odd, 1, 37, 53, C.c_void_p(1 << 21), None) == -1 and "misaligned" in last_error()
    assert raw.dvd_ad_align(fake, fake, 1, 37, 53, fake, None) == -1 and "must not be b" in last_error()
    assert raw.dvd_ad_weighted(fake, fake, 1, 37, 53, fake, None, None) == -1 and "ad_weighted: null" in last_error()
    assert raw.dvd_ad_weighted(fake, fake, 1, 8193, 53, fake, fake, None) == -1 and "8192" in last_error()
    assert raw.dvd_ad_weighted(fake, fake, 0, 37, 53, fake, fake, None) == -1 and "batch" in last_error()
    assert raw.dvd_ad_weighted(fake, fake, 1, 37, 53, odd, fake, None) == -1 and "misaligned" in last_error()


def test_ops_argument_checks_need_no_gpu():
    x = torch.zeros(1, 96, 96)
    u8 = torch.zeros(200, 200, 3, dtype=torch.uint8)
    for kw in (dict(levels=0), dict(w_top=11), dict(d=32768), dict(T=65400), dict(eps=0), dict(iters=0), dict(levels=2.0), dict(window=3)):
        with pytest.raises(ValueError, match="aligned_distortion"):
            ops.aligned_distortion(x, x, **kw)
        with pytest.raises(ValueError, match="ad_u8"):
            ops.ad_u8(u8, u8, **kw)
    with pytest.raises(ValueError, match="top level"):
        ops.aligned_distortion(torch.zeros(1, 88, 96), torch.zeros(1, 88, 96))
    with pytest.raises(ValueError, match="one shape"):
        ops.aligned_distortion(x, torch.zeros(1, 96, 97))
    with pytest.raises(ValueError, match="one shape"):
        ops.aligned_distortion(x[0], x[0])
    with pytest.raises(ValueError, match="top level"):
        ops.ad_u8(torch.zeros(300, 420, 3, dtype=torch.uint8), torch.zeros(352, 250, 3, dtype=torch.uint8), area=80 * 90)
    with pytest.raises(ValueError, match=r"expected \[H,W,3\]"):
        ops.ad_u8(torch.zeros(300, 420, dtype=torch.uint8), u8)
    with pytest.raises(ValueError, match="area"):
        ops.ad_u8(u8, u8, area=0)
    for metrics in (("psnr",), ("ms_ssim", "ad", "psnr"), ()):
        with pytest.raises(ValueError, match="metrics"):
            ops.gt_metrics_u8(u8, u8, metrics)
    with pytest.raises(ValueError, match="top level"):                        # 'ad' alone needs the chain's working size too
        ops.gt_metrics_u8(torch.zeros(300, 420, 3, dtype=torch.uint8), torch.zeros(352, 250, 3, dtype=torch.uint8), ("ad",), area=80 * 90)
    f = torch.zeros(1, 2, 37, 53, dtype=torch.int16)
    for bad in (f[0], f.int(), torch.zeros(1, 3, 37, 53, dtype=torch.int16), torch.zeros(0, 2, 37, 53, dtype=torch.int16),
                torch.zeros(1, 2, 0, 53, dtype=torch.int16)):
        with pytest.raises(ValueError, match="ad_fit"):
            ops.ad_fit(bad)
    p = torch.zeros(2, 37, 53)
    c = torch.zeros(2, 4, dtype=torch.int32)
    for b_, c_ in ((p[0], c), (p.double(), c), (p, c[:1]), (p, c.long()), (p, torch.zeros(2, 3, dtype=torch.int32))):
        with pytest.raises(ValueError, match="ad_align"):
            ops.ad_align(b_, c_)
    for a_, f_ in ((p[0], f), (p, f), (p[:1], f.int()), (p[:1].half(), f), (p[:1], f[:, :, :36])):
        with pytest.raises(ValueError, match="ad_weighted"):
            ops.ad_weighted(a_, f_)
    for call in (lambda: ops.ad_fit(f), lambda: ops.ad_align(p, c), lambda: ops.ad_weighted(p[:1], f), lambda: ops.aligned_distortion(x, x)):
        with pytest.raises(lib.DvdError, match="device tensor"):              # good arguments on the host: there is no CPU path
            call()
