"""The aligned-distortion kernels (the AD section of dvd_amd/csrc/sflow.hip) against the integer model of tests/adist_model.py
(DESIGN.md 4.8).

Everything but LD and AD is an integer and is held to the model exactly: sums, coefficients, the resampled page and both flows
are compared with array_equal.  AD is a quotient of a float64 sum of at most 2^20 non-negative terms (each a correctly rounded
root times an integer, correctly rounded) and an exact integer; only the order of the additions can differ from the model's,
which moves the sum by at most N 2^-53 relative, so |AD - model| <= 1e-9 max(1, AD), LD's bound with LD's derivation.
Expected values come from the model at test time; the shapes are the smallest that take every path: sizes that are no multiple
of 256, one-pixel axes (a zero denominator), more partials than the finalize has lanes (300 x 300: 352), sums that leave 32
bits, coefficients that clamp every pixel, a flat scan (the fallback), a batch."""
import os

import numpy as np
import pytest
import torch

import adist_model as A
import msssim_model as MS
import sflow_model as M
from dvd_amd import synth

pytestmark = pytest.mark.gpu

SMALL = dict(levels=2, w_top=3, w=2, iters_top=12, iters=6)
BOUND = 1e-9


def _cuda(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()


def _stripes(h, w):
    """Columns in pairs of 0 and 255: g = 255 at every interior pixel"""
    return np.broadcast_to(((np.arange(w) // 2) % 2) * 255, (h, w)).copy()


def _wide_strip():
    X = 2 * np.arange(8192) - 8191
    return np.stack([np.broadcast_to(630 * np.sign(X), (2, 8192)), np.zeros((2, 8192), np.int64)])


# ---- fit ----------------------------------------------------------------------------------------------------------------------
FIT_FLOWS = {
    "37x53": lambda rng: rng.integers(-94, 95, (1, 2, 37, 53)),
    "1x7": lambda rng: rng.integers(-94, 95, (1, 2, 1, 7)),
    "7x1": lambda rng: rng.integers(-94, 95, (1, 2, 7, 1)),
    "300x300": lambda rng: rng.integers(-94, 95, (1, 2, 300, 300)),           # 352 partials: the finalize's strided loop
    "2x8192": lambda rng: _wide_strip()[None],                                # Sxu = 630 * 8192^2 > 2^32
    "batch": lambda rng: rng.integers(-94, 95, (2, 2, 37, 53)),
    "extremes": lambda rng: np.array([[[[-32767, 32767]], [[-32768, -32768]]]]),   # 1 x 2: bx saturates
}


@pytest.mark.parametrize("name", list(FIT_FLOWS))
def test_fit_equals_the_model(name):
    from dvd_amd import ops
    flows = FIT_FLOWS[name](np.random.default_rng(7))
    sums, coef = ops.ad_fit(_cuda(flows, torch.int16))
    assert sums.dtype == torch.int64 and coef.dtype == torch.int32 and sums.shape == coef.shape == (flows.shape[0], 4)
    for k, f in enumerate(flows):
        want_sums, want_coef = A.fit(f)
        assert np.array_equal(sums[k].cpu().numpy(), want_sums), (name, k)
        assert np.array_equal(coef[k].cpu().numpy(), want_coef), (name, k)
    if name == "2x8192":
        assert int(sums[0, 1]) == 630 * 8192 * 8192
    if name in ("1x7", "7x1"):
        assert int(coef[0, 3 if name == "1x7" else 1]) == 0


# ---- align --------------------------------------------------------------------------------------------------------------------
ALIGN_COEFS = {"identity": (0, 0, 0, 0), "half": (32768, 0, -32768, 0), "shrink": (-70000, -5000, 12345, -3000),
               "grow": (4321, 6000, -99999, 2500), "clamp": (1 << 30, 0, -(1 << 30), 0)}


@pytest.mark.parametrize("size", [(13, 12), (37, 53), (1, 9)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_align_equals_the_model(size):
    """all five coefficient sets as one batch of five copies of the plane"""
    from dvd_amd import ops
    h, w = size
    b = M.page(h, w, 5) if h > 12 else np.random.default_rng(8).integers(0, 256, (h, w))
    coefs = np.array(list(ALIGN_COEFS.values()), np.int32)
    got = ops.ad_align(_cuda(np.stack([b] * len(coefs))), _cuda(coefs, torch.int32))
    assert got.dtype == torch.float32 and got.shape == (len(coefs), h, w)
    for k, name in enumerate(ALIGN_COEFS):
        assert np.array_equal(got[k].cpu().numpy(), A.align(b, coefs[k])), name
    assert np.array_equal(got[0].cpu().numpy(), b)
    assert (got[4] == float(b[0, w - 1])).all()


# ---- weighted mean ------------------------------------------------------------------------------------------------------------
WEIGHT_PLANES = {"stripes": _stripes, "flat": lambda h, w: np.full((h, w), 131), "page": lambda h, w: M.page(h, w, 6)}


@pytest.mark.parametrize("size", [(37, 53), (300, 300)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", list(WEIGHT_PLANES))
def test_weighted_mean_equals_the_model(name, size):
    from dvd_amd import ops
    h, w = size
    a = WEIGHT_PLANES[name](h, w)
    f = np.random.default_rng(9).integers(-94, 95, (2, h, w))
    want = A.ad_sum(A.weights(a), f)
    got = ops.ad_weighted(_cuda(a[None]), _cuda(f[None], torch.int16))
    print(f"{name} {h}x{w}: AD {got[0]!r} against the model's {want!r}")
    assert got.shape == (1,) and got.dtype == np.float64
    assert abs(got[0] - want) <= BOUND * max(1.0, want)
    if name == "flat":
        assert abs(got[0] - M.ld_sum(f)) <= BOUND * max(1.0, want)
    if name == "stripes":
        assert A.weights(a)[:, 1:-1].min() == 255


# ---- chain --------------------------------------------------------------------------------------------------------------------
def _shift_case():
    a = M.page(37, 53, 90)
    return a, M.shifted(a, 2, -1)


def _scale_case():
    a = M.page(48, 64, 112)
    return a, A.scaled(a, 1.06, 1.06, 2, -1)


def _check_chain(ops, a, b, got_ad, got_ld, x, k, want):
    for key in ("flow1", "sums", "coef", "aligned", "flow2"):
        assert np.array_equal(x[key][k].cpu().numpy(), want[key]), key
    print(f"LD {got_ld!r} / {want['ld']!r}, AD {got_ad!r} / {want['ad']!r}")
    assert abs(got_ld - want["ld"]) <= BOUND * max(1.0, want["ld"])
    assert abs(got_ad - want["ad"]) <= BOUND * max(1.0, want["ad"])


@pytest.mark.parametrize("case", [_shift_case, _scale_case], ids=["37x53-shift", "48x64-scale+shift"])
def test_whole_chain(case):
    from dvd_amd import ops
    a, b = case()
    want = A.aligned_distortion(a, b, **SMALL)
    ad, ld, x = ops.aligned_distortion(_cuda(a[None]), _cuda(b[None]), intermediates=True, **SMALL)
    assert ad.shape == ld.shape == (1,) and ad.dtype == ld.dtype == np.float64
    assert x["flow1"].dtype == x["flow2"].dtype == torch.int16 and x["aligned"].dtype == torch.float32
    _check_chain(ops, a, b, ad[0], ld[0], x, 0, want)
    flow, ld_alone = ops.sift_flow(_cuda(a[None]), _cuda(b[None]), **SMALL)
    assert ld[0] == ld_alone[0] and torch.equal(flow, x["flow1"])              # pass 1 IS the LD chain
    ad2, ld2 = ops.aligned_distortion(_cuda(a[None]), _cuda(b[None]), **SMALL)      # without the optional outputs
    assert ad2[0] == ad[0] and ld2[0] == ld[0]
    assert want["ad"] < want["ld"] / 4


def test_batch_document_equals_itself_alone():
    from dvd_amd import ops
    a0 = M.page(40, 44, 11)
    a = np.stack([a0, M.page(40, 44, 12)])
    b = np.stack([M.shifted(a0, 1, 3), A.scaled(a[1], 1.05, 0.97, -1, 1)])
    ad, ld, x = ops.aligned_distortion(_cuda(a), _cuda(b), intermediates=True, **SMALL)
    assert ad.shape == ld.shape == (2,) and x["flow2"].shape == (2, 2, 40, 44) and x["coef"].shape == (2, 4)
    for k in range(2):
        ad1, ld1, x1 = ops.aligned_distortion(_cuda(a[k:k + 1]), _cuda(b[k:k + 1]), intermediates=True, **SMALL)
        assert ad1[0] == ad[k] and ld1[0] == ld[k], k
        for key in x:
            assert torch.equal(x1[key][0], x[key][k]), (k, key)
        _check_chain(ops, a[k], b[k], ad[k], ld[k], x, k, A.aligned_distortion(a[k], b[k], **SMALL))
    assert not torch.equal(x["coef"][0], x["coef"][1])


def test_identical_planes_and_a_flat_scan():
    from dvd_amd import ops
    a = M.page(37, 53, 90)
    ad, ld, x = ops.aligned_distortion(_cuda(a[None]), _cuda(a[None]), intermediates=True, **SMALL)
    assert ad[0] == 0.0 and ld[0] == 0.0 and not bool(x["coef"].any()) and np.array_equal(x["aligned"][0].cpu().numpy(), a)
    flat = np.full((37, 53), 131)
    want = A.aligned_distortion(flat, a, **SMALL)
    ad, ld, x = ops.aligned_distortion(_cuda(flat[None]), _cuda(a[None]), intermediates=True, **SMALL)
    assert np.array_equal(x["flow2"][0].cpu().numpy(), want["flow2"]) and want["flow2"].any()
    assert abs(ad[0] - want["ad"]) <= BOUND * max(1.0, want["ad"]) and want["ad"] == want["ld2"]
    assert ad[0] == ops.sift_flow(_cuda(flat[None]), x["aligned"], **SMALL)[1][0]      # the fallback: pass 2's LD, bit for bit


# ---- u8 images and the run ----------------------------------------------------------------------------------------------------
def _rgb(key, h, w):
    img = synth.smooth_image(key, h, w).transpose(1, 2, 0).astype(np.float64) * 255.0
    noise = (synth.uniform01(key + "/n", h * w * 3, 5).reshape(h, w, 3).astype(np.float64) - 0.5) * 60.0
    return np.clip(np.rint(img + noise), 0, 255).astype(np.uint8)


def test_ad_u8_end_to_end():
    """The benchmark's preparation, then the chain: equal to the model on the model-resized planes (the inputs hold no pixel on an
    exact half before the resize's rounding - counted from the model - so the planes are the model's, as in test_ld_u8_end_to_end).
    The two images differ in size."""
    from dvd_amd import ops
    gt = _rgb("ad/gt", 200, 260)
    noise = (synth.uniform01("ad/pred/n", 200 * 260 * 3, 3).reshape(200, 260, 3).astype(np.float64) - 0.5) * 30.0
    pred = np.clip(np.rint(np.roll(gt, (3, -4), axis=(0, 1)) + noise), 0, 255).astype(np.uint8)
    pred = np.ascontiguousarray(pred[:188, :248])                       # another size than the scan's
    gt, pred = gt & 0xF8, pred & 0xF8
    area = 60 * 78
    assert MS.target_size(200, 260, area) == (60, 78)
    assert not MS.knife_edge(pred, 60, 78).any() and not MS.knife_edge(gt, 60, 78).any()
    kw = dict(levels=2, w_top=3, w=2, iters_top=6, iters=4)
    want = A.aligned_distortion(MS.resize_gray(gt, 60, 78), MS.resize_gray(pred, 60, 78), **kw)
    p, g = _cuda(pred, torch.uint8), _cuda(gt, torch.uint8)
    got = ops.ad_u8(p, g, area, **kw)
    print(f"ad_u8: {got!r} against the model's {want['ad']!r} (LD {want['ld']!r})")
    assert isinstance(got, float) and want["flow2"].any()
    assert abs(got - want["ad"]) <= BOUND * max(1.0, want["ad"])
    assert ops.gt_metrics_u8(p, g, ("ad",), area=area, **kw) == {"ad": got}
    pair = ops.gt_metrics_u8(p, g, ("ld", "ad"), area=area, **kw)             # one run of the chain: LD is pass 1's
    assert pair == {"ld": ops.ld_u8(p, g, area, **kw), "ad": got}
    assert abs(pair["ld"] - want["ld"]) <= BOUND * max(1.0, want["ld"])
    big = 180 * 234                                                           # MS-SSIM needs sides of 176: a larger working size
    three = ops.gt_metrics_u8(p, g, ("ms_ssim", "ld", "ad"), area=big, **kw)
    assert list(three) == ["ms_ssim", "ld", "ad"]
    assert three == {"ms_ssim": ops.ms_ssim_u8(p, g, area=big), "ld": ops.ld_u8(p, g, big, **kw), "ad": ops.ad_u8(p, g, big, **kw)}


def test_evaluation_scores_ad_against_gt_dir(tmp_path, monkeypatch, capsys):
    """The synthetic route with env.gt_dir and env.gt_ad: PNGs for two of three documents."""
    import admin.settings as ws
    from PIL import Image
    from dvd_amd import ops, val_TDiff
    monkeypatch.chdir(tmp_path)

    def settings(name, gt_ad, docs):
        s = ws.Settings()
        s.env.grid_size, s.env.diffusion_steps = 16, 3
        s.env.num_synthetic_docs, s.env.batch_docs, s.env.full_res = docs, 2, (160, 120)
        s.env.visualize, s.env.use_prestage_nets = False, False
        s.env.gt_dir = str(tmp_path / "gt")
        s.env.gt_ad = gt_ad
        s.name, s.seed, s.severity, s.corruption_number = name, 0, 0, 0
        return s

    gts = {0: _rgb("ad/gt0", 200, 150), 2: _rgb("ad/gt2", 190, 260)}
    os.makedirs("gt")
    for i, a in gts.items():
        Image.fromarray(a).save(f"gt/synthetic_{i:05d}.png")
    plain = settings("plain", False, 1)                              # the default, one document: MS-SSIM alone, as before
    torch.manual_seed(0)
    val_TDiff.run(plain)
    assert len(plain.ms_ssim) == 1 and os.path.exists("vis_hp/synthetic/plain/ms_ssim.txt")
    assert not os.path.exists("vis_hp/synthetic/plain/ad.txt") and not hasattr(plain, "ad")
    s = settings("with_ad", True, 3)
    torch.manual_seed(0)
    capsys.readouterr()
    got = val_TDiff.run(s)
    log = capsys.readouterr().out
    assert len(s.ms_ssim) == 2 and not hasattr(s, "ld")
    assert [p for p, _ in s.ad] == ["synthetic_00000", "synthetic_00002"]
    for path, value in s.ad:
        assert isinstance(value, float) and value >= 0.0 and f"{path} ad {value:.6f}" in log
    for (path, value), (_, ssim) in zip(s.ad, s.ms_ssim):                 # each equal to the metric alone
        k = int(path[-5:])
        assert value == ops.ad_u8(got[k][1], _cuda(gts[k], torch.uint8)), path
        assert ssim == ops.ms_ssim_u8(got[k][1], _cuda(gts[k], torch.uint8)), path
    assert "synthetic_00001 ms_ssim,ad skipped" in log and "mean ad" in log and "mean ms_ssim" in log
    lines = open("vis_hp/synthetic/with_ad/ad.txt").read().split("\n")
    assert [ln.split(" ")[0] for ln in lines if ln] == ["synthetic_00000", "synthetic_00002"]
    assert [ln.split(" ")[1] for ln in lines if ln] == [f"{v:.6f}" for _, v in s.ad]
