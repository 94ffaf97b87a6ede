"""The MS-SSIM kernels (dvd_amd/csrc/metrics.hip) against the float64 model of tests/msssim_model.py.

Bars.  The metric is printed to four decimals, so |ms_ssim - model| <= 5e-5 on every input (BAR_MS).  The per-scale bar is
MEASURED, not chosen: `restate_f32` below is an f32 NumPy restatement of the kernels' arithmetic (both planes less 127.5, the
window applied separably along the row and then down the column, every product and sum rounded to f32, the reduce in f32);
its largest deviation from the float64 model over the inputs of this file, on the CPU, is
    RESTATED_DEV = 3.71e-06   (the ssim of scale 1 of 'wang' on the 177 x 191 pair with the flat 250 / 251 region)
and the bar is 4 x that figure, BAR_SCALE = 1.48e-05: the margin covers the tile reduction's and the vertical pass's other
summation orders and the kernels' fused multiply-adds.  The test recomputes the figure and holds the kernels to
4 x what it finds; the kernels' own output never enters a bar.
The kernels' own figures: not yet run on an MI355X (DESIGN.md 4.3 records them once they are).
"""
import os

import numpy as np
import pytest
import torch

import msssim_model as M
from dvd_amd import synth

pytestmark = pytest.mark.gpu

BAR_MS = 5e-5
F32 = np.float32


# ---- inputs (CPU, deterministic) --------------------------------------------------------------------------------------------
def _page(key, h, w):
    return np.rint(synth.smooth_image(key, h, w).mean(axis=0).astype(np.float64) * 255.0)


def smooth_pair(key, h, w):
    """A page and a warped (shifted, blended) and noised copy: scores land mid-range."""
    x = _page(key, h, w)
    noise = (synth.uniform01(key + "/n", h * w, 7).reshape(h, w).astype(np.float64) - 0.5) * 40.0
    y = 0.6 * x + 0.4 * np.roll(x, (2, 3), axis=(0, 1)) + noise
    return x, np.clip(np.rint(y), 0, 255)


def flat_pair(key, h, w):
    """The worst case of the cancellation in E[x^2] - mu^2: a flat 70 x 70 region at 250 against 251."""
    x, y = smooth_pair(key, h, w)
    x[40:110, 50:120], y[40:110, 50:120] = 250.0, 251.0
    return x, y


def noise_pair(key, h, w):
    """Independent noise: covariance near 0, small cs in the product combination."""
    u = synth.uniform01(key, 2 * h * w, 11).reshape(2, h, w).astype(np.float64)
    return np.floor(u[0] * 256.0).clip(0, 255), np.floor(u[1] * 256.0).clip(0, 255)


def _batch(*pairs):
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


CASES = {
    "smooth176x176": lambda: _batch(smooth_pair("ms/a", 176, 176)),          # the fifth scale of 'wang' is one pixel
    "flat177x191": lambda: _batch(flat_pair("ms/b", 177, 191)),              # odd at every level
    "noise200x333": lambda: _batch(noise_pair("ms/c", 200, 333)),            # tiles cut on both axes at every scale
    "batch3x176x208": lambda: _batch(smooth_pair("ms/d0", 176, 208), flat_pair("ms/d1", 176, 208),
                                     noise_pair("ms/d2", 176, 208)),         # grid z, the per-document finalize
}


# ---- the f32 restatement of the kernels' arithmetic -------------------------------------------------------------------------
def _filter_f32(a, g, axis, border):
    a = np.moveaxis(a, axis, -1)
    n = a.shape[-1]
    idx = np.arange(n - 10 if border == "valid" else n)
    acc = np.zeros(a.shape[:-1] + (len(idx),), F32)
    for k in range(11):
        src = a[..., idx + k] if border == "valid" else a[..., np.clip(idx + k - 5, 0, n - 1)]
        acc = acc + g[k] * src                                      # f32 product, f32 sum
    return np.moveaxis(acc, -1, axis)


def _reduce_f32(a, axis, taps):
    a = np.moveaxis(a, axis, -1)
    n = a.shape[-1]
    i = np.arange((n + 1) // 2)
    t = lambda d: a[..., np.clip(2 * i + d, 0, n - 1)]              # noqa: E731
    if taps == 2:
        out = (t(0) + t(1)) * F32(0.5)
    else:
        out = (((t(-2) + t(2)) + F32(4) * (t(-1) + t(1))) + F32(6) * t(0)) * F32(0.0625)
    return np.moveaxis(out, -1, axis)


def restate_f32(x, y, preset):
    """[N,H,W] -> [N,5,2] float64, every step of the kernels in float32 (means of the maps in float64, as the finalize)."""
    g = M.window().astype(F32)
    c1, c2, c = F32(M.C1), F32(M.C2), F32(127.5)
    border, taps = ("valid", 2) if preset == "wang" else ("replicate", 5)
    x, y = x.astype(F32), y.astype(F32)
    out = []
    for s in range(5):
        a, b = x - c, y - c
        f = lambda p: _filter_f32(_filter_f32(p, g, -1, border), g, -2, border)   # noqa: E731
        mx, my, exx, eyy, exy = f(a), f(b), f(a * a), f(b * b), f(a * b)
        vxx, vyy, vxy = exx - mx * mx, eyy - my * my, exy - mx * my
        cs = ((vxy + vxy) + c2) / ((vxx + vyy) + c2)
        ux, uy = mx + c, my + c
        uxy = ux * uy
        ssim = cs * (((uxy + uxy) + c1) / ((ux * ux + uy * uy) + c1))
        assert ssim.dtype == F32 and cs.dtype == F32
        out.append(np.stack([ssim.astype(np.float64).mean(axis=(-2, -1)), cs.astype(np.float64).mean(axis=(-2, -1))], -1))
        if s < 4:
            x, y = (_reduce_f32(_reduce_f32(p, -1, taps), -2, taps) for p in (x, y))
    return np.stack(out, axis=-2)


@pytest.fixture(scope="module")
def data():
    """Inputs, the model's numbers and the restatement's, computed once and left unchanged."""
    d = {}
    for name, make in CASES.items():
        x, y = make()
        d[name] = {"x": x, "y": y}
        for preset in M.PRESETS:
            d[name][preset] = M.ssim_scales(x, y, preset)
            d[name][preset + "/f32"] = restate_f32(x, y, preset)
    dev = max(float(np.abs(d[n][p + "/f32"] - d[n][p]).max()) for n in CASES for p in M.PRESETS)
    d["restated_dev"] = dev
    return d


def _cuda(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda().contiguous()


def test_restated_deviation_is_the_recorded_one(data):
    """The figure in this file's header is what the restatement gives (CPU arithmetic only, but it sets a GPU bar)."""
    dev = data["restated_dev"]
    print(f"restated f32 deviation {dev:.3e}, per-scale bar {4 * dev:.3e}")
    assert 0.0 < dev and abs(dev - 3.71e-06) <= 0.02e-06, dev
    for n in CASES:                               # mid-range scores, small cs on the noise pair
        print(n, [round(float(v), 4) for v in M.combine(data[n]["docunet"], "docunet")],
              [round(float(v), 4) for v in M.combine(data[n]["wang"], "wang")])
    assert 0.2 < float(M.combine(data["smooth176x176"]["docunet"], "docunet")[0]) < 0.95
    # independent noise: no covariance at the fine scales (the coarse ones flatten towards C2 / C2), a small product
    assert float(np.abs(data["noise200x333"]["wang"][0, :2, 1]).max()) < 0.02
    assert float(M.combine(data["noise200x333"]["wang"], "wang")[0]) < 0.2


@pytest.mark.parametrize("preset", M.PRESETS)
@pytest.mark.parametrize("case", list(CASES))
def test_ssim_scales_against_the_model(data, case, preset):
    from dvd_amd import ops
    d = data[case]
    got = ops.ssim_scales(_cuda(d["x"]), _cuda(d["y"]), preset).cpu().numpy().astype(np.float64)
    want = d[preset]
    assert got.shape == want.shape == (d["x"].shape[0], 5, 2)
    bar = 4.0 * data["restated_dev"]
    err = float(np.abs(got - want).max())
    ms_got = np.array([ops.msssim_combine(s.tolist(), preset) for s in got])
    ms_err = float(np.abs(ms_got - M.combine(want, preset)).max())
    print(f"{case} {preset}: per-scale err {err:.3e} (bar {bar:.3e}), ms_ssim err {ms_err:.3e} (bar {BAR_MS:.0e}), "
          f"ms_ssim {[round(float(v), 5) for v in ms_got]}")
    assert err <= bar, (err, bar)
    assert ms_err <= BAR_MS, ms_err
    # ops.ms_ssim is the same combination of the same launch
    np.testing.assert_array_equal(ops.ms_ssim(_cuda(d["x"]), _cuda(d["y"]), preset), ms_got)


@pytest.mark.parametrize("preset", M.PRESETS)
def test_exactness_probes(data, preset):
    from dvd_amd import ops
    d = data["batch3x176x208"]
    x, y = _cuda(d["x"]), _cuda(d["y"])
    same = ops.ssim_scales(x, x.clone(), preset)
    assert same.shape == (3, 5, 2) and bool((same == 1.0).all()), same            # identical inputs: 1.0f, ssim and cs alike
    a, b = ops.ssim_scales(x, y, preset), ops.ssim_scales(x, y, preset)
    assert torch.equal(a, b)                                                       # an ordered reduction: the same bits
    for k in range(3):                                                             # document k of the batch == alone
        assert torch.equal(ops.ssim_scales(x[k:k + 1].contiguous(), y[k:k + 1].contiguous(), preset)[0], a[k]), k
    d = data["noise200x333"]                                                       # partial tiles on both axes
    x, y = _cuda(d["x"]), _cuda(d["y"])
    assert bool((ops.ssim_scales(y, y.clone(), preset) == 1.0).all())
    assert torch.equal(ops.ssim_scales(x, y, preset), ops.ssim_scales(x, y, preset))


def _rgb(key, h, w):
    """A noised page.  Its outermost rows and columns are constant along themselves: where an upscale clamps every tap of one
    axis onto the border sample, the other axis alone decides the value, and at 180 -> 200 its weights are multiples of 1/20,
    which would put 5 % of a noisy border row exactly on k + 0.5 (the knife edge the resize test has to waive)."""
    img = synth.smooth_image(key, h, w).transpose(1, 2, 0).astype(np.float64) * 255.0
    noise = (synth.uniform01(key + "/n", h * w * 3, 5).reshape(h, w, 3).astype(np.float64) - 0.5) * 60.0
    out = np.clip(np.rint(img + noise), 0, 255).astype(np.uint8)
    out[0], out[-1] = out[0, w // 2], out[-1, w // 2]
    out[:, 0], out[:, -1] = out[h // 2, 0], out[h // 2, -1]
    return out


@pytest.mark.parametrize("shape", [(353, 257, 176, 241), (180, 180, 353, 200)], ids=lambda s: "%dx%d-%dx%d" % s)
def test_resize_gray_against_the_model(shape):
    from dvd_amd import ops
    h, w, oh, ow = shape
    imgs = np.stack([_rgb("ms/rs0", h, w), _rgb("ms/rs1", h, w)])
    if w == 180 and ow == 200:
        # 180 -> 200 has weights that are odd multiples of 1/20 (0.25 / 0.75 among them) and 180 -> 353 has one row of
        # weights 0.5 / 0.5: on arbitrary bytes 0.12 .. 0.2 % of the pixels are EXACT halves, the knife edge this test has
        # to waive.  Bytes that are multiples of 8 hold none (counted below, from the model).
        imgs &= 0xF8
    got = ops.resize_gray_u8(_cuda(imgs, torch.uint8), oh, ow).cpu().numpy()
    assert got.shape == (2, oh, ow) and got.dtype == np.float32
    for k in range(2):
        want = M.resize_gray(imgs[k], oh, ow)
        edge = M.knife_edge(imgs[k], oh, ow)                  # counted from the MODEL: a byte may differ only there
        assert edge.mean() < 1e-3, edge.mean()                # the inputs put fewer than 0.1 % of the pixels on the edge
        diff = np.abs(got[k].astype(np.float64) - want)
        print(f"{shape} image {k}: {int(edge.sum())} knife-edge pixels, {int((diff > 0).sum())} pixels differ")
        assert (diff[~edge] == 0).all(), int((diff[~edge] > 0).sum())
        assert (diff[edge] <= 1).all()


@pytest.mark.parametrize("preset", M.PRESETS)
def test_ms_ssim_u8_end_to_end(preset):
    from dvd_amd import ops
    gt = _rgb("ms/gt", 352, 250)
    noise = (synth.uniform01("ms/pred/n", 300 * 420 * 3, 3).reshape(300, 420, 3).astype(np.float64) - 0.5) * 50.0
    pred = np.clip(np.rint(M.resize_f64(np.roll(gt, (3, -2), axis=(0, 1)), 300, 420) + noise), 0, 255).astype(np.uint8)
    area = 176 * 248
    assert M.target_size(352, 250, area) == (248, 176)
    th, tw = 248, 176
    assert max(M.knife_edge(pred, th, tw).mean(), M.knife_edge(gt, th, tw).mean()) < 1e-3
    want = M.ms_ssim_u8(pred, gt, preset, area)
    got = ops.ms_ssim_u8(_cuda(pred, torch.uint8), _cuda(gt, torch.uint8), preset, area)
    print(f"ms_ssim_u8 {preset}: {got:.6f} against the model's {want:.6f}")
    assert isinstance(got, float) and 0.1 < want < 0.98
    assert abs(got - want) <= BAR_MS, (got, want)


def test_evaluation_scores_against_gt_dir(tmp_path, monkeypatch, capsys):
    """The synthetic route with env.gt_dir: PNGs for two of three documents."""
    import admin.settings as ws
    from PIL import Image
    from dvd_amd import ops, val_TDiff
    monkeypatch.chdir(tmp_path)

    def settings(name):
        s = ws.Settings()
        s.env.grid_size, s.env.diffusion_steps = 16, 3
        s.env.num_synthetic_docs, s.env.batch_docs, s.env.full_res = 3, 2, (160, 120)
        s.env.visualize, s.env.use_prestage_nets = False, False
        s.name, s.seed, s.severity, s.corruption_number = name, 0, 0, 0
        return s

    torch.manual_seed(0)
    want = val_TDiff.run(settings("plain"))                       # what the function returns today
    assert not os.path.exists("vis_hp/synthetic/plain/ms_ssim.txt")
    gts = {0: _rgb("ms/gt0", 200, 150), 2: _rgb("ms/gt2", 190, 260)}
    os.makedirs("gt")
    for i, a in gts.items():
        Image.fromarray(a).save(f"gt/synthetic_{i:05d}.png")
    s = settings("scored")
    s.env.gt_dir = str(tmp_path / "gt")
    torch.manual_seed(0)
    capsys.readouterr()
    got = val_TDiff.run(s)
    log = capsys.readouterr().out
    assert len(got) == len(want) == 3
    for (pa, a), (pb, b) in zip(want, got):
        assert pa == pb and torch.equal(a, b), pa
    assert [p for p, _ in s.ms_ssim] == ["synthetic_00000", "synthetic_00002"]
    for (path, value), i in zip(s.ms_ssim, (0, 2)):
        assert value == ops.ms_ssim_u8(got[i][1], _cuda(gts[i], torch.uint8))
        assert f"{path} ms_ssim {value:.6f}" in log
    assert "synthetic_00001 ms_ssim skipped" in log and "mean ms_ssim" in log
    lines = open("vis_hp/synthetic/scored/ms_ssim.txt").read().split("\n")
    assert [ln.split(" ")[0] for ln in lines if ln] == ["synthetic_00000", "synthetic_00002"]
