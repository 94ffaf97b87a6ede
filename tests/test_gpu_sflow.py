"""The local-distortion kernels (dvd_amd/csrc/sflow.hip) against the integer model of tests/sflow_model.py.

Everything but LD is an integer and is held to the model exactly: descriptors, cost volumes and flows are compared with
array_equal.  LD is a float64 mean of at most 2^20 correctly rounded square roots; only the order of the additions can differ
from the model's, which moves the sum by at most N 2^-53 relative, so |LD - model| <= 1e-9 max(1, LD).
Expected values come from the model at test time; the shapes are the smallest that take every path: a plane smaller than the
descriptor's halo, sizes that are no multiple of a tile, more than one workgroup, the 5 x 5 label grid (registers), the 7 x 7
and 21 x 21 grids (LDS), odd sizes through the pyramid's ceil, a batch."""
import os

import numpy as np
import pytest
import torch

import msssim_model as MS
import sflow_model as M
from dvd_amd import synth

pytestmark = pytest.mark.gpu

SMALL = dict(levels=2, w_top=3, w=2, iters_top=12, iters=6)


def _cuda(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()


def _checker(h, w):
    ys, xs = np.mgrid[0:h, 0:w]
    return ((ys + xs) % 2) * 255


def _stripes(h, w):
    """Columns in pairs of 0 and 255: |gx| = 255 at every interior pixel, the largest histogram entries (the chequerboard's
    central differences vanish in its interior)."""
    return np.broadcast_to(((np.arange(w) // 2) % 2) * 255, (h, w)).copy()


DESCRIPTOR_PLANES = {
    "13x12": lambda: M.page(13, 12, 1),                      # smaller than the halo: everything clamps
    "37x53": lambda: M.page(37, 53, 2),                      # 3 x 4 tiles, none of them full on the right / bottom
    "flat": lambda: np.full((18, 21), 131),                  # n = 0: eps alone divides
    "checker": lambda: _checker(20, 23),                     # 0 / 255 chequerboard
    "stripes": lambda: _stripes(20, 23),                     # the largest sum of squares: the 64-bit norm
}


@pytest.mark.parametrize("name", list(DESCRIPTOR_PLANES))
def test_descriptors_equal_the_model(name):
    from dvd_amd import ops
    img = DESCRIPTOR_PLANES[name]()
    want = M.dsift(img)
    got = ops.dense_sift_u8(_cuda(img[None]))
    assert got.shape == (1,) + want.shape and got.dtype == torch.uint8
    assert np.array_equal(got[0].cpu().numpy(), want)
    if name == "flat":
        assert not want.any()
    if name == "stripes":
        assert want.max() > 0


@pytest.fixture(scope="module")
def one_level():
    """37 x 53, random window centres in -2..2: descriptors, offsets and the model's cost volume, computed once"""
    rng = np.random.default_rng(5)
    a = M.page(37, 53, 90)
    b = M.shifted(a, 2, -1)
    da, db = M.dsift(a), M.dsift(b)
    off = (rng.integers(-2, 3, (37, 53)), rng.integers(-2, 3, (37, 53)))
    return da, db, off, M.cost_volume(da, db, off, 2)


def test_one_level_cost_volume(one_level):
    from dvd_amd import ops
    da, db, off, want = one_level
    got = ops.sflow_cost(_cuda(da, torch.uint8), _cuda(db, torch.uint8), _cuda(np.stack(off), torch.int16), 2)
    assert np.array_equal(got.cpu().numpy(), want)


@pytest.mark.parametrize("iters", [1, 5])
def test_one_level_flow(one_level, iters):
    """1 and 5 iterations: the last message buffer is the second and the first of the ping-pong pair"""
    from dvd_amd import ops
    da, db, off, dc = one_level
    p = M.params()
    want = M.select(dc, M.propagate(dc, off, 2, iters, p["alpha"], p["d"]), off, 2)
    got = ops.sflow_level(_cuda(da, torch.uint8), _cuda(db, torch.uint8), _cuda(np.stack(off), torch.int16), 2, iters)
    assert got.dtype == torch.int16 and np.array_equal(got.cpu().numpy(), want)


def test_top_level_window_of_ten():
    """L = 441 labels: the LDS route, seven labels per lane"""
    from dvd_amd import ops
    a = M.page(19, 27, 7)
    b = M.shifted(a, -1, 1)
    da, db = M.dsift(a), M.dsift(b)
    zero = np.zeros((19, 27), np.int64)
    dc = M.cost_volume(da, db, (zero, zero), 10)
    p = M.params()
    want = M.select(dc, M.propagate(dc, (zero, zero), 10, 3, p["alpha"], p["d"]), (zero, zero), 10)
    off = _cuda(np.zeros((2, 19, 27)), torch.int16)
    assert np.array_equal(ops.sflow_cost(_cuda(da, torch.uint8), _cuda(db, torch.uint8), off, 10).cpu().numpy(), dc)
    got = ops.sflow_level(_cuda(da, torch.uint8), _cuda(db, torch.uint8), off, 10, 3)
    assert np.array_equal(got.cpu().numpy(), want)


CHAINS = {
    "37x53": (37, 53, (2, -1), SMALL),
    "48x64": (48, 64, (-3, 2), SMALL),
    "50x70": (50, 70, (-2, 1), dict(levels=3, w_top=3, w=2, iters_top=8, iters=4)),       # 25 x 35, 13 x 18: odd through ceil
}


@pytest.mark.parametrize("name", list(CHAINS))
def test_whole_chain(name):
    from dvd_amd import ops
    h, w, (su, sv), kw = CHAINS[name]
    a = M.page(h, w, h + w)
    b = M.shifted(a, su, sv)
    want_flow, want_ld = M.sift_flow(a, b, **kw)
    flow, ld = ops.sift_flow(_cuda(a[None]), _cuda(b[None]), **kw)
    assert flow.shape == (1, 2, h, w) and flow.dtype == torch.int16 and ld.shape == (1,) and ld.dtype == np.float64
    assert np.array_equal(flow[0].cpu().numpy(), want_flow)
    print(f"{name}: LD {ld[0]!r} against the model's {want_ld!r}")
    assert abs(ld[0] - want_ld) <= 1e-9 * max(1.0, want_ld)
    assert ops.local_distortion(_cuda(a[None]), _cuda(b[None]), **kw)[0] == ld[0]
    same_flow, same_ld = ops.sift_flow(_cuda(a[None]), _cuda(a[None]), **kw)
    assert not bool(same_flow.any()) and same_ld[0] == 0.0


def test_batch_document_equals_itself_alone():
    from dvd_amd import ops
    pages = [M.page(40, 44, s) for s in (11, 12, 13)]
    a = np.stack(pages)
    b = np.stack([M.shifted(pages[0], 1, 3), M.shifted(pages[1], -2, 0), pages[2]])
    flow, ld = ops.sift_flow(_cuda(a), _cuda(b), **SMALL)
    assert flow.shape == (3, 2, 40, 44) and ld.shape == (3,)
    for k in range(3):
        f1, l1 = ops.sift_flow(_cuda(a[k:k + 1]), _cuda(b[k:k + 1]), **SMALL)
        assert torch.equal(f1[0], flow[k]) and l1[0] == ld[k], k
    assert ld[2] == 0.0 and ld[0] > 1.0
    assert np.array_equal(flow[0].cpu().numpy(), M.sift_flow(a[0], b[0], **SMALL)[0])


def _rgb(key, h, w):
    img = synth.smooth_image(key, h, w).transpose(1, 2, 0).astype(np.float64) * 255.0
    noise = (synth.uniform01(key + "/n", h * w * 3, 5).reshape(h, w, 3).astype(np.float64) - 0.5) * 60.0
    return np.clip(np.rint(img + noise), 0, 255).astype(np.uint8)


def test_ld_u8_end_to_end():
    """The benchmark's preparation, then the chain: equal to the model on the model-resized planes.  The device resize equals
    the model's except where a value lies exactly on k + 0.5 before its rounding; the inputs hold no such pixel (counted from
    the model), so the planes - and with them every integer after them - are the model's."""
    from dvd_amd import ops
    gt = _rgb("ld/gt", 200, 260)
    noise = (synth.uniform01("ld/pred/n", 200 * 260 * 3, 3).reshape(200, 260, 3).astype(np.float64) - 0.5) * 30.0
    pred = np.clip(np.rint(np.roll(gt, (3, -4), axis=(0, 1)) + noise), 0, 255).astype(np.uint8)
    gt, pred = gt & 0xF8, pred & 0xF8                 # 200 -> 60 puts 3 pixels of arbitrary bytes on exact halves; multiples of 8: none
    area = 60 * 78
    assert MS.target_size(200, 260, area) == (60, 78)
    assert not MS.knife_edge(pred, 60, 78).any() and not MS.knife_edge(gt, 60, 78).any()
    kw = dict(levels=2, w_top=3, w=2, iters_top=6, iters=4)
    want_flow, want = M.sift_flow(MS.resize_gray(gt, 60, 78), MS.resize_gray(pred, 60, 78), **kw)
    got = ops.ld_u8(_cuda(pred, torch.uint8), _cuda(gt, torch.uint8), area, **kw)
    print(f"ld_u8: {got!r} against the model's {want!r}")
    assert isinstance(got, float) and want_flow.any()
    assert abs(got - want) <= 1e-9 * max(1.0, want)
    both = ops.gt_metrics_u8(_cuda(pred, torch.uint8), _cuda(gt, torch.uint8), ("ld",), area=area, **kw)
    assert both == {"ld": got}


def test_evaluation_scores_ld_against_gt_dir(tmp_path, monkeypatch, capsys):
    """The synthetic route with env.gt_dir and env.gt_metrics: PNGs for two of three documents."""
    import admin.settings as ws
    from PIL import Image
    from dvd_amd import ops, val_TDiff
    monkeypatch.chdir(tmp_path)

    def settings(name, metrics=None):
        s = ws.Settings()
        s.env.grid_size, s.env.diffusion_steps = 16, 3
        s.env.num_synthetic_docs, s.env.batch_docs, s.env.full_res = 3, 2, (160, 120)
        s.env.visualize, s.env.use_prestage_nets = False, False
        s.env.gt_dir = str(tmp_path / "gt")
        if metrics is not None:
            s.env.gt_metrics = metrics
        s.name, s.seed, s.severity, s.corruption_number = name, 0, 0, 0
        return s

    gts = {0: _rgb("ld/gt0", 200, 150), 2: _rgb("ld/gt2", 190, 260)}
    os.makedirs("gt")
    for i, a in gts.items():
        Image.fromarray(a).save(f"gt/synthetic_{i:05d}.png")
    plain = settings("plain")                                       # the default: MS-SSIM alone, as before
    torch.manual_seed(0)
    want = val_TDiff.run(plain)
    assert not os.path.exists("vis_hp/synthetic/plain/ld.txt") and not hasattr(plain, "ld")
    s = settings("both", "ms_ssim,ld")
    torch.manual_seed(0)
    capsys.readouterr()
    got = val_TDiff.run(s)
    log = capsys.readouterr().out
    for (pa, a), (pb, b) in zip(want, got):
        assert pa == pb and torch.equal(a, b), pa
    assert s.ms_ssim == plain.ms_ssim and len(s.ms_ssim) == 2         # bit-equal to the run without 'ld'
    assert [p for p, _ in s.ld] == ["synthetic_00000", "synthetic_00002"]
    for path, value in s.ld:
        assert isinstance(value, float) and value >= 0.0 and f"{path} ld {value:.6f}" in log
    assert s.ld[0][1] == ops.ld_u8(got[0][1], _cuda(gts[0], torch.uint8))
    assert "synthetic_00001 ms_ssim,ld skipped" in log and "mean ld" in log and "mean ms_ssim" in log
    lines = open("vis_hp/synthetic/both/ld.txt").read().split("\n")
    assert [ln.split(" ")[0] for ln in lines if ln] == ["synthetic_00000", "synthetic_00002"]
    assert open("vis_hp/synthetic/both/ms_ssim.txt").read() == open("vis_hp/synthetic/plain/ms_ssim.txt").read()
