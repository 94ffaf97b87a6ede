"""CPU-side checks of the MS-SSIM metric: the float64 model's own properties (tests/msssim_model.py needs no
second implementation for these), the ground-truth file rule of the evaluation, and the argument checks of the new entry
points, which - like tests/test_ragged.py - return before any HIP call, so no device is needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import msssim_model as M
from dvd_amd import lib, ops
from dvd_amd.evaluation import find_gt, gt_candidates

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
PTR = 0x1000          # a non-null "device pointer": rejected calls never follow it
NEW_EXPORTS = ("dvd_resize_gray_scratch_bytes", "dvd_resize_gray_u8", "dvd_ssim_scale", "dvd_ssim_finalize",
               "dvd_reduce2_pair", "dvd_msssim_workspace_bytes", "dvd_msssim_scales")


def last_error():
    return lib.raw().dvd_last_error().decode()


def planes(seed, h=176, w=190):
    rng = np.random.RandomState(seed)
    return np.rint(rng.uniform(0, 255, (h, w))), np.rint(rng.uniform(0, 255, (h, w)))


# ---- the model's own properties ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("preset", M.PRESETS)
def test_identical_planes_give_exactly_one(preset):
    x, _ = planes(0)
    s = M.ssim_scales(x, x.copy(), preset)
    assert s.shape == (5, 2) and (s == 1.0).all()
    # the product of ones is 1; the published weights of the sum add up to 1.0001, and that is what the sum of ones gives
    want = 1.0 if preset == "wang" else float(np.sum(np.asarray(M.WEIGHTS) * 1.0))
    assert M.combine(s, preset) == want


@pytest.mark.parametrize("preset", M.PRESETS)
def test_constant_planes(preset):
    a, b = 37.0, 201.0
    s = M.ssim_scales(np.full((180, 177), a), np.full((180, 177), b), preset)
    np.testing.assert_allclose(s[:, 1], 1.0, rtol=0, atol=1e-12)
    np.testing.assert_allclose(s[:, 0], (2 * a * b + M.C1) / (a * a + b * b + M.C1), rtol=0, atol=1e-12)


@pytest.mark.parametrize("preset", M.PRESETS)
def test_swapping_the_planes_changes_nothing(preset):
    x, y = planes(1)
    assert (M.ssim_scales(x, y, preset) == M.ssim_scales(y, x, preset)).all()


@pytest.mark.parametrize("taps", (2, 5))
def test_reduce_sizes_are_ceil_half(taps):
    for n in (176, 177, 11, 12, 1):
        assert M.reduce_axis(np.arange(n, dtype=np.float64), 0, taps).shape == ((n + 1) // 2,)
    assert M.reduce2(np.zeros((177, 190)), taps).shape == (89, 95)
    x = np.arange(7, dtype=np.float64)
    np.testing.assert_array_equal(M.reduce_axis(x, 0, 2), [0.5, 2.5, 4.5, 6.0])          # the last pair is (x[6], x[6])
    np.testing.assert_array_equal(M.reduce_axis(x, 0, 5), [(6 * 0 + 4 * 1 + 2 + 5 * 0) / 16.0, 2.0, 4.0,
                                                           (4 + 4 * 5 + 6 * 6 + 4 * 6 + 6) / 16.0])


def test_model_sizes_and_presets():
    x, y = planes(2, 175, 176)
    with pytest.raises(ValueError):
        M.ssim_scales(x, y)
    x, y = planes(2, 176, 176)
    assert M.ssim_scales(x, y, "wang").shape == (5, 2)       # the fifth scale of 'wang' is one pixel
    with pytest.raises(ValueError):
        M.ssim_scales(x, y, "matlab")
    assert M.target_size(3508, 2480) == (920, 650) and M.target_size(352, 250, 176 * 248) == (248, 176)


def test_resize_at_ratio_one_is_the_identity():
    img = np.random.RandomState(3).randint(0, 256, (23, 17, 3)).astype(np.uint8)
    np.testing.assert_array_equal(M.axis_matrix(17, 17), np.eye(17))
    np.testing.assert_array_equal(M.resize_u8(img, 23, 17), img)


def test_resize_at_ratio_half_is_the_1331_filter():
    n = 14
    x = np.random.RandomState(4).uniform(0, 255, n)
    pad = np.concatenate([x[:1], x, x[-1:]])                 # indices clamped at the ends
    want = np.array([(pad[2 * o] + 3 * pad[2 * o + 1] + 3 * pad[2 * o + 2] + pad[2 * o + 3]) / 8.0 for o in range(n // 2)])
    np.testing.assert_allclose(M.axis_matrix(n, n // 2) @ x, want, rtol=0, atol=1e-12)


def test_gray_is_the_rounded_weighted_sum():
    rng = np.random.RandomState(5)
    rgb = rng.randint(0, 256, (64, 64, 3)).astype(np.uint8)
    f = 0.2989 * rgb[..., 0] + 0.5870 * rgb[..., 1] + 0.1140 * rgb[..., 2]
    g = M.gray(rgb)
    far = np.abs(f - np.floor(f) - 0.5) > 1e-9               # away from a tie the float expression rounds the same way
    np.testing.assert_array_equal(g[far], np.rint(f)[far])
    assert M.gray(np.array([[[255, 255, 255]]], np.uint8))[0, 0] == 255.0
    assert M.gray(np.array([[[0, 0, 125]]], np.uint8))[0, 0] == 14.0     # 14.25 -> 14
    assert M.gray(np.array([[[0, 25, 0]]], np.uint8))[0, 0] == 15.0      # 14.675 -> 15


def test_replicate_filter_against_scipy():
    ndimage = pytest.importorskip("scipy.ndimage")
    x, _ = planes(6, 40, 53)
    g = M.window()
    assert abs(g.sum() - 1.0) < 1e-15 and g[5] == g.max()
    for axis in (0, 1):
        want = ndimage.correlate1d(x, g, axis=axis, mode="nearest")
        np.testing.assert_allclose(M.filter_axis(x, g, axis, "replicate"), want, rtol=0, atol=1e-11)
    want = ndimage.correlate1d(x, g, axis=1, mode="nearest")[:, 5:-5]
    np.testing.assert_allclose(M.filter_axis(x, g, 1, "valid"), want, rtol=0, atol=1e-11)


# ---- the ground-truth file rule ---------------------------------------------------------------------------------------------
def test_gt_candidates():
    assert gt_candidates("12_1 copy.png") == ["12_1 copy.png", "12.png"]
    assert gt_candidates("some/dir/12_1 copy.png") == ["12_1 copy.png", "12.png"]
    assert gt_candidates("7") == ["7.png"]
    assert gt_candidates("007_2.jpg") == ["007_2.png", "007.png"]
    assert gt_candidates("synthetic_00002") == ["synthetic_00002.png"]      # no LEADING integer


def test_find_gt_prefers_the_exact_stem(tmp_path):
    (tmp_path / "12.png").write_bytes(b"")
    assert find_gt(str(tmp_path), "12_1 copy.png") == str(tmp_path / "12.png")
    (tmp_path / "12_1 copy.png").write_bytes(b"")
    assert find_gt(str(tmp_path), "12_1 copy.png") == str(tmp_path / "12_1 copy.png")
    assert find_gt(str(tmp_path), "13_2.png") is None


def test_gt_dir_defaults_to_off():
    import admin.settings as ws
    env = ws.Settings().env
    assert env.gt_dir == "" and env.metric_preset == "docunet"


# ---- bindings and argument checks (no launch) -------------------------------------------------------------------------------
def test_header_declares_and_lib_binds_the_metric_entry_points():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dvd_hip.h")).read(), flags=re.S)
    for name in NEW_EXPORTS:
        assert re.search(rf"\b{name}\s*\(", text), name
        assert getattr(lib.raw(), name).argtypes == lib.SIGNATURES[name]
    for name in ("dvd_resize_gray_scratch_bytes", "dvd_msssim_workspace_bytes"):
        assert getattr(lib.raw(), name).restype is C.c_long
    for macro, value in (("DVD_SSIM_REPLICATE", lib.SSIM_REPLICATE), ("DVD_SSIM_VALID", lib.SSIM_VALID),
                         ("DVD_MSSSIM_DOCUNET", lib.MSSSIM_DOCUNET), ("DVD_MSSSIM_WANG", lib.MSSSIM_WANG)):
        assert int(re.search(rf"#define\s+{macro}\s+(\d+)", text).group(1)) == value
    assert ops.MSSSIM_WEIGHTS == M.WEIGHTS and ops.MSSSIM_MIN_SIDE == M.MIN_SIDE and ops.MSSSIM_AREA == M.AREA
    assert ops.msssim_target_size(3508, 2480) == M.target_size(3508, 2480)


def test_workspace_bytes():
    raw = lib.raw()
    assert raw.dvd_msssim_workspace_bytes(175, 176, 1) == -1 and "msssim_workspace_bytes" in last_error()
    assert raw.dvd_msssim_workspace_bytes(176, 175, 1) == -1
    assert raw.dvd_msssim_workspace_bytes(176, 176, 0) == -1
    one = raw.dvd_msssim_workspace_bytes(176, 176, 1)
    # 6 x 6 tile partials (two f64 each) and two f32 planes of 88^2, 44^2, 22^2 and 11^2, every piece on a 256-byte boundary
    up = lambda v: -(-v // 256) * 256  # noqa: E731
    assert one == up(36 * 16) + 2 * sum(up(4 * s * s) for s in (88, 44, 22, 11))
    assert raw.dvd_msssim_workspace_bytes(177, 191, 3) >= 3 * 2 * 4 * (89 * 96 + 45 * 48 + 23 * 24 + 12 * 12)
    assert raw.dvd_resize_gray_scratch_bytes(0, 4, 4, 4) == -1 and "resize_gray_scratch_bytes" in last_error()
    assert raw.dvd_resize_gray_scratch_bytes(353, 257, 176, 241) > 0


@pytest.mark.parametrize("what, args", [
    ("h = 175", lambda: (PTR, PTR, 1, 175, 176, 0, PTR, PTR)),
    ("w = 175", lambda: (PTR, PTR, 1, 176, 175, 1, PTR, PTR)),
    ("null workspace at 176", lambda: (PTR, PTR, 1, 176, 176, 0, None, PTR)),
    ("null x", lambda: (None, PTR, 1, 176, 176, 0, PTR, PTR)),
    ("null y", lambda: (PTR, None, 1, 176, 176, 0, PTR, PTR)),
    ("null out", lambda: (PTR, PTR, 1, 176, 176, 0, PTR, None)),
    ("n = 0", lambda: (PTR, PTR, 0, 176, 176, 0, PTR, PTR)),
    ("unknown preset", lambda: (PTR, PTR, 1, 176, 176, 2, PTR, PTR)),
])
def test_msssim_scales_rejects_bad_arguments_before_any_launch(what, args):
    rc = lib.raw().dvd_msssim_scales(*args(), None)
    assert rc == -1, what
    assert "msssim_scales" in last_error(), what
    if "17" in what:
        assert ("null" in last_error()) == ("null" in what), (what, last_error())    # 176 passes the size check, 175 does not


@pytest.mark.parametrize("name, what, args", [
    ("dvd_resize_gray_u8", "null src", lambda: (None, 1, 8, 8, PTR, 4, 4, PTR)),
    ("dvd_resize_gray_u8", "null scratch", lambda: (PTR, 1, 8, 8, PTR, 4, 4, None)),
    ("dvd_resize_gray_u8", "n = 0", lambda: (PTR, 0, 8, 8, PTR, 4, 4, PTR)),
    ("dvd_resize_gray_u8", "out_h = 0", lambda: (PTR, 1, 8, 8, PTR, 0, 4, PTR)),
    ("dvd_ssim_scale", "null partials", lambda: (PTR, PTR, 1, 32, 32, 0, None)),
    ("dvd_ssim_scale", "h = 10", lambda: (PTR, PTR, 1, 10, 32, 1, PTR)),
    ("dvd_ssim_scale", "unknown border", lambda: (PTR, PTR, 1, 32, 32, 2, PTR)),
    ("dvd_ssim_scale", "n = 0", lambda: (PTR, PTR, 0, 32, 32, 0, PTR)),
    ("dvd_ssim_finalize", "null out", lambda: (PTR, 1, 4, 100, None, 0)),
    ("dvd_ssim_finalize", "scale = 5", lambda: (PTR, 1, 4, 100, PTR, 5)),
    ("dvd_ssim_finalize", "count = 0", lambda: (PTR, 1, 4, 0, PTR, 0)),
    ("dvd_reduce2_pair", "null x_out", lambda: (PTR, PTR, None, PTR, 1, 8, 8, 2)),
    ("dvd_reduce2_pair", "taps = 3", lambda: (PTR, PTR, PTR, PTR, 1, 8, 8, 3)),
    ("dvd_reduce2_pair", "w = 0", lambda: (PTR, PTR, PTR, PTR, 1, 8, 0, 5)),
])
def test_metric_kernels_reject_bad_arguments_before_any_launch(name, what, args):
    rc = getattr(lib.raw(), name)(*args(), None)
    assert rc == -1, (name, what)
    assert name[4:] in last_error(), (name, what, last_error())


def test_ops_checks_return_before_any_launch():
    x = torch.zeros(1, 176, 176)
    with pytest.raises(ValueError, match="preset"):
        ops.ssim_scales(x, x, preset="matlab")
    with pytest.raises(ValueError, match="preset"):
        ops.ms_ssim_u8(torch.zeros(200, 200, 3, dtype=torch.uint8), torch.zeros(200, 200, 3, dtype=torch.uint8), preset="ssim")
    with pytest.raises(ValueError, match="one shape"):
        ops.ssim_scales(x, torch.zeros(1, 176, 177))
    with pytest.raises(ValueError, match="one shape"):
        ops.ssim_scales(x[0], x[0])                                        # [H,W]: the batch axis is not optional
    with pytest.raises(ValueError, match="176"):
        ops.ssim_scales(torch.zeros(1, 175, 300), torch.zeros(1, 175, 300))
    with pytest.raises(lib.DvdError, match="device tensor"):
        ops.ssim_scales(x, x)                                              # 176 is accepted; a CPU tensor is not
    with pytest.raises(lib.DvdError, match="device tensor"):
        ops.ms_ssim(x, x, preset="wang")
    with pytest.raises(ValueError, match="N,H,W,3"):
        ops.resize_gray_u8(torch.zeros(8, 8, 3, dtype=torch.uint8), 4, 4)
    with pytest.raises(ValueError, match="bad shape"):
        ops.resize_gray_u8(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), 0, 4)
    with pytest.raises(lib.DvdError, match="device tensor"):
        ops.resize_gray_u8(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), 4, 4)
    with pytest.raises(ValueError, match="below 176"):
        ops.ms_ssim_u8(torch.zeros(300, 420, 3, dtype=torch.uint8), torch.zeros(352, 250, 3, dtype=torch.uint8), area=170 * 240)
    with pytest.raises(lib.DvdError, match="device tensor"):
        ops.ms_ssim_u8(torch.zeros(300, 420, 3, dtype=torch.uint8), torch.zeros(352, 250, 3, dtype=torch.uint8), area=176 * 248)


class _OnDevice:
    """A tensor that says it lives on the device: contiguity and dtype are checked after the device, and no GPU is here."""
    def __init__(self, t):
        self._t = t

    is_cuda = True

    def __getattr__(self, name):
        return getattr(self._t, name)


def test_ops_reject_non_contiguous_and_wrong_dtype_before_any_launch():
    base = torch.zeros(1, 176, 352)
    strided = _OnDevice(base[:, :, ::2])
    assert tuple(strided.shape) == (1, 176, 176) and not strided.is_contiguous()
    with pytest.raises(lib.DvdError, match="contiguous"):
        ops.ssim_scales(strided, strided)
    half = _OnDevice(torch.zeros(1, 176, 176, dtype=torch.float16))
    with pytest.raises(lib.DvdError, match="contiguous torch.float32"):
        ops.ssim_scales(half, half)
    img = _OnDevice(torch.zeros(1, 8, 16, 3, dtype=torch.uint8)[:, :, ::2])
    with pytest.raises(lib.DvdError, match="contiguous"):
        ops.resize_gray_u8(img, 4, 4)


def test_msssim_combine_matches_the_model():
    s = np.random.RandomState(7).uniform(0.2, 1.0, (5, 2))
    for preset in M.PRESETS:
        assert abs(ops.msssim_combine(s.tolist(), preset) - float(M.combine(s, preset))) < 1e-15
