"""CPU checks of the bicubic warp mode: the float64 model of tests/bicubic_model.py against torch's own CPU kernel (so the
model - the yardstick of tests/test_gpu_bicubic.py - is F.grid_sample's bicubic, not a private one), and the argument
checks of the Python surface that need no device."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bicubic_model as BM

# (source shape, output size): identity-sized, odd sizes with magnification, minification, a large source
CASES = [((2, 3, 16, 16), (16, 16)), ((2, 3, 37, 52), (40, 64)), ((2, 3, 64, 64), (96, 32)), ((2, 3, 200, 300), (64, 64))]


@pytest.mark.parametrize("sshape,osize", CASES, ids=lambda v: "x".join(map(str, v)))
def test_model_agrees_with_torch_cpu_bicubic(sshape, osize):
    """Source uniform in 0..255, grid uniform in [-1.15, 1.15] (taps fall off every side): torch's f32 CPU kernel is within
    the per-value bound K 2^-24 S of the model (bicubic_model's docstring derives K = 20 for the HIP kernels' sequence;
    torch's own sequence needs K of about 7)."""
    gen = torch.Generator().manual_seed(sum(sshape) + osize[0])
    src = torch.rand(sshape, generator=gen) * 255.0
    grid = (torch.rand((sshape[0], 2) + osize, generator=gen) * 2.0 - 1.0) * 1.15
    want = F.grid_sample(src, grid.permute(0, 2, 3, 1), mode="bicubic", padding_mode="zeros", align_corners=True).numpy()
    model, s_abs = BM.bicubic_model(src.numpy(), grid.numpy())
    print(f"torch CPU vs model: worst K = {BM.worst_k(want, model, s_abs):.2f} (bound K = {BM.K})")
    assert np.all(np.abs(want - model) <= BM.bound(s_abs))


def test_model_tells_a_wrong_kernel_apart():
    """The bound is a check, not a formality: A = -0.5, or taps shifted by one column, miss it by orders of magnitude."""
    gen = torch.Generator().manual_seed(3)
    src = torch.rand((1, 2, 24, 24), generator=gen) * 255.0
    grid = (torch.rand((1, 2, 16, 16), generator=gen) * 2.0 - 1.0) * 0.8
    model, s_abs = BM.bicubic_model(src.numpy(), grid.numpy())
    shifted, _ = BM.bicubic_model(torch.roll(src, 1, dims=3).numpy(), grid.numpy())
    assert BM.worst_k(shifted, model, s_abs) > 1e4
    a = BM.A
    try:
        BM.A = -0.5
        other, _ = BM.bicubic_model(src.numpy(), grid.numpy())
    finally:
        BM.A = a
    assert BM.worst_k(other, model, s_abs) > 1e4


def test_model_non_finite_grid_is_nan():
    src = np.arange(2 * 8 * 8, dtype=np.float64).reshape(1, 2, 8, 8)
    grid = np.zeros((1, 2, 4, 4), dtype=np.float32)
    grid[0, 0, 1, 2], grid[0, 1, 3, 0] = np.nan, np.inf
    out, _ = BM.bicubic_model(src, grid)
    assert np.isnan(out[0, :, 1, 2]).all() and np.isnan(out[0, :, 3, 0]).all() and np.isnan(out).sum() == 4


def test_register_model2_accepts_bicubic_and_refuses_nearest():
    from datasets.utils.warping import SpatialTransformer2, register_model2
    m = register_model2((512, 512), "bicubic")
    assert list(m.parameters()) == [] and m.spatial_trans.mode == "bicubic"
    assert SpatialTransformer2((8, 8), "bicubic").mode == "bicubic"
    for bad in ("nearest", "area", "BICUBIC"):
        with pytest.raises(NotImplementedError):
            register_model2((512, 512), bad)


def test_ops_refuse_an_unknown_mode_before_any_launch():
    """mode is checked first: host tensors (which every launch refuses with DvdError) never get that far."""
    from dvd_amd import ops
    flow = torch.zeros(1, 2, 8, 8)
    img = torch.zeros(8, 8, 3, dtype=torch.uint8)
    for bad in ("nearest", "cubic", None):
        with pytest.raises(ValueError, match="'bilinear' or 'bicubic'"):
            ops.grid_sample(torch.zeros(1, 1, 8, 8), torch.zeros(1, 2, 8, 8), mode=bad)
        with pytest.raises(ValueError, match="'bilinear' or 'bicubic'"):
            ops.unwarp_u8(flow, img, mode=bad)
        with pytest.raises(ValueError, match="'bilinear' or 'bicubic'"):
            ops.unwarp_u8_batch(flow, img[None], mode=bad)
        with pytest.raises(ValueError, match="'bilinear' or 'bicubic'"):
            ops.unwarp_u8_ragged(flow, [img], mode=bad)
