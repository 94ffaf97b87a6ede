"""GPU tests of mode='bicubic': dvd_grid_sample_bicubic_zeros_ac (general and LDS-tiled kernels, the direct gather of a
tile too large to stage), the fused u8 tail dvd_unwarp_u8_bicubic_batch / _ragged, and the Python surface above them.

Yardsticks: the float64 model of tests/bicubic_model.py with its per-value bound K 2^-24 S (K = 20, derived there from the
operation sequence of the shared device function; tests/test_bicubic_cpu.py pins the model to torch's CPU kernel), and
bit-equality between kernel routes - every route sums a pixel with the same device function."""
import numpy as np
import pytest
import torch

import bicubic_model as BM
from dvd_amd import lib, ops

pytestmark = pytest.mark.gpu


def _rand(shape, seed, lo=0.0, hi=255.0):
    gen = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=gen) * (hi - lo) + lo


def _smooth_grid(n, h, w, seed, amp=0.05):
    """Identity plus a low-frequency displacement of +-amp: what a dewarping flow looks like."""
    ys = torch.linspace(-1, 1, h)[None, :, None].expand(n, h, w)
    xs = torch.linspace(-1, 1, w)[None, None, :].expand(n, h, w)
    ph = _rand((n, 4), seed, 0.0, 6.28)
    dx = amp * torch.sin(2.1 * ys + ph[:, 0, None, None]) * torch.cos(1.7 * xs + ph[:, 1, None, None])
    dy = amp * torch.cos(1.3 * ys + ph[:, 2, None, None]) * torch.sin(2.6 * xs + ph[:, 3, None, None])
    return torch.stack([xs + dx, ys + dy], 1).contiguous()


def _check(got, src, grid, what, src_batch_div=1):
    """got within the bound of the model everywhere (NaN where the model is NaN); prints the K the kernel needed."""
    model, s_abs = BM.bicubic_model(src.numpy(), grid.numpy(), src_batch_div)
    got = got.cpu().numpy()
    nan = np.isnan(model)
    assert np.array_equal(np.isnan(got), nan), what
    ok = ~nan
    print(f"{what}: worst K = {BM.worst_k(got[ok], model[ok], s_abs[ok]):.2f} (bound K = {BM.K})")
    assert np.all(np.abs(got[ok] - model[ok]) <= BM.bound(s_abs[ok])), what
    return model, s_abs


def test_general_kernel_against_the_model():
    """Odd sizes (w = 7: the general kernel), 5 channels, grid in [-1.3, 1.3]: taps fall off all four sides."""
    src, grid = _rand((2, 5, 13, 19), 1), _rand((2, 2, 11, 7), 2, -1.3, 1.3)
    _check(ops.grid_sample(src.cuda(), grid.cuda(), mode="bicubic"), src, grid, "general")


LDS_CASES = {"magnify": ((2, 4, 48, 64), (96, 96)), "partial_tiles": ((2, 4, 64, 96), (40, 36))}


@pytest.fixture(scope="module")
def lds_runs():
    """The two LDS-kernel problems (w and win multiples of 4), run once: name -> (src, grid, out on the device)."""
    runs = {}
    for k, (name, (sshape, osize)) in enumerate(LDS_CASES.items()):
        src, grid = _rand(sshape, 10 + k), _smooth_grid(sshape[0], osize[0], osize[1], 20 + k)
        runs[name] = (src, grid, ops.grid_sample(src.cuda(), grid.cuda(), mode="bicubic"))
    return runs


@pytest.mark.parametrize("name", list(LDS_CASES))
def test_lds_kernel_against_the_model(lds_runs, name):
    """A smooth grid (identity + a +-0.05 low-frequency displacement).  4 channels leave a remainder of the 3 planes staged
    together; 96 x 96 from 48 x 64 magnifies; 40 x 36 has partial tiles on both edges."""
    src, grid, out = lds_runs[name]
    _check(out, src, grid, f"lds {name}")


def test_lds_and_general_kernels_give_the_same_bits(lds_runs):
    """The first 35 columns of the 40 x 36 problem as a w = 35 problem (the general kernel) equal those columns of the
    w = 36 run (the LDS kernel) bit for bit."""
    src, grid, out36 = lds_runs["partial_tiles"]
    out35 = ops.grid_sample(src.cuda(), grid[..., :35].contiguous().cuda(), mode="bicubic")
    assert torch.equal(out35.view(torch.int32), out36[..., :35].contiguous().view(torch.int32))


def test_staged_and_direct_tiles_give_the_same_bits():
    """src [1,3,64,64] -> 64 x 64 at unit scale (four tiles), smooth grid of +-0.05 = +-1.6 px: a tile's box is about
    39 rows x 44 floats = 1700 floats <= LCAP_C = 3072, so every tile STAGES - asserted from the kernel's box arithmetic
    (bicubic_model.lds_tiles_staged).  With one pixel per tile sent to the opposite corner the tile's box is the whole
    64 x 64 plane = 4096 floats > 3072: every tile gathers DIRECTLY - asserted likewise.  Every unchanged pixel keeps its
    bits."""
    src, grid = _rand((1, 3, 64, 64), 30), _smooth_grid(1, 64, 64, 31)
    assert BM.lds_tiles_staged(grid[0].numpy(), 64, 64) == [True] * 4
    staged = ops.grid_sample(src.cuda(), grid.cuda(), mode="bicubic")
    far = grid.clone()
    moved = torch.zeros(64, 64, dtype=torch.bool)
    for ty in range(2):
        for tx in range(2):
            y, x = ty * 32 + 5 + tx, tx * 32 + 9 + ty
            far[0, 0, y, x] = 0.99 if x < 32 else -0.99      # the corner opposite to the tile's own footprint
            far[0, 1, y, x] = 0.99 if y < 32 else -0.99
            moved[y, x] = True
    assert BM.lds_tiles_staged(far[0].numpy(), 64, 64) == [False] * 4
    direct = ops.grid_sample(src.cuda(), far.cuda(), mode="bicubic")
    keep = ~moved.cuda()
    assert torch.equal(direct.view(torch.int32)[0][:, keep], staged.view(torch.int32)[0][:, keep])
    _check(staged, src, grid, "staged tiles")
    _check(direct, src, far, "direct-gather tiles")


def test_src_batch_div():
    """4 grids on 2 sources with src_batch_div = 2 equal the 4 single calls (and the model, which indexes n // 2)."""
    src, grid = _rand((2, 3, 16, 24), 40).cuda(), _rand((4, 2, 12, 20), 41, -1.1, 1.1).cuda()
    got = ops.grid_sample(src, grid, src_batch_div=2, mode="bicubic")
    for n in range(4):
        one = ops.grid_sample(src[n // 2:n // 2 + 1].contiguous(), grid[n:n + 1].contiguous(), mode="bicubic")
        assert torch.equal(got[n:n + 1].view(torch.int32), one.view(torch.int32)), n
    _check(got, src.cpu(), grid.cpu(), "src_batch_div", src_batch_div=2)


def test_register_model2_bicubic_call_shape():
    """The reference's call shape: register_model2((512, 512), 'bicubic')([feat, grid]) on [2,256,16,16] features."""
    from datasets.utils.warping import register_model2
    feat, grid = _rand((2, 256, 16, 16), 50, -1.0, 1.0), _rand((2, 2, 16, 16), 51, -1.05, 1.05)
    m = register_model2((512, 512), "bicubic")
    got = m([feat.cuda(), grid.cuda()])
    assert torch.equal(got.view(torch.int32), ops.grid_sample(feat.cuda(), grid.cuda(), mode="bicubic").view(torch.int32))
    _check(got, feat, grid, "register_model2")
    assert not torch.equal(got, ops.grid_sample(feat.cuda(), grid.cuda()))          # it is not the bilinear kernel
    with pytest.raises(lib.DvdError):
        m([feat, grid])                                                              # no CPU route


def test_non_finite_grid_values_give_nan():
    """One NaN and one +inf in an 8 x 8 grid on src [1,3,8,8]: those outputs are NaN in every channel, all the others
    within the bound - on the LDS kernel (8 x 8) and on the general kernel (the same grid cut to 8 x 7)."""
    src, grid = _rand((1, 3, 8, 8), 60), _rand((1, 2, 8, 8), 61, -1.1, 1.1)
    grid[0, 0, 2, 3], grid[0, 1, 6, 1] = float("nan"), float("inf")
    for g in (grid, grid[..., :7].contiguous()):
        out = ops.grid_sample(src.cuda(), g.cuda(), mode="bicubic")
        assert torch.isnan(out[0, :, 2, 3]).all() and torch.isnan(out[0, :, 6, 1]).all() and int(torch.isnan(out).sum()) == 6
        _check(out, src, g, f"non-finite w={g.shape[-1]}")


# ---------------------------------------------------------------------------------------------------------------------
# the fused u8 tail
# ---------------------------------------------------------------------------------------------------------------------
TAIL_SIZES = [(45, 38), (160, 100)]      # h + w <= 128: the `small` interpolation order, w % 4 != 0; two tiles wide, five tall


@pytest.fixture(scope="module", params=TAIL_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def tail_case(request):
    """G = 8, flow uniform +-0.05, 3 documents of random bytes; the batched bicubic tail and, per document, the grid of
    ops.unwarp_grid and the f32 drop-in result on the same image - computed once per size and shared."""
    h, w = request.param
    gen = torch.Generator().manual_seed(70 + h)
    flow = _rand((3, 2, 8, 8), 71 + h, -0.05, 0.05).cuda()
    src = torch.randint(0, 256, (3, h, w, 3), generator=gen, dtype=torch.uint8).cuda()
    got = ops.unwarp_u8_batch(flow, src, mode="bicubic")
    grids = [ops.unwarp_grid(flow[d:d + 1].contiguous(), h, w) for d in range(3)]
    f32 = [ops.grid_sample(src[d].permute(2, 0, 1)[None].float().contiguous(), grids[d], mode="bicubic") for d in range(3)]
    return flow, src, got, grids, f32


def test_u8_tail_equals_the_clamped_f32_kernel(tail_case):
    """Byte for byte: the tail's grid is dvd_unwarp_grid's and its sum is the drop-in kernel's device function."""
    flow, src, got, grids, f32 = tail_case
    for d in range(3):
        want = f32[d].clamp(0, 255).to(torch.uint8)[0].permute(1, 2, 0)
        assert torch.equal(got[d], want), d


def test_u8_tail_against_the_model(tail_case):
    """Where the model value is at least one bound away from the nearest integer the byte is floor(clip(model)); elsewhere
    it may differ by 1.  The left-out share stays below 5 % (about 0.5 % for K = 20 on random bytes), and both clamps are
    hit: random bytes make bicubic overshoot 0 and 255."""
    flow, src, got, grids, f32 = tail_case
    left_out = total = 0
    low = high = 0
    for d in range(3):
        srcf = src[d].permute(2, 0, 1)[None].float().cpu()
        model, s_abs = BM.bicubic_model(srcf.numpy(), grids[d].cpu().numpy())
        want = np.floor(np.clip(model, 0.0, 255.0)).astype(np.int64)[0].transpose(1, 2, 0)
        have = got[d].cpu().numpy().astype(np.int64)
        sure = (np.abs(model - np.rint(model)) >= BM.bound(s_abs))[0].transpose(1, 2, 0)
        assert np.array_equal(have[sure], want[sure]), d
        assert np.abs(have - want).max() <= 1, d
        left_out += int((~sure).sum())
        total += sure.size
        m = model[0].transpose(1, 2, 0)
        low += int(((m < -1.0) & (have == 0)).sum())
        high += int(((m > 256.0) & (have == 255)).sum())
        assert np.all(have[m < -1.0] == 0) and np.all(have[m > 256.0] == 255)
    print(f"u8 tail: {left_out} of {total} values within a bound of an integer ({100.0 * left_out / total:.2f} %); "
          f"{low} clamped at 0, {high} at 255")
    assert left_out <= 0.05 * total
    assert low > 0 and high > 0


def test_ragged_tail_and_the_bilinear_default():
    """ops.unwarp_u8_ragged(mode='bicubic') on 45 x 38, 160 x 100 and 64 x 64 equals the three ops.unwarp_u8(mode='bicubic')
    calls; and mode='bilinear' of all four functions equals the call without mode."""
    sizes = TAIL_SIZES + [(64, 64)]
    gen = torch.Generator().manual_seed(80)
    flow = _rand((3, 2, 8, 8), 81, -0.05, 0.05).cuda()
    srcs = [torch.randint(0, 256, (h, w, 3), generator=gen, dtype=torch.uint8).cuda() for h, w in sizes]
    ragged = ops.unwarp_u8_ragged(flow, srcs, mode="bicubic")
    for d, s in enumerate(srcs):
        one = ops.unwarp_u8(flow[d:d + 1].contiguous(), s, mode="bicubic")
        assert torch.equal(ragged[d], one), sizes[d]
        assert not torch.equal(one, ops.unwarp_u8(flow[d:d + 1].contiguous(), s)), sizes[d]
        assert torch.equal(ops.unwarp_u8(flow[d:d + 1].contiguous(), s, mode="bilinear"), ops.unwarp_u8(flow[d:d + 1].contiguous(), s))
    for a, b in zip(ops.unwarp_u8_ragged(flow, srcs, mode="bilinear"), ops.unwarp_u8_ragged(flow, srcs)):
        assert torch.equal(a, b)
    same = torch.stack([srcs[2]] * 3)
    assert torch.equal(ops.unwarp_u8_batch(flow, same, mode="bilinear"), ops.unwarp_u8_batch(flow, same))
    feat, grid = _rand((1, 3, 16, 16), 82).cuda(), _rand((1, 2, 16, 16), 83, -1.0, 1.0).cuda()
    assert torch.equal(ops.grid_sample(feat, grid, mode="bilinear"), ops.grid_sample(feat, grid))


def test_u8_tail_direct_gather_route():
    """A G = 8 flow of +-0.5 on 160 x 100 and 70 x 130 documents: between two flow nodes the sampling position moves by up
    to the whole page, so most 32 x 32 tiles' byte footprints exceed the 2048 staged dwords (or 64 dwords a row) and take
    the direct byte gather of unwarp_u8_bicubic_tile - asserted from the kernel's box arithmetic on ops.unwarp_grid's grid
    (bicubic_model.u8_tiles_staged).  Batched and ragged launches both equal clamp(ops.grid_sample(mode='bicubic')) on that
    grid byte for byte, as the staged route does in test_u8_tail_equals_the_clamped_f32_kernel."""
    gen = torch.Generator().manual_seed(85)
    for h, w in [(160, 100), (70, 130)]:
        flow = _rand((2, 2, 8, 8), 86 + h, -0.5, 0.5).cuda()
        src = torch.randint(0, 256, (2, h, w, 3), generator=gen, dtype=torch.uint8).cuda()
        batched = ops.unwarp_u8_batch(flow, src, mode="bicubic")
        ragged = ops.unwarp_u8_ragged(flow, [src[0], src[1]], mode="bicubic")
        direct = 0
        for d in range(2):
            grid = ops.unwarp_grid(flow[d:d + 1].contiguous(), h, w)
            routes = BM.u8_tiles_staged(grid[0].cpu().numpy(), h, w)
            direct += routes.count(False)
            f32 = ops.grid_sample(src[d].permute(2, 0, 1)[None].float().contiguous(), grid, mode="bicubic")
            want = f32.clamp(0, 255).to(torch.uint8)[0].permute(1, 2, 0)
            assert torch.equal(batched[d], want), (h, w, d)
            assert torch.equal(ragged[d], want), (h, w, d)
        print(f"u8 direct gather {h}x{w}: {direct} tiles on the direct route")
        assert direct >= 2, (h, w)


def test_u8_tail_cases_stage(tail_case):
    """The +-0.05 cases above are the STAGED route: every tile's footprint fits (the same box arithmetic)."""
    flow, src, got, grids, f32 = tail_case
    h, w = src.shape[1:3]
    for g in grids:
        assert all(BM.u8_tiles_staged(g[0].cpu().numpy(), h, w))


def test_run_evaluation_docunet_bicubic_float_source(tmp_path, monkeypatch):
    """The third route: a document that carries only a float `source_vis` which is not a byte image.  With
    env.unwarp_mode = 'bicubic' its page is clamp(ops.grid_sample(source, ops.unwarp_grid(flow), mode='bicubic'), 0, 255)
    as uint8 (NaN -> 0); with the default it is the fused f32 tail, truncated.  The tail alone is compared: the sampler is
    replaced by a fixed flow."""
    import admin.settings as ws
    import dvd_amd.evaluation as ev
    from dvd_amd import logger, synth
    monkeypatch.chdir(tmp_path)
    G, (h, w) = 16, (44, 36)
    flow = _rand((1, 2, G, G), 95, -0.05, 0.05).cuda()
    monkeypatch.setattr(ev, "run_sample_lr_dewarping", lambda *a, **k: flow.clone())
    s = ws.Settings()
    s.name, s.env.grid_size, s.env.batch_docs = "pytest_bicubic", G, 1
    s.env.visualize, s.env.eval_dataset_name = False, "docunet"
    vis = _rand((3, h, w), 96, 0.0, 255.0)                  # not integers: no byte image can be made of it
    doc = dict(synth.synth_document(0, G, 1234), path="doc_0", source_vis=vis)
    doc.pop("src_u8", None)
    model = torch.nn.Linear(1, 1).cuda()
    s.env.unwarp_mode = "bicubic"
    (_, cubic), = ev.run_evaluation_docunet(s, logger, [dict(doc)], None, model, None, None, None)
    s.env.unwarp_mode = "bilinear"
    (_, linear), = ev.run_evaluation_docunet(s, logger, [dict(doc)], None, model, None, None, None)
    srcf = vis[None].cuda().contiguous()
    want = ops.grid_sample(srcf, ops.unwarp_grid(flow, h, w), mode="bicubic")[0].clamp(0, 255).to(torch.uint8).permute(1, 2, 0)
    assert cubic.dtype == torch.uint8 and tuple(cubic.shape) == (h, w, 3) and torch.equal(cubic, want)
    assert torch.equal(linear, ops.unwarp_f32(flow, srcf).to(torch.uint8)) and not torch.equal(linear, cubic)


def test_run_evaluation_docunet_unwarp_mode(tmp_path, monkeypatch):
    """run_evaluation_docunet on two synthetic documents of different sizes (G = 16, batch_docs = 2).  Only the TAIL is
    compared: the sampler (run_sample_lr_dewarping) is replaced by a fixed flow, so every run unwarps the same flow.
    env.unwarp_mode = 'bicubic' gives ops.unwarp_u8_ragged(flow, ..., mode='bicubic'); the default gives the bilinear
    bytes, and so does an env without the attribute."""
    import admin.settings as ws
    import dvd_amd.evaluation as ev
    from dvd_amd import logger, synth
    monkeypatch.chdir(tmp_path)
    G, sizes = 16, [(72, 56), (50, 90)]
    flow = _rand((2, 2, G, G), 90, -0.05, 0.05).cuda()
    monkeypatch.setattr(ev, "run_sample_lr_dewarping", lambda *a, **k: flow.clone())
    s = ws.Settings()
    s.name, s.env.grid_size, s.env.batch_docs = "pytest_bicubic", G, 2
    s.env.visualize, s.env.eval_dataset_name = False, "docunet"
    model = torch.nn.Linear(1, 1).cuda()

    def docs():
        out = []
        for i, hw in enumerate(sizes):
            d = dict(synth.synth_document(i, G, 1234, full_res=hw))
            d["path"] = f"doc_{i}"
            out.append(d)
        return out

    def run():
        return [o for _, o in ev.run_evaluation_docunet(s, logger, docs(), None, model, None, None, None)]
    srcs = [torch.from_numpy(d["src_u8"]).cuda() for d in docs()]
    assert s.env.unwarp_mode == "bilinear"
    default = run()
    s.env.unwarp_mode = "bicubic"
    cubic = run()
    del s.env.unwarp_mode
    absent = run()
    for a, b, c, w_lin, w_cub in zip(default, absent, cubic, ops.unwarp_u8_ragged(flow, srcs),
                                     ops.unwarp_u8_ragged(flow, srcs, mode="bicubic")):
        assert torch.equal(a, b) and torch.equal(a, w_lin)
        assert torch.equal(c, w_cub) and not torch.equal(c, a)
