"""GPU tests of the GeoTr init-flow prior (env.use_init_flow): its new kernels against float64 torch, each stage against the
real reference's outputs (tests/tools/gen_geotr_golden.py), batch invariance, and the sampling chain it feeds."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from dvd_amd import lib, prestage, synth

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
SEED_MSK, SEED_GEOTR, G = 11, 31, 64


def _t(sd):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}


def _dewarp():
    m = prestage.GeoTr_Seg_Inf()
    m.msk.load_state_dict(_t(synth.synth_convnet_state_dict("u2netp", SEED_MSK)), strict=True)
    m.GeoTr.load_state_dict(_t(synth.synth_geotr_state_dict(SEED_GEOTR)), strict=True)
    return m.to("cuda").eval()


def _source_288(docs):
    y = torch.stack([torch.from_numpy(synth.synth_document(d, G, 1234)["y512"]) for d in docs]).cuda()
    return prestage.resize_bilinear(y, 288, True)


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


def test_attention_hd32_vs_float64():
    n, t, heads = 2, 1296, 8
    g = torch.Generator().manual_seed(0)
    q, k, v = (torch.randn(n, t, heads * 32, generator=g) for _ in range(3))
    vt = v.reshape(n, t, heads * 32).transpose(1, 2).contiguous()
    out = torch.empty(n, t, heads * 32, device="cuda")
    d = lib.AttnDesc()
    d.head_dim, d.heads, d.batch, d.tq, d.tk, d.kv_batch_div = 32, heads, n, t, t, 1
    qc, kc, vc = q.cuda(), k.cuda(), vt.cuda()
    d.Q, d.ldq, d.strideQ = qc.data_ptr(), 256, t * 256
    d.K, d.ldk, d.strideK = kc.data_ptr(), 256, t * 256
    d.Vt, d.ldvt, d.strideVt = vc.data_ptr(), t, 256 * t
    d.O, d.ldo, d.strideO = out.data_ptr(), 256, t * 256
    d.scale = float(np.float32(32 ** -0.5))
    import ctypes as C
    lib.call("dvd_flash_attn_f32", C.byref(d), lib.stream_ptr())
    qh = q.double().reshape(n, t, heads, 32).transpose(1, 2) * 32 ** -0.5
    kh = k.double().reshape(n, t, heads, 32).transpose(1, 2)
    vh = v.double().reshape(n, t, heads, 32).transpose(1, 2)
    want = (torch.softmax(qh @ kh.transpose(-1, -2), -1) @ vh).transpose(1, 2).reshape(n, t, 256)
    err = float((out.cpu().double() - want).abs().max())
    print(f"attention hd32 f32 vs float64: max abs {err:.2e}")
    assert err < 2.5e-6, err           # measured 7.0e-7 (x3)
    assert lib.flash_attn_kernel_name(32, 1296, 1296) == "flash_attn_f32_hd32_kernel"


def _call(name, *args):
    lib.call(name, *args, lib.stream_ptr())
    torch.cuda.synchronize()


@pytest.mark.parametrize("rows", [1, 3, 4, 5, 1297])
def test_layernorm256_vs_float64(rows):
    """One wave per row, four rows per workgroup: rows below, at and past a workgroup, and a ragged last one."""
    import ctypes as C
    x = torch.from_numpy(synth.normalish(f"geotr/ln/x{rows}", (rows, 256), 3)) * 2.0 + 0.5
    gamma = torch.from_numpy(synth.uniform("geotr/ln/g", (256,), 0.5, 1.5, 3))
    beta = torch.from_numpy(synth.uniform("geotr/ln/b", (256,), -0.5, 0.5, 3))
    out = torch.full((rows + 1, 256), 7.0, device="cuda")
    xd, gd, bd = x.cuda(), gamma.cuda(), beta.cuda()
    _call("dvd_layernorm256_f32", lib.ptr(xd), lib.ptr(out), rows, lib.ptr(gd), lib.ptr(bd), C.c_float(1e-5))
    want = F.layer_norm(x.double(), (256,), gamma.double(), beta.double(), 1e-5)
    err = float((out[:rows].cpu().double() - want).abs().max() / want.abs().max())
    print(f"layernorm256 rows {rows}: max abs / max |want| {err:.2e}")
    assert err <= 2e-6, err
    assert bool((out[rows] == 7.0).all()), "wrote past the last row"


@pytest.mark.parametrize("c", [4, 256])
def test_add_rows_ragged_position_table(c):
    rows, pos_rows = 7, 3                            # rows % pos_rows != 0: the table wraps and the last pass is cut short
    a = torch.from_numpy(synth.normalish(f"geotr/addrows/a{c}", (rows, c), 3))
    pos = torch.from_numpy(synth.normalish(f"geotr/addrows/p{c}", (pos_rows, c), 3))
    out = torch.full((rows + 1, c), 7.0, device="cuda")
    ad, pd = a.cuda(), pos.cuda()
    _call("dvd_add_rows_f32", lib.ptr(ad), lib.ptr(pd), lib.ptr(out), rows, pos_rows, c)
    assert torch.equal(out[:rows].cpu(), a + pos[torch.arange(rows) % pos_rows])
    assert bool((out[rows] == 7.0).all())


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("rows,cols", [(33, 31), (1, 70), (1296, 256)])
def test_transpose(n, rows, cols):
    x = torch.from_numpy(synth.normalish(f"geotr/tr/{rows}x{cols}", (n, rows, cols), 3))
    out = torch.full((n * rows * cols + 64,), 7.0, device="cuda")
    xd = x.cuda()
    _call("dvd_transpose_f32", lib.ptr(xd), lib.ptr(out), n, rows, cols)
    assert torch.equal(out[:n * rows * cols].cpu().reshape(n, cols, rows), x.transpose(1, 2))
    assert bool((out[n * rows * cols:] == 7.0).all())


@pytest.mark.parametrize("hw", [1, 255, 257])
@pytest.mark.parametrize("c", [1, 3])
def test_soft_mask_mul(hw, c):
    n = 2
    msk = torch.from_numpy(synth.uniform(f"geotr/smm/m{hw}", (n, 1, 1, hw), 0, 1, 3))
    x = torch.from_numpy(synth.normalish(f"geotr/smm/x{hw}/{c}", (n, c, 1, hw), 3))
    got = prestage.soft_mask_mul(msk.cuda(), x.cuda())
    assert torch.equal(got.cpu(), msk * x)


def _convex_upsample_float64(mask, dflow):
    """GeoTr.upsample_flow(coords1 - coords0, 0.25 * mask) in float64 (RAFT's convex upsampling): softmax over the 9 taps, the
    zero-padded 3x3 unfold of 8 * flow with flow = (coords0 + dflow) - coords0, summed over the taps."""
    n, _, h, w = dflow.shape
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float64), torch.arange(w, dtype=torch.float64), indexing="ij")
    coords0 = torch.stack((xs, ys))[None]
    flow = (coords0 + dflow.double()) - coords0
    m = torch.softmax((0.25 * mask.double()).view(n, 1, 9, 8, 8, h, w), dim=2)
    up = F.unfold(8 * flow, [3, 3], padding=1).view(n, 2, 9, 1, 1, h, w)
    return torch.sum(m * up, dim=2).permute(0, 1, 4, 2, 5, 3).reshape(n, 2, 8 * h, 8 * w)


@pytest.mark.parametrize("h,w", [(3, 5), (4, 4)])
def test_convex_upsample_vs_float64(h, w):
    """Maps so small that every coarse pixel touches a border (zero-padded taps everywhere), two documents.

    bm is checked on a rough field (large random flows, sharp random tap weights) and on a gentle one; init_flow on the
    gentle one only, because its bar of 5e-7 presumes a map as smooth as a real backward map: the kernel forms the source
    position as ATen does, scale * index in f32, which is off the exact position by up to 2 * 2^-24 * (8 max(h, w) - 1)
    fine pixels per axis, and that offset times the slope of bm / norm per fine pixel is a difference from the float64
    reference no kernel following ATen can avoid.  The test asserts on its OWN reference field that this term stays below
    1e-7 (a fifth of the bar); on the rough field the term may reach 4.5e-6."""
    import ctypes as C
    n, norm = 2, float(8 * max(h, w) - 1)
    for kind, mask_scale, amp in (("rough", 4.0, 0.5 * max(h, w)), ("gentle", 1.0, 0.1)):
        mask = torch.from_numpy(synth.normalish(f"geotr/cu/m{h}x{w}", (n, 576, h, w), 3)) * mask_scale
        dflow = torch.from_numpy(synth.uniform(f"geotr/cu/f{h}x{w}", (n, 2, h, w), -amp, amp, 3))
        want = _convex_upsample_float64(mask, dflow)
        md, fd = mask.cuda(), dflow.cuda()
        v = want / norm
        slope = float((v[..., 1:] - v[..., :-1]).abs().max()) + float((v[..., 1:, :] - v[..., :-1, :]).abs().max())
        index_term = slope * 2.0 ** -23 * norm
        if kind == "gentle":
            assert index_term <= 1e-7, index_term           # about the test's data, not about the kernel
        for g in (7, 16):
            bm = torch.empty(n, 2, 8 * h, 8 * w, device="cuda")
            init = torch.empty(n, 2, g, g, device="cuda")
            _call("dvd_convex_upsample", lib.ptr(md), lib.ptr(fd), n, h, w, lib.ptr(bm), lib.ptr(init), g, C.c_float(norm))
            e_bm = float((bm.cpu().double() - want).abs().max())
            want_init = F.interpolate(v, size=(g, g), mode="bilinear", align_corners=True)
            e_if = float((init.cpu().double() - want_init).abs().max())
            print(f"convex upsample {h}x{w} {kind} g {g}: bm max abs {e_bm:.2e} px, init_flow max abs {e_if:.2e} "
                  f"(source-position term of the reference field <= {index_term:.1e})")
            assert e_bm <= 1.5e-4, e_bm
            assert e_if <= 5e-7 + (0.0 if kind == "gentle" else index_term), e_if
            # init_flow alone (bm not requested) is the same kernel on the same values
            init2 = torch.empty_like(init)
            _call("dvd_convex_upsample", lib.ptr(md), lib.ptr(fd), n, h, w, None, lib.ptr(init2), g, C.c_float(norm))
            assert torch.equal(init2, init)


def test_strided_conv_instnorm_residual_vs_torch():
    """The executor's new ops on a small net: 7x7/2 conv, InstanceNorm + ReLU, 3x3/2 conv, 1x1/2 conv, relu(a + b)."""
    P = prestage.Program(3)
    a = P.instnorm(P.conv(0, 24, ("plain", "c1.weight", "c1.bias"), 7, 1, 0, stride=2), True)
    b = P.instnorm(P.conv(a, 32, ("plain", "c2.weight", "c2.bias"), 3, 1, 0, stride=2), True)
    c = P.instnorm(P.conv(a, 32, ("plain", "c3.weight", "c3.bias"), 1, 1, 0, stride=2), False)
    out = P.add(c, b, relu=True)
    shapes = {"c1": (24, 3, 7, 7), "c2": (32, 24, 3, 3), "c3": (32, 24, 1, 1)}
    sd = {}
    for name, shp in shapes.items():
        sd[name + ".weight"] = torch.from_numpy(synth.synth_tensor("t/" + name, shp, "w", 5))
        sd[name + ".bias"] = torch.from_numpy(synth.synth_tensor("t/" + name + "b", shp[:1], "b", 5))
    x = torch.from_numpy(synth.smooth_image("t/img", 50, 46, 3))[None].repeat(2, 1, 1, 1).contiguous()
    x[1] = x[1].flip(-1)
    net = prestage.ConvNet(P, [a, out], (50, 46), batch=2)
    net.load_state_dict(sd)
    got_a, got = net.run(x.cuda())
    inorm = lambda t: (t - t.mean((2, 3), keepdim=True)) / torch.sqrt(t.var((2, 3), unbiased=False, keepdim=True) + 1e-5)  # noqa: E731
    w = {k: v.double() for k, v in sd.items()}
    ra = torch.relu(inorm(F.conv2d(x.double(), w["c1.weight"], w["c1.bias"], stride=2, padding=3)))
    rb = torch.relu(inorm(F.conv2d(ra, w["c2.weight"], w["c2.bias"], stride=2, padding=1)))
    rc = inorm(F.conv2d(ra, w["c3.weight"], w["c3.bias"], stride=2))
    want = torch.relu(rb + rc)
    assert tuple(got.shape) == tuple(want.shape) == (2, 32, 13, 12)
    e1, e2 = _rel(got_a.cpu().double(), ra), _rel(got.cpu().double(), want)
    print(f"strided conv + instnorm: rel {e1:.2e} / {e2:.2e}")
    assert e1 < 2e-6 and e2 < 2e-6, (e1, e2)     # measured 5.8e-7 / 6.3e-7 (x3)


def test_geotr_stages_vs_reference_golden():
    g = np.load(os.path.join(GOLD, "geotr_stages.npz"))
    m = _dewarp()
    x = _source_288([0])
    msk = m.msk(x)[0]
    st = m.GeoTr.stages(prestage.soft_mask_mul(msk, x))
    bm, _ = m.GeoTr.upsample(st["dflow"], st["mask"], None, True)
    sub = int(g["sub"])
    errs = {"fnet": _rel(st["fnet"][0, ::16].cpu(), torch.from_numpy(g["fnet"])),
            "encoder": _rel(st["encoder"][0, ::16].cpu(), torch.from_numpy(g["encoder"])),
            "decoder": _rel(st["decoder"][0, ::16].cpu(), torch.from_numpy(g["decoder"])),
            "dflow": _rel(st["dflow"][0].cpu(), torch.from_numpy(g["dflow"])),
            "mask": _rel(0.25 * st["mask"][0, ::32].cpu(), torch.from_numpy(g["mask"]))}
    bm_err = float((bm[0, :, ::sub, ::sub].cpu() - torch.from_numpy(g["bm"])).abs().max())
    print("GeoTr stages vs reference (max abs / max |ref|):", {k: f"{v:.2e}" for k, v in errs.items()},
          f"bm max abs {bm_err:.2e} px")
    for k, v in errs.items():
        assert v < 1.5e-5, (k, v)        # measured 1.7e-6 .. 4.5e-6 (x3)
    assert bm_err < 1.5e-4, bm_err        # pixels, measured 4.2e-5 (x3); init_flow = bm / 287


def test_bm_and_init_flow_two_documents_vs_golden():
    g = np.load(os.path.join(GOLD, "geotr_docs.npz"))
    m = _dewarp()
    bm, _, init = m.mask_and_init_flow(_source_288([0, 1]), G, want_bm=True)
    sub = int(g["sub"])
    e_bm = float((bm[:, :, ::sub, ::sub].cpu() - torch.from_numpy(g["bm"])).abs().max())
    e_if = float((init.cpu() - torch.from_numpy(g["init_flow"])).abs().max())
    print(f"two documents: bm max abs {e_bm:.2e} px, init_flow max abs {e_if:.2e}")
    assert e_bm < 1.5e-4 and e_if < 5e-7, (e_bm, e_if)      # measured 4.2e-5 px / 1.4e-7 (x3)
    # forward() keeps the reference's return: (bm [N,2,288,288] in pixels, mask at 512)
    bm2, mask512 = m(_source_288([0, 1]))
    assert torch.equal(bm2, bm) and tuple(mask512.shape) == (2, 1, 512, 512)


def test_document_alone_equals_in_a_batch_of_8():
    m = _dewarp()
    docs = list(range(8))
    _, _, batch = m.mask_and_init_flow(_source_288(docs), G)
    for d in (0, 5):
        _, _, alone = m.mask_and_init_flow(_source_288([d]), G)
        assert torch.equal(alone[0], batch[d]), d


def test_sampling_chain_with_init_flow_vs_reference_golden():
    """The reference's chain (ddim_sample_loop, G = 64, S = 3, H = 2) fed with ITS GeoTr init_flow, against the HIP chain
    fed with the HIP GeoTr's init_flow from the same document: the coordinate error of the whole use_init_flow path."""
    from test_gpu_dropin import build
    g = np.load(os.path.join(GOLD, "geotr_chain_g64_s3.npz"))
    s, model, diffusion = build(64, 3)
    doc = {k: torch.from_numpy(v)[None].cuda() for k, v in synth.synth_document(0, 64, 1234).items()}
    init = prestage.init_flow(_dewarp(), doc["y512"], 64)
    e_init = float((init.cpu() - torch.from_numpy(g["init_flow"])).abs().max())
    kw = {"init_flow": init, "src_feat": None, "src_64": None, "y512": doc["y512"], "tmode": s.env.train_mode,
          "mask_cat": doc["mask_cat"], "init_feat": torch.zeros(1, 256, 64, 64, device="cuda"), "iter": True,
          "mask_y512": doc["mask_y512"], "line_msk": doc["line_msk"]}
    sample, _ = diffusion.ddim_sample_loop(model, (1, 2, 64, 64), noise=torch.from_numpy(g["x_T"]), clip_denoised=False,
                                           model_kwargs=kw, eta=0.0, progress=True, denoised_fn=None,
                                           sampling_kwargs={"src_img": doc["y512"]}, logger=None, n_batch=2,
                                           time_variant=True, pyramid=None)
    err = float(np.sqrt(((sample.cpu().numpy() - g["sample"]) ** 2).mean()))
    print(f"chain with init_flow: init_flow max abs {e_init:.2e}, coordinate RMSE {err:.2e}")
    assert e_init < 5e-7, e_init
    assert err < 2e-4, err                # measured 6.4e-5 (x3); north_star's bar: 1e-3


def test_flag_off_conditioning_never_builds_geotr():
    m = prestage.GeoTr_Seg_Inf()
    m.msk.load_state_dict(_t(synth.synth_convnet_state_dict("u2netp", SEED_MSK)), strict=True)
    m.to("cuda").eval()
    bm, mask512 = m(_source_288([0]))
    assert bm is None and tuple(mask512.shape) == (1, 1, 512, 512)
    assert "GeoTr" not in m._modules and m.live_geotr() is None


def test_plugin_run_with_use_init_flow(tmp_path, monkeypatch):
    """val_TDiff.run with env.use_init_flow (synthetic GeoTr weights): it runs, and the prior changes the result."""
    monkeypatch.chdir(tmp_path)
    import admin.settings as ws
    from dvd_amd import val_TDiff

    def settings(flag):
        s = ws.Settings()
        s.env.grid_size, s.env.diffusion_steps = 16, 3
        s.env.num_synthetic_docs, s.env.batch_docs, s.env.full_res = 2, 2, (96, 80)
        s.env.visualize = False
        s.env.use_init_flow = flag
        s.name, s.seed, s.severity, s.corruption_number = "pytest", 0, 0, 0
        return s
    torch.manual_seed(0)
    on = val_TDiff.run(settings(True))
    torch.manual_seed(0)
    off = val_TDiff.run(settings(False))
    assert len(on) == len(off) == 2
    assert any(not torch.equal(a[1], b[1]) for a, b in zip(on, off))
