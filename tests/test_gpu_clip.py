"""GPU tests of clip_denoised / denoised_fn / iter=False: the fused clip export against torch on the CPU bit for bit, the
three reference chains of tests/tools/gen_clip_golden.py through the diffusion object, the single-step calls with their
default arguments, and env.clip_denoised through val_TDiff.run.

Loop bars.  The project's rule is RMSE measured on the MI355X x 3, never above north_star's 1e-3.  The four chains have
NOT been measured on the MI355X yet; every test prints its per-step and final figures before it asserts.  Until they are
in, clip_fixtures.LOOP_BAR is the un-clipped loop goldens' bar, 2.7e-4 (measured 6.5e-5 .. 9.0e-5, x 3), by reasoning and
not by what this code gives: the clamp is 1-Lipschitz, so a clipped chain should not err more than the un-clipped chain
of the same length; a no-feedback chain has no compounding at all."""
import numpy as np
import pytest
import torch

import clip_fixtures as CF
from dvd_amd import synth

pytestmark = pytest.mark.gpu


def build(grid, steps):
    import admin.settings as ws
    from dvd_amd.script_util import args_to_dict, create_model_and_diffusion, model_and_diffusion_defaults
    s = ws.Settings()
    s.env.grid_size, s.env.diffusion_steps = grid, steps
    s.name = "pytest"
    model, diffusion = create_model_and_diffusion(device="cuda", train_mode=s.env.train_mode, tv=s.env.time_variant,
                                                  grid_size=grid, **args_to_dict(s, model_and_diffusion_defaults().keys()))
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in synth.synth_state_dict(grid, 7).items()}
    model.cpu().load_state_dict(sd, strict=False)
    model.to("cuda")
    model.eval()
    return s, model, diffusion


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _torch_step(c, x_t, x0, noise, G):
    """The step on the CPU with torch's separately rounded tensor ops in the reference's operation order
    (idf/gaussian_diffusion.py:384,434-438,480-489 / :270-292,:622) on the kernel's float32 coefficients."""
    f = lambda v: torch.tensor([v], dtype=torch.float32)  # noqa: E731
    p0 = x0.clamp(-1, 1)
    if c.kind == 0:
        eps = (f(c.c_recip) * x_t - p0) / f(c.c_recipm1)
        mean = p0 * f(c.sqrt_abar_prev) + f(c.dir_coef) * eps
    else:
        mean = f(c.coef1) * p0 + f(c.coef2) * x_t
    x_prev = mean + f(c.sigma) * (noise if noise is not None else torch.zeros_like(x_t))
    ar = torch.arange(G, dtype=torch.float32) / torch.tensor(float(G - 1))
    base = torch.stack([ar[None, :].expand(G, G), ar[:, None].expand(G, G)])[None]
    return p0, x_prev, (p0 + base) * 2 - 1


@pytest.mark.parametrize("kind", ["ddim_eta0", "ddim_eta05", "ddpm"])
def test_sched_step_clip_is_torch_bit_for_bit(kind):
    from dvd_amd import ops, schedule
    G, N = 24, 3
    x_t = torch.from_numpy(synth.normalish("clipk/x", (N, 2, G, G), 5))
    x0 = torch.from_numpy(synth.uniform("clipk/x0", (N, 2, G, G), -3.0, 3.0, 5))
    one = np.float32(1)
    x0.view(-1)[:8] = torch.tensor([1.0, -1.0, 0.0, -0.0, float(np.nextafter(one, np.float32(2))),
                                    float(np.nextafter(-one, np.float32(-2))), float(np.nextafter(one, np.float32(0))), -3.0])
    nz = torch.from_numpy(synth.normalish("clipk/n", (N, 2, G, G), 5))
    tab = schedule.Tables(schedule.named_betas("cosine", 10))
    for i in (9, 5, 1, 0):
        c = {"ddim_eta0": lambda: tab.ddim_coef(i, 0.0), "ddim_eta05": lambda: tab.ddim_coef(i, 0.5),
             "ddpm": lambda: tab.ddpm_coef(i)}[kind]()
        noise = nz if c.sigma != 0.0 else None
        x0_dev = x0.cuda()
        out, grid = ops.sched_step(c, x_t.cuda(), x0_dev, None if noise is None else noise.cuda(), want_grid=True, clip=True)
        p0, x_prev, ngrid = _torch_step(c, x_t, x0, noise, G)
        assert torch.equal(_bits(x0_dev), _bits(p0)), (kind, i, "x0 in place")          # bit views: -0 stays -0
        assert torch.equal(_bits(out), _bits(x_prev)), (kind, i, "x_prev")
        assert torch.equal(_bits(grid), _bits(ngrid)), (kind, i, "next_grid")
        assert float(x0_dev.abs().max()) == 1.0
        # on inputs that are in range already the plain export gives the same bits (and leaves x0 alone)
        in_range = p0.cuda()
        keep = in_range.clone()
        out2, grid2 = ops.sched_step(c, x_t.cuda(), in_range, None if noise is None else noise.cuda(), want_grid=True)
        assert torch.equal(_bits(out2), _bits(out)) and torch.equal(_bits(grid2), _bits(grid))
        assert torch.equal(_bits(in_range), _bits(keep))


def test_sched_step_clip_keeps_nan_and_checks_its_arguments():
    from dvd_amd import lib, ops, schedule
    tab = schedule.Tables(schedule.named_betas("cosine", 10))
    x0 = torch.tensor([float("nan"), 2.0, -2.0, 0.5] * 8).view(1, 2, 4, 4).cuda()
    want = _bits(x0.cpu().clamp(-1, 1))
    out = ops.sched_step(tab.ddim_coef(5), torch.zeros(1, 2, 4, 4, device="cuda"), x0, clip=True)
    assert torch.equal(_bits(x0), want)                          # torch.clamp passes the NaN through, payload and all
    assert bool(torch.isnan(out).view(-1)[0::4].all()) and not bool(torch.isnan(out).view(-1)[1::4].any())
    c = tab.ddpm_coef(5)
    with pytest.raises(lib.DvdError, match="noise"):
        ops.sched_step(c, torch.zeros(1, 2, 4, 4, device="cuda"), x0, clip=True)
    with pytest.raises(lib.DvdError, match="in place"):
        ops.sched_step(tab.ddim_coef(5), x0, x0, clip=True)
    c.kind = 7
    with pytest.raises(lib.DvdError, match="kind"):
        ops.sched_step(c, torch.zeros(1, 2, 4, 4, device="cuda"), x0, torch.zeros(1, 2, 4, 4, device="cuda"), clip=True)


def _doc_kwargs(s, grid, init_flow, iterate=True):
    """model_kwargs as run_sample_lr_dewarping builds them (dvd_amd/evaluation.py; reference evaluation.py:121-135)."""
    doc = {k: torch.from_numpy(v)[None].cuda() for k, v in synth.synth_document(0, grid, 1234).items()}
    kw = {"init_flow": init_flow.cuda(), "src_feat": None, "src_64": None, "y512": doc["y512"], "tmode": s.env.train_mode,
          "mask_cat": doc["mask_cat"], "init_feat": torch.zeros(1, 256, grid, grid, device="cuda"), "iter": iterate,
          "mask_y512": doc["mask_y512"], "line_msk": doc["line_msk"]}
    return doc, kw


def _traced(monkeypatch):
    """Record the roll-out's per-step processed x0 (sampler.sample's `trace`) of calls made through the diffusion object."""
    from dvd_amd import sampler
    trace, real = [], sampler.sample

    def spy(*a, **k):
        del trace[:]
        return real(*a, trace=trace, **k)
    monkeypatch.setattr(sampler, "sample", spy)
    return trace


def _check_steps(tag, g, trace, sample, ref_sample):
    ref = CF.processed(g)
    per_step = [CF.rmse(trace[k][:1].cpu().numpy(), ref[k]) for k in range(len(trace))]
    err = CF.rmse(sample.cpu().numpy(), ref_sample)
    print(f"{tag}: per-step processed x0 rmse (hypothesis 0) {['%.2e' % e for e in per_step]}  sample rmse {err:.3e}")
    assert len(trace) == int(g["steps"])
    assert max(per_step) < CF.LOOP_BAR, (tag, per_step)
    assert err < CF.LOOP_BAR, (tag, err)


@pytest.mark.parametrize("tag", ["clip", "noiter"])
def test_ddim_sample_loop_vs_reference_chain(tag, monkeypatch):
    """ddim_sample_loop called as run_sample_lr_dewarping calls it (explicit noise = the fixture's x_T), with
    clip_denoised=True / model_kwargs['iter']=False, against the real reference's 10-step chain at G = 64."""
    g = CF.load(tag)
    s, model, diffusion = build(64, 10)
    doc, kw = _doc_kwargs(s, 64, torch.from_numpy(g["init_flow"]), iterate=bool(g["iter"]))
    trace = _traced(monkeypatch)
    sample, final = diffusion.ddim_sample_loop(model, (1, 2, 64, 64), noise=torch.from_numpy(g["x_T"]),
                                               clip_denoised=bool(g["clip_denoised"]), model_kwargs=kw, eta=0.0, progress=True,
                                               denoised_fn=None, sampling_kwargs={"src_img": doc["y512"]}, logger=None,
                                               n_batch=2, time_variant=True, pyramid=None)
    assert tuple(sample.shape) == (1, 2, 64, 64) and set(final) == {"sample", "pred_xstart", "feat_dict"}
    if tag == "clip":
        assert all(float(t.abs().max()) <= 1.0 for t in trace)
    _check_steps(tag, g, trace, sample, g["sample"])
    # and the flag matters: the reference's result with the flag at its other value is far outside the bar
    other = CF.load("loop_g64_s10.npz")["sample"] if tag == "clip" else g["sample_iter"]
    assert CF.rmse(sample.cpu().numpy(), other) > 5 * CF.LOOP_BAR


def test_no_feedback_with_the_callers_init_feat_vs_reference_chain(monkeypatch):
    """iter = False with a NON-ZERO init_feat (feature mode 3 at every step, the engine's persistent feat0 buffer, two
    replayed graphs) at G = 32: the no-feedback branch never adds base64, so this is the reference's own
    ddim_sample_loop.  Then one step of the chain by hand: ddim_sample(model, x, t, model_kwargs={..., 'iter': False}) at
    t_model = 900, where with iter = True the model would swap in the pyramid features."""
    g = CF.load("noiterfeat")
    assert str(g["kind"]) == "ddim_sample_loop" and not bool(g["iter"])
    s, model, diffusion = build(32, 10)
    doc, kw = _doc_kwargs(s, 32, torch.from_numpy(g["init_flow"]), iterate=False)
    kw["init_feat"] = torch.from_numpy(CF.noiterfeat_init_feat()).cuda()
    trace = _traced(monkeypatch)
    for rep in range(2):                            # the second roll-out replays the captured evaluations
        sample, _ = diffusion.ddim_sample_loop(model, (1, 2, 32, 32), noise=torch.from_numpy(g["x_T"]),
                                               clip_denoised=bool(g["clip_denoised"]), model_kwargs=kw, eta=0.0,
                                               progress=True, denoised_fn=None, sampling_kwargs={"src_img": doc["y512"]},
                                               logger=None, n_batch=2, time_variant=True, pyramid=None)
        _check_steps(f"noiterfeat (roll-out {rep})", g, trace, sample, g["sample"])
    # a zero init_feat is another chain: the features are live
    kw0 = dict(kw, init_feat=torch.zeros(1, 256, 32, 32, device="cuda"))
    other, _ = diffusion.ddim_sample_loop(model, (1, 2, 32, 32), noise=torch.from_numpy(g["x_T"]), clip_denoised=True,
                                          model_kwargs=kw0, eta=0.0, n_batch=2, time_variant=True)
    assert CF.rmse(other.cpu().numpy(), g["sample"]) > 5 * CF.LOOP_BAR
    # one step by hand on hypothesis 0
    kw1 = {k: v for k, v in kw.items() if k not in ("src_feat", "src_64")}
    kw1.update(tv=True, mode=None)
    out = diffusion.ddim_sample(model, torch.from_numpy(g["x_in_steps"][0]).cuda(), torch.tensor([9], device="cuda"),
                                model_kwargs=kw1)
    e0 = CF.rmse(out["pred_xstart"].cpu().numpy(), CF.processed(g)[0])
    e1 = CF.rmse(out["sample"].cpu().numpy(), g["x_in_steps"][1])
    print(f"noiterfeat single step: pred_xstart rmse {e0:.3e}  sample rmse {e1:.3e}")
    assert e0 < 1.6e-4 and e1 < CF.LOOP_BAR       # one denoiser call: the bar of test_gpu_dropin's single-call tests


def test_denoised_fn_then_clamp_vs_reference_chain(monkeypatch):
    """denoised_fn = 0.9 x with clip_denoised=True at G = 32: the function first, the clamp second.  The reference chain is
    ddim_sample_loop_for_training(mode=None, timestep=-1) - its only loop whose warp base follows the grid size
    (idf/gaussian_diffusion.py:744-752; ddim_sample_loop adds base64 whatever the grid) - which clamps the per-hypothesis
    maps and takes no mean.  Checked through that call, and through ddim_sample_loop, whose result is then the
    hypothesis mean of the same maps."""
    g = CF.load("fn")
    assert str(g["kind"]) == "ddim_sample_loop_for_training"
    fn = CF.fn_of(g)
    s, model, diffusion = build(32, 10)
    doc, kw = _doc_kwargs(s, 32, torch.from_numpy(g["init_flow"]))
    trace = _traced(monkeypatch)
    kw2 = {k: v for k, v in kw.items() if k not in ("tmode", "iter")}
    calls = []
    sample, feat = diffusion.ddim_sample_loop_for_training(
        model, (1, 2, 32, 32), noise=torch.from_numpy(g["x_T"]), clip_denoised=True,
        denoised_fn=lambda x: calls.append(1) or fn(x), model_kwargs=kw2, eta=0.0, n_batch=2, time_variant=True, iter=True,
        mode=None, timestep=-1)
    assert len(calls) == 10 and tuple(sample.shape) == (2, 2, 32, 32)
    _check_steps("fn (training variant)", g, trace, sample, g["sample"])
    sample2, _ = diffusion.ddim_sample_loop(model, (1, 2, 32, 32), noise=torch.from_numpy(g["x_T"]), clip_denoised=True,
                                            model_kwargs=kw, eta=0.0, progress=True, denoised_fn=fn,
                                            sampling_kwargs={"src_img": doc["y512"]}, logger=None, n_batch=2,
                                            time_variant=True, pyramid=None)
    ref_mean = np.clip(g["sample"].mean(axis=0, keepdims=True), -1, 1)
    _check_steps("fn (ddim_sample_loop)", g, trace, sample2, ref_mean)


def test_single_step_defaults_vs_reference_golden():
    """p_mean_variance / ddim_sample with DEFAULT arguments (clip_denoised=True) on a model whose output spans [-3, 3]."""
    g = CF.load("single_step_clip.npz")
    x_t, raw = torch.from_numpy(g["x_t"]).cuda(), torch.from_numpy(g["x0_raw"]).cuda()
    keep = raw.clone()
    fake = lambda x, t, **kw: (raw, None)  # noqa: E731
    _, _, diffusion = build(16, 50)
    worst = 0.0
    for i in range(50):
        out = diffusion.ddim_sample(fake, x_t, torch.tensor([i, i], device="cuda"), model_kwargs={})
        assert np.array_equal(out["pred_xstart"].cpu().numpy(), g["pred_xstart"])
        assert float(out["pred_xstart"].abs().max()) <= 1.0
        err = CF.rmse(out["sample"].cpu().numpy(), g["ddim50/sample"][i])
        worst = max(worst, err)
        assert err < CF.SINGLE_STEP_BAR, (i, err)
    _, _, diffusion = build(16, 250)
    for i in range(0, 250, 7):
        out = diffusion.p_mean_variance(fake, x_t, torch.tensor([i, i], device="cuda"), model_kwargs={})
        assert set(out) == {"mean", "variance", "log_variance", "pred_xstart", "feat_dict"}
        assert np.array_equal(out["pred_xstart"].cpu().numpy(), g["pred_xstart"])
        err = CF.rmse(out["mean"].cpu().numpy(), g["ddpm250/mean"][i])
        worst = max(worst, err)
        assert err < CF.SINGLE_STEP_BAR, (i, err)
    print("single step with default arguments: worst rmse", worst)
    assert torch.equal(_bits(raw), _bits(keep)), "the caller's model output was clamped in place"


def _run_settings(name, grid, steps, docs, batch):
    import admin.settings as ws
    s = ws.Settings()
    s.env.grid_size, s.env.diffusion_steps = grid, steps
    s.env.num_synthetic_docs, s.env.batch_docs, s.env.full_res = docs, batch, (96, 80)
    s.env.visualize = False
    s.name, s.seed, s.severity, s.corruption_number = name, 0, 0, 0
    return s


def test_env_clip_denoised_through_the_plugin_run(tmp_path, monkeypatch):
    """env.clip_denoised = True through val_TDiff.run on two synthetic documents: the flow the run samples equals a
    direct ddim_sample_loop(clip_denoised=True) on the same inputs and the same x_T bit for bit, and differs from the
    un-clipped one."""
    monkeypatch.chdir(tmp_path)
    import dvd_amd.gaussian_diffusion as gd
    from dvd_amd import evaluation, val_TDiff
    s = _run_settings("pytest_clip", 16, 10, 2, 2)
    s.env.clip_denoised = True
    seen, draws = {}, []
    real_sampling, real_randn = evaluation.run_sample_lr_dewarping, torch.randn

    def spy_sampling(settings, logger, diffusion, model, radius, source, feature_size, raw_corr, init_flow, c20, source_64,
                     pyramid, doc_mask, seg_map_all=None, textline_map=None, init_feat=None):
        flow = real_sampling(settings, logger, diffusion, model, radius, source, feature_size, raw_corr, init_flow, c20,
                             source_64, pyramid, doc_mask, seg_map_all, textline_map, init_feat)
        seen.update(diffusion=diffusion, model=model, source=source, init_flow=init_flow, doc_mask=doc_mask, seg=seg_map_all,
                    line=textline_map, init_feat=init_feat, flow=flow.clone(), clip=settings.env.clip_denoised)
        return flow

    def spy_randn(*shape, **kw):
        out = real_randn(*shape, **kw)
        draws.append(out.clone())
        return out
    monkeypatch.setattr(evaluation, "run_sample_lr_dewarping", spy_sampling)
    monkeypatch.setattr(gd.th, "randn", spy_randn)
    results = val_TDiff.run(s)
    monkeypatch.setattr(gd.th, "randn", real_randn)
    assert len(results) == 2 and seen["clip"] is True
    H = s.env.n_batch
    shapes = [tuple(d.shape) for d in draws]
    assert (2, 2, 16, 16) in shapes                             # the discarded draw (:562) ...
    x_T = draws[shapes.index((2 * H, 2, 16, 16))]               # ... and x_T (:569)
    kw = {"init_flow": seen["init_flow"], "src_feat": None, "src_64": None, "y512": seen["source"], "tmode": s.env.train_mode,
          "mask_cat": seen["doc_mask"], "init_feat": seen["init_feat"], "iter": True, "mask_y512": seen["seg"],
          "line_msk": seen["line"]}
    direct = {}
    for clip in (True, False):
        out, _ = seen["diffusion"].ddim_sample_loop(seen["model"], (2, 2, 16, 16), noise=x_T, clip_denoised=clip,
                                                    model_kwargs=dict(kw), eta=0.0, n_batch=H, time_variant=True)
        direct[clip] = torch.clamp(out, -1, 1)
    assert torch.equal(_bits(seen["flow"]), _bits(direct[True]))
    assert not torch.equal(seen["flow"], direct[False])


def test_clipped_document_alone_equals_itself_in_a_batch_of_8():
    """Batch invariance with clipping on (G = 64): document 3 sampled alone and as one of 8 gives the same bits."""
    G, S, H = 64, 10, 2                     # 10 steps of the plain family: over half of the last x0 is out of range
    s, model, diffusion = build(G, S)
    docs = [synth.synth_document(d, G, 1234) for d in range(8)]
    keys = ("y512", "mask_cat", "mask_y512", "line_msk")
    x_T = torch.from_numpy(synth.synth_noise(0, 8 * H, G, 777)).cuda()

    def run(idx):
        b = len(idx)
        kw = {k: torch.from_numpy(np.stack([docs[d][k] for d in idx])).cuda() for k in keys}
        kw.update(init_flow=torch.zeros(b, 2, G, G, device="cuda"), init_feat=torch.zeros(b, 256, G, G, device="cuda"),
                  src_feat=None, src_64=None, tmode=s.env.train_mode, iter=True)
        rows = torch.cat([x_T[d * H:(d + 1) * H] for d in idx])
        out, _ = diffusion.ddim_sample_loop(model, (b, 2, G, G), noise=rows, clip_denoised=True, model_kwargs=kw, eta=0.0,
                                            n_batch=H, time_variant=True)
        return out
    batch = run(list(range(8)))
    alone = run([3])
    assert torch.equal(_bits(alone[0]), _bits(batch[3]))
