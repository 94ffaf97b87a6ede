"""CPU tests of clip_denoised / denoised_fn / iter=False: the reference fixtures are self-consistent with the oracle's
arithmetic and move the result far more than the GPU tests' bar, and the host loop - with the library's compute entry
points stubbed at lib.call - picks the clip export, keeps the flow fixed without feedback, and calls denoised_fn once
per step before the scheduler launch."""
import numpy as np
import pytest
import torch

import clip_fixtures as CF
from oracle import dvd_oracle as O


@pytest.mark.parametrize("tag", ["clip", "noiter", "fn", "noiterfeat"])
def test_fixture_chain_is_the_oracle_arithmetic_bit_for_bit(tag):
    """pred_xstart[k] == clamp(fn(raw[k])) and x_in[k+1] == oracle.ddim_step(x_in[k], pred_xstart[k]), bit for bit."""
    g = CF.load(tag)
    S = int(g["steps"])
    sch = O.Schedule(S)
    fn, clip = CF.fn_of(g), bool(g["clip_denoised"])
    x_in, raw, pred = g["x_in_steps"], g["raw_steps"], CF.processed(g)
    assert x_in.shape == raw.shape == pred.shape == (S, 1, 2, int(g["grid"]), int(g["grid"]))
    assert np.array_equal(x_in[0], g["x_T"][:1])
    for k in range(S):
        want = torch.from_numpy(raw[k])
        if fn is not None:
            want = fn(want)
        if clip:
            want = want.clamp(-1, 1)
        assert np.array_equal(want.numpy(), pred[k]), (tag, k)
        if k + 1 < S:
            nxt = O.ddim_step(sch, S - 1 - k, torch.from_numpy(x_in[k]), torch.from_numpy(pred[k]))
            assert np.array_equal(nxt.numpy(), x_in[k + 1]), (tag, k)
    if clip:
        assert float(np.abs(pred).max()) <= 1.0


def test_clipped_fixtures_bite():
    """The clamp changes at least 1 % of the elements of at least one step (recomputed from the stored raw output of
    hypothesis 0, and as the generator counted it over both hypotheses)."""
    for tag in ("clip", "fn"):
        g = CF.load(tag)
        assert float(g["clamp_share"].max()) >= 0.01, (tag, g["clamp_share"])
        fn = CF.fn_of(g)
        pre = g["raw_steps"] if fn is None else np.stack([fn(torch.from_numpy(r)).numpy() for r in g["raw_steps"]])
        share = (np.abs(pre) > 1).reshape(pre.shape[0], -1).mean(axis=1)
        assert float(share.max()) >= 0.01, (tag, share)
    # step 0 of the un-clipped chain is in range, so the clipped and the un-clipped chain share step 1's raw output
    a, b = CF.load("clip"), CF.load("loop_g64_s10.npz")
    assert np.array_equal(a["x_T"], b["x_T"])
    assert np.array_equal(a["raw_steps"][:2], b["x0_steps"][:2, :1])
    assert not np.array_equal(a["raw_steps"][2], b["x0_steps"][2, :1])


def test_fixtures_move_the_result_by_ten_bars():
    """A build that ignores clip_denoised or iter=False cannot pass the GPU tests: what each flag changes in the
    reference's own result is at least 10 x the bar those tests use."""
    clip, plain, noiter = CF.load("clip"), CF.load("loop_g64_s10.npz"), CF.load("noiter")
    d_clip = CF.rmse(clip["sample"], plain["sample"])
    d_iter = CF.rmse(noiter["sample"], noiter["sample_iter"])
    print("clip vs plain sample rmse", d_clip, " noiter vs iter sample rmse", d_iter)
    assert d_clip >= 10 * CF.LOOP_BAR and d_iter >= 10 * CF.LOOP_BAR
    # the function fixture pins the ORDER: clamp(0.9 x) differs from 0.9 clamp(x) wherever 1 < |x| < 1/0.9 ...
    g = CF.load("fn")
    raw = torch.from_numpy(g["raw_steps"])
    swapped = CF.fn_of(g)(raw.clamp(-1, 1)).numpy()
    per_step = [CF.rmse(swapped[k], g["pred_steps"][k]) for k in range(raw.shape[0])]
    assert max(per_step) >= 10 * CF.LOOP_BAR, per_step
    # ... and from no function at all
    assert max(CF.rmse(raw[k].clamp(-1, 1).numpy(), g["pred_steps"][k]) for k in range(raw.shape[0])) >= 10 * CF.LOOP_BAR
    assert float(np.abs(noiter["init_flow"]).max()) > 0.05 and not bool(noiter["iter"])


# ------------------------------------------------------------------------------------------------
# The host loop with the compute entry points stubbed at the lib.call boundary (no GPU here; the host-only entry points
# - create / workspace / set_option - run for real).
# ------------------------------------------------------------------------------------------------
COMPUTE = {"dvd_engine_prepare_docs", "dvd_engine_denoise_step", "dvd_engine_feat_nchw", "dvd_sched_step",
           "dvd_sched_step_clip", "dvd_hyp_mean_clamp"}


@pytest.fixture
def stubbed(monkeypatch):
    from dvd_amd import engine, lib, ops
    calls = []
    real_call = lib.call

    def call(name, *args):
        if name in COMPUTE:
            calls.append((name, args))
            return
        return real_call(name, *args)
    monkeypatch.setattr(lib, "call", call)
    for mod in (engine, ops):
        monkeypatch.setattr(mod, "stream_ptr", lambda: None)
    monkeypatch.setattr(ops, "_chk", lambda *a, **k: None)
    monkeypatch.setattr(engine, "_is_dev", lambda t: True)
    return calls


def _addr(c_void_p):
    return None if c_void_p is None else c_void_p.value


def _roll(calls, S=10, **kw):
    from dvd_amd import sampler, schedule
    from dvd_amd.engine import Engine
    eng = Engine(16, 1, 2, device="cpu")
    tab = schedule.Tables(schedule.named_betas("cosine", S))
    del calls[:]
    out = sampler.sample(eng, tab, torch.zeros(2, 2, 16, 16), **kw)
    return eng, out


def test_loop_passes_the_clip_export_at_every_step(stubbed):
    eng, _ = _roll(stubbed, clip_denoised=True)
    names = [n for n, _ in stubbed]
    assert names.count("dvd_sched_step_clip") == 10 and "dvd_sched_step" not in names
    # the buffer the scheduler clamps in place is the one the denoiser wrote and the next evaluation reads as its flow
    den = [a for n, a in stubbed if n == "dvd_engine_denoise_step"]
    sch = [a for n, a in stubbed if n == "dvd_sched_step_clip"]
    for k in range(10):
        assert _addr(sch[k][2]) == _addr(den[k][6])
        if k + 1 < 10:
            assert _addr(den[k + 1][4]) == _addr(den[k][6])
    # and with the flag off the plain export, as before
    _roll(stubbed)
    names = [n for n, _ in stubbed]
    assert names.count("dvd_sched_step") == 10 and "dvd_sched_step_clip" not in names


@pytest.mark.parametrize("feat", ["none", "zero", "given"])
def test_no_feedback_loop_hands_the_engine_one_flow_and_mode_0_or_3(stubbed, feat):
    init_feat = {"none": None, "zero": torch.zeros(2, 256, 16, 16), "given": torch.ones(2, 256, 16, 16)}[feat]
    eng, _ = _roll(stubbed, iterate=False, init_flow=torch.full((2, 2, 16, 16), 0.1), init_feat=init_feat)
    den = [a for n, a in stubbed if n == "dvd_engine_denoise_step"]
    assert len(den) == 10
    io = eng.io_buffers()
    assert {_addr(a[4]) for a in den} == {io["flow0"].data_ptr()}
    assert float(io["flow0"].min()) == float(io["flow0"].max()) == pytest.approx(0.1)
    assert {a[3] for a in den} == ({3} if feat == "given" else {0})
    if feat == "given":
        assert {_addr(a[5]) for a in den} == {eng.io_feat0().data_ptr()} and bool((eng.io_feat0() == 1).all())
    else:
        assert {_addr(a[5]) for a in den} == {None}
    # the evaluations a graph-replaying engine sees: two (x_t, flow, x0) address triples, whatever the step count
    assert len({(_addr(a[1]), _addr(a[4]), _addr(a[6])) for a in den}) == 2
    # with feedback (the default) the flow pointer moves and modes 1 / 2 appear
    _roll(stubbed)
    den = [a for n, a in stubbed if n == "dvd_engine_denoise_step"]
    assert len({_addr(a[4]) for a in den}) == 3 and {a[3] for a in den} == {1, 2}


def test_denoised_fn_runs_once_per_step_before_the_scheduler_call(stubbed):
    events = []

    def fn(x):
        events.append(("fn", len(stubbed)))
        return 0.5 * x
    trace = []
    eng, _ = _roll(stubbed, denoised_fn=fn, clip_denoised=True, trace=trace)
    assert len(events) == 10 and len(trace) == 10
    names = [n for n, _ in stubbed]
    for _, at in events:                       # called right after the step's denoiser call, before its scheduler call
        assert names[at - 1] == "dvd_engine_denoise_step" and names[at] == "dvd_sched_step_clip"


def test_single_step_calls_with_default_arguments_no_longer_raise(stubbed):
    from dvd_amd import gaussian_diffusion as gd
    diff = gd.GaussianDiffusion(betas=gd.get_named_beta_schedule("cosine", 10), model_mean_type=gd.ModelMeanType.START_X,
                                model_var_type=gd.ModelVarType.FIXED_LARGE, loss_type=gd.LossType.MSE,
                                rescale_timesteps=True)
    kept = torch.full((2, 2, 16, 16), 2.0)
    model = lambda x, t, **kw: (kept, None)  # noqa: E731
    x, t, kw = torch.zeros(2, 2, 16, 16), torch.tensor([4, 4]), {"init_flow": None}
    out = diff.ddim_sample(model, x, t, model_kwargs=kw)
    assert [n for n, _ in stubbed] == ["dvd_sched_step_clip"] and set(out) == {"sample", "pred_xstart", "feat_dict"}
    # a foreign callable may keep the tensor it returns: the in-place clamp works on a copy of it
    assert out["pred_xstart"].data_ptr() != kept.data_ptr()
    del stubbed[:]
    seen = []
    out = diff.p_mean_variance(model, x, t, denoised_fn=lambda v: seen.append(1) or v, model_kwargs=kw)
    assert [n for n, _ in stubbed] == ["dvd_sched_step_clip"] and seen == [1]
    assert set(out) == {"mean", "variance", "log_variance", "pred_xstart", "feat_dict"}
    del stubbed[:]
    diff.ddim_sample(model, x, t, clip_denoised=False, model_kwargs=kw)
    assert [n for n, _ in stubbed] == ["dvd_sched_step"]


def test_all_zero_init_feat_is_dropped_before_it_is_tiled():
    """Without feedback init_feat is read at every step; the evaluation path's all-zero one must reach feature mode 0
    without being tiled over the hypotheses first."""
    from dvd_amd import gaussian_diffusion as gd
    diff = gd.GaussianDiffusion(betas=gd.get_named_beta_schedule("cosine", 10), model_mean_type=gd.ModelMeanType.START_X,
                                model_var_type=gd.ModelVarType.FIXED_LARGE, loss_type=gd.LossType.MSE,
                                rescale_timesteps=True)
    flow = torch.full((1, 2, 16, 16), 0.1)
    out = diff._first_step_kwargs({"init_flow": flow, "init_feat": torch.zeros(1, 256, 16, 16)}, 2, every_step=True)
    assert set(out) == {"init_flow"} and tuple(out["init_flow"].shape) == (2, 2, 16, 16)
    out = diff._first_step_kwargs({"init_flow": flow, "init_feat": torch.ones(1, 256, 16, 16)}, 2, every_step=True)
    assert tuple(out["init_feat"].shape) == (2, 256, 16, 16)
    out = diff._first_step_kwargs({"init_flow": flow, "init_feat": torch.ones(1, 256, 16, 16)}, 2)
    assert set(out) == {"init_flow"}              # with feedback the model overwrites it while t_model > 600


def test_what_stays_refused_says_why():
    from dvd_amd import gaussian_diffusion as gd
    diff = gd.GaussianDiffusion(betas=gd.get_named_beta_schedule("cosine", 10), model_mean_type=gd.ModelMeanType.START_X,
                                model_var_type=gd.ModelVarType.FIXED_LARGE, loss_type=gd.LossType.MSE)
    with pytest.raises(NotImplementedError, match="different network"):
        diff.ddim_sample_loop(None, (1, 2, 16, 16), model_kwargs={"iter": False}, time_variant=False)
    with pytest.raises(NotImplementedError, match="feeds the previous"):
        next(diff.ddim_sample_for_training(None, (1, 2, 16, 16), model_kwargs={}, time_variant=True, iter=False, timestep=-1))
