"""The kernels of dvd_amd/csrc/noise.hip against the NumPy definition tests/noise_model.py, bit for bit; the keys
through the diffusion object; --keyed_noise and the map_dev column through the launcher.  Expected values come from the model at
test time.  Shapes: g = 9 has a short last quad and samples that start 8 bytes off a 16-byte boundary (the scalar-store path),
g = 16 and 64 take the 16-byte stores; g = 9 fills part of one workgroup of the deviation, g = 64 four."""
import numpy as np
import pytest
import torch

import noise_model as N
from dvd_amd import synth

pytestmark = pytest.mark.gpu

KEYS = [N.key(7, f"doc{i}") for i in range(3)]


def _bits(a):
    if torch.is_tensor(a):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("g", (9, 16, 64))
def test_randn_keyed_equals_the_model(g):
    from dvd_amd import ops
    for n_hyp in (1, 2):
        for slot in (0, 7):
            want = N.randn_keyed(KEYS, n_hyp, g, slot)
            got = ops.randn_keyed(KEYS, n_hyp, g, slot)
            assert got.dtype == torch.float32 and tuple(got.shape) == (3 * n_hyp, 2, g, g)
            assert np.array_equal(_bits(got), _bits(want)), (n_hyp, slot, int((_bits(got) != _bits(want)).sum()))
    # an out= buffer is filled in place, past neither end; device keys (what the loop uploads once) give the same bits
    buf = torch.full((3 * 2 * 2 * g * g + 8,), 5.0, device="cuda")
    out = buf[4:-4].view(6, 2, g, g)
    keys_dev = ops.noise_keys_tensor(KEYS, "cuda")
    assert ops.randn_keyed(keys_dev, 2, g, 7, out=out) is out
    assert np.array_equal(_bits(out), _bits(want)) and buf[:4].tolist() == [5.0] * 4 and buf[-4:].tolist() == [5.0] * 4
    # a document alone equals the document in the batch
    for i, k in enumerate(KEYS):
        assert np.array_equal(_bits(ops.randn_keyed([k], 2, g, 7)), _bits(want[2 * i:2 * i + 2])), i


@pytest.mark.parametrize("g", (9, 64))
def test_map_deviation_equals_the_model(g):
    from dvd_amd import ops
    rng = np.random.default_rng(g)
    a = rng.uniform(-1, 1, (3, 2, g, g)).astype(np.float32)
    b = (a + rng.normal(0, 0.02, a.shape)).astype(np.float32)
    b[1] = a[1]
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    got = ops.map_deviation(ta, tb)
    dist = N.point_distances(a, b)                                   # float32, each operation rounded
    plain = N.KPX * np.sum(dist.astype(np.float64), axis=1) / (g * g)
    print(f"g = {g}: map_dev {got}, against np.sum {[abs(x - y) / y if y else 0.0 for x, y in zip(got, plain)]} relative")
    for d in range(3):
        assert abs(got[d] - plain[d]) <= g * g * 2.0 ** -52 * plain[d], d      # f64 additions of g^2 terms
    assert got == N.map_deviation(a, b)                               # the distances are the model's, added in the model's order
    assert got[1] == 0.0 and ops.map_deviation(ta, ta) == [0.0, 0.0, 0.0]
    assert ops.map_deviation(ta[2:], tb[2:]) == got[2:]               # a document alone


# ---- through the diffusion object ---------------------------------------------------------------------------------------------
G, STEPS, DOCS, HYP = 16, 3, 2, 2


@pytest.fixture(scope="module")
def built():
    import admin.settings as ws
    from dvd_amd.script_util import args_to_dict, create_model_and_diffusion, model_and_diffusion_defaults
    s = ws.Settings()
    s.env.grid_size, s.env.diffusion_steps = G, STEPS
    s.name = "pytest"
    model, diffusion = create_model_and_diffusion(device="cuda", train_mode=s.env.train_mode, tv=s.env.time_variant,
                                                  grid_size=G, **args_to_dict(s, model_and_diffusion_defaults().keys()))
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in synth.synth_state_dict(G, 7).items()}
    model.cpu().load_state_dict(sd, strict=False)
    model.to("cuda")
    model.eval()
    docs = [synth.synth_document(i, G, 1234) for i in range(DOCS)]
    doc = {k: torch.stack([torch.from_numpy(d[k]) for d in docs]).cuda() for k in ("y512", "mask_cat", "mask_y512", "line_msk")}
    kw = {"init_flow": torch.zeros(DOCS, 2, G, G, device="cuda"), "src_feat": None, "src_64": None, "y512": doc["y512"],
          "tmode": s.env.train_mode, "mask_cat": doc["mask_cat"], "init_feat": torch.zeros(DOCS, 256, G, G, device="cuda"), "iter": True,
          "mask_y512": doc["mask_y512"], "line_msk": doc["line_msk"]}
    return model, diffusion, kw


def _spy(monkeypatch):
    """Record what reaches sampler.sample: x_T, and every tensor its noise_fn hands out, by step index."""
    from dvd_amd import sampler
    seen, real = {"x_T": [], "noise": []}, sampler.sample

    def spy(eng, tables, x_T, *a, noise_fn=None, **k):
        seen["x_T"].append(x_T.clone())
        recording = None
        if noise_fn is not None:
            def recording(i):
                t = noise_fn(i)
                seen["noise"].append((i, t.clone()))
                return t
        return real(eng, tables, x_T, *a, noise_fn=recording, **k)
    monkeypatch.setattr(sampler, "sample", spy)
    return seen


def _loop(built, keys, seed, **extra):
    model, diffusion, kw = built
    torch.manual_seed(seed)
    sampling_kwargs = {"src_img": kw["y512"]}
    if keys is not None:
        sampling_kwargs["noise_keys"] = keys
    sample, _ = diffusion.ddim_sample_loop(model, (DOCS, 2, G, G), noise=None, clip_denoised=False, model_kwargs=kw, eta=0.0,
                                           progress=True, denoised_fn=None, sampling_kwargs=sampling_kwargs, logger=None,
                                           n_batch=HYP, time_variant=True, pyramid=None, **extra)
    return sample


def test_keys_decide_x_T_whatever_the_torch_seed(built, monkeypatch):
    seen = _spy(monkeypatch)
    keys = KEYS[:DOCS]
    a = _loop(built, keys, seed=1)
    b = _loop(built, keys, seed=2)
    want = N.randn_keyed(keys, HYP, G, 0)
    assert len(seen["x_T"]) == 2 and not seen["noise"]
    for x_T in seen["x_T"]:
        assert np.array_equal(_bits(x_T), _bits(want))
    assert tuple(a.shape) == (DOCS, 2, G, G) and np.array_equal(_bits(a), _bits(b))          # two whole calls: byte-equal maps
    c, d = _loop(built, None, seed=1), _loop(built, None, seed=2)                              # torch's generator, as ever
    assert not np.array_equal(_bits(c), _bits(d))
    assert not np.array_equal(_bits(seen["x_T"][2]), _bits(want))
    assert np.array_equal(_bits(_loop(built, None, seed=1)), _bits(c))
    explicit = torch.from_numpy(N.randn_keyed(KEYS[1:3], HYP, G, 0))
    model, diffusion, kw = built
    diffusion.ddim_sample_loop(model, (DOCS, 2, G, G), noise=explicit, model_kwargs=kw, n_batch=HYP, time_variant=True,
                               sampling_kwargs={"noise_keys": keys})
    assert np.array_equal(_bits(seen["x_T"][-1]), _bits(explicit))                             # an explicit noise= still wins


def test_keyed_loop_draws_nothing_from_torch(built):
    torch.manual_seed(3)
    before = torch.cuda.get_rng_state().clone()
    _loop(built, KEYS[:DOCS], seed=3, sampler_kind="ddpm")
    assert torch.equal(torch.cuda.get_rng_state(), before)
    _loop(built, None, seed=3)
    assert not torch.equal(torch.cuda.get_rng_state(), before)


def test_ddpm_noise_of_step_i_is_slot_1_plus_i(built, monkeypatch):
    seen = _spy(monkeypatch)
    keys = KEYS[:DOCS]
    a = _loop(built, keys, seed=1, sampler_kind="ddpm")
    steps = [i for i, _ in seen["noise"]]
    assert steps and set(steps) <= set(range(STEPS)) and len(set(steps)) == len(steps) and len(steps) >= STEPS - 1
    for i, t in seen["noise"]:
        assert np.array_equal(_bits(t), _bits(N.randn_keyed(keys, HYP, G, 1 + i))), i
    assert np.array_equal(_bits(seen["x_T"][0]), _bits(N.randn_keyed(keys, HYP, G, 0)))
    model, diffusion, kw = built
    torch.manual_seed(9)
    b, _ = diffusion.p_sample_loop(model, (DOCS, 2, G, G), model_kwargs=kw, n_batch=HYP, time_variant=True,
                                   sampling_kwargs={"noise_keys": keys}, clip_denoised=False)
    assert np.array_equal(_bits(a), _bits(b))


# ---- end to end ---------------------------------------------------------------------------------------------------------------
def _launcher(monkeypatch, tmp_path):
    import types
    import admin.settings as ws
    import run_sampling as R
    monkeypatch.chdir(tmp_path)
    made = []

    class Small(ws.Settings):
        def __init__(self):
            super().__init__()
            self.env.grid_size, self.env.diffusion_steps = 16, 3
            self.env.num_synthetic_docs, self.env.batch_docs, self.env.full_res = 2, 2, (96, 80)
            self.env.visualize, self.env.use_prestage_nets = False, True
            self.env.eval_dataset_name = "synthetic"
            made.append(self)
    monkeypatch.setattr(R, "ws_settings", types.SimpleNamespace(Settings=Small))
    monkeypatch.setattr(R, "shutil", types.SimpleNamespace(copyfile=lambda *a: None))
    return R, made


PATHS = ["synthetic_00000", "synthetic_00001"]


@pytest.fixture(scope="module")
def keyed_run(tmp_path_factory):
    """The launcher under --keyed_noise, once: G = 16, 3 steps, synthetic weights, two synthetic image documents; the clean
    round, then brightness at severity 3.  The tests below stay in its directory."""
    tmp_path = tmp_path_factory.mktemp("keyed_run")
    with pytest.MonkeyPatch.context() as mp:
        R, made = _launcher(mp, tmp_path)
        R.run_sampling("dvd", "val_TDiff", 77, "exp", keyed_noise=True, severity=3, corruption_number=10)
        settings, = made
        yield settings, tmp_path / "vis_hp" / "synthetic" / "exp"


def test_keyed_run_writes_the_clean_round_map_dev_and_the_table(keyed_run):
    settings, root = keyed_run
    assert sorted(settings.map_ref) == PATHS and all(tuple(v.shape) == (2, 16, 16) and not v.is_cuda for v in settings.map_ref.values())
    assert not (root / "map_dev.txt").exists()                                 # the clean round scored nothing
    lines = (root / "c10_brightness_s3" / "map_dev.txt").read_text().splitlines()
    values = [float(ln.split()[1]) for ln in lines]
    assert [ln.split()[0] for ln in lines] == PATHS and all(np.isfinite(v) and v > 0 for v in values)
    assert [p for p, _ in settings.map_dev] == PATHS and all(abs(v - w) <= 5e-7 for (_, v), w in zip(settings.map_dev, values))
    table = (root / "corruption_table.txt").read_text().splitlines()
    assert table[0].split()[:3] == ["no", "kind", "severity"] and table[0].split()[-1] == "map_dev" and len(table) == 2
    assert table[1].split()[:3] == ["10", "brightness", "3"] and abs(float(table[1].split()[-1]) - sum(values) / 2) < 1e-6


def test_clean_round_again_deviates_by_exactly_zero(keyed_run):
    """The clean round a second time, against the stored reference maps: the same keys, the same noise, the same maps."""
    from dvd_amd import val_TDiff
    settings, root = keyed_run
    settings.severity, settings.corruption_number, settings.name = 0, 0, "exp"
    val_TDiff.run(settings)
    assert settings.map_dev == [(p, 0.0) for p in PATHS]
    assert (root / "map_dev.txt").read_text().splitlines() == [f"{p} 0.000000" for p in PATHS]


def test_the_same_run_without_the_flag_writes_no_map_dev(tmp_path, monkeypatch):
    R, made = _launcher(monkeypatch, tmp_path)
    R.run_sampling("dvd", "val_TDiff", 77, "exp", severity=3, corruption_number=10)
    settings, = made
    assert not hasattr(settings, "map_dev") and not hasattr(settings, "map_ref") and not hasattr(settings, "keyed_noise")
    root = tmp_path / "vis_hp" / "synthetic" / "exp"
    assert (root / "c10_brightness_s3").is_dir() and not list(root.rglob("map_dev.txt"))
    assert not (root / "corruption_table.txt").exists() or "map_dev" not in (root / "corruption_table.txt").read_text()
