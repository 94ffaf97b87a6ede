"""Keyed sampler noise and the map deviation without a GPU: the stand-alone CPU restatement of the kernels
(dvd_amd/csrc/noise_host_check.cpp on noise_core.h), built under ASan/UBSan, against the NumPy definition tests/noise_model.py
bit for bit; the accuracy of the written-out logarithm, cosine and sine against float64; the distribution of the normals; every
refusal; how the keys travel from settings.keyed_noise to the sampling loop; the launcher's baseline round and map_dev column."""
import ctypes as C
import math
import subprocess
import types

import numpy as np
import pytest
import torch

import noise_model as N
from host_check import build_host_check

KEYS = [N.key(7, f"doc{i}") for i in range(3)]
KEY = N.key(1992, "12_1 copy.png")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("noise_host")
    exe = build_host_check("noise", tmp)

    def run(head, payload=b""):
        (tmp / "in.bin").write_bytes(np.array(head, np.int32).tobytes() + payload)
        r = subprocess.run([str(exe), str(tmp / "in.bin"), str(tmp / "out.bin")], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        status = int(r.stdout.strip())
        return status, ((tmp / "out.bin").read_bytes() if status == 0 else None)
    return run


def _host_randn(host_check, keys, n_hyp, g, slot):
    status, raw = host_check([0, len(keys), n_hyp, g, slot], np.array(keys, np.uint32).tobytes())
    assert status == 0
    return np.frombuffer(raw, np.float32).reshape(len(keys) * n_hyp, 2, g, g)


def _host_deviation(host_check, a, b):
    docs, _, g, _ = a.shape
    status, raw = host_check([1, docs, g], np.ascontiguousarray(a, np.float32).tobytes() + np.ascontiguousarray(b, np.float32).tobytes())
    assert status == 0
    return np.frombuffer(raw[:8 * docs], np.float64), np.frombuffer(raw[8 * docs:], np.float32).reshape(docs, g * g)


# ---- the restatement --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", (9, 16, 64))
def test_host_restatement_equals_the_model_under_sanitizers(host_check, g):
    """g = 9: 162 elements, a short last quad and samples that start 8 bytes off a 16-byte boundary; 16 and 64: whole quads.
    Three documents, one to three hypotheses, x_T's slot, the first step's and a large one."""
    for n_hyp in (1, 2, 3):
        for slot in (0, 1, 4001):
            got = _host_randn(host_check, KEYS, n_hyp, g, slot)
            want = N.randn_keyed(KEYS, n_hyp, g, slot)
            assert got.shape == want.shape and np.array_equal(_bits(got), _bits(want)), (n_hyp, slot, int((_bits(got) != _bits(want)).sum()))
    assert np.isfinite(want).all() and 0.5 < want.std() < 1.5


def test_host_restatement_document_alone_equals_the_document_in_the_batch(host_check):
    batch = _host_randn(host_check, KEYS, 2, 9, 3)
    for i, k in enumerate(KEYS):
        alone = _host_randn(host_check, [k], 2, 9, 3)
        assert np.array_equal(_bits(alone), _bits(batch[2 * i:2 * i + 2])), i
    assert not np.array_equal(batch[0], batch[1]) and not np.array_equal(batch[0], batch[2])      # another hypothesis, another document
    assert not np.array_equal(batch, _host_randn(host_check, KEYS, 2, 9, 4))                        # another slot


def test_host_restatement_refusals_and_empty_batches(host_check):
    for head in ([0, 1, 1, 1, 0], [0, 1, 1, 8193, 0], [0, -1, 1, 16, 0], [0, 1, -1, 16, 0], [0, 65536, 1, 16, 0], [1, 1, 1], [1, -1, 16],
                 [1, 1, 8193]):
        assert host_check(head, b"\0" * 8)[0] == -1, head
    assert _host_randn(host_check, [], 2, 16, 0).size == 0 and _host_randn(host_check, KEYS, 0, 16, 0).size == 0


@pytest.mark.parametrize("g", (9, 64))
def test_host_deviation_equals_the_model(host_check, g):
    """g = 9: one partly filled workgroup; g = 64: four of them.  Document 1's maps are equal: exactly 0.0."""
    rng = np.random.default_rng(g)
    a = rng.uniform(-1, 1, (3, 2, g, g)).astype(np.float32)
    b = (a + rng.normal(0, 0.02, a.shape)).astype(np.float32)
    b[1] = a[1]
    dev, dist = _host_deviation(host_check, a, b)
    assert np.array_equal(_bits(dist), _bits(N.point_distances(a, b)))
    assert dev.tolist() == N.map_deviation(a, b)
    assert dev[1] == 0.0 and dev[0] > 0 and dev[2] > 0
    plain = N.KPX * np.sum(dist.astype(np.float64), axis=1) / (g * g)
    assert np.all(np.abs(dev - plain) <= g * g * 2.0 ** -52 * plain)
    alone, _ = _host_deviation(host_check, a[2:], b[2:])
    assert alone[0] == dev[2]


def test_deviation_is_pixels_of_the_network_input():
    """A shift of the whole map by (3, 4) / 511 moves every sampling point by 0.987 * 5 pixels."""
    a = np.zeros((1, 2, 16, 16), np.float32)
    b = a.copy()
    b[0, 0] += np.float32(3 / 511)
    b[0, 1] += np.float32(4 / 511)
    assert abs(N.map_deviation(a, b)[0] - 0.987 * 5) < 1e-5


# ---- accuracy -----------------------------------------------------------------------------------------------------------------
# Bars by reasoning, not from what the code gives.  ln: the series and the reduction are each within a few ulp of the result
# (two roundings of s and its double, one product, two sums, against a result of at least 0.35 wherever e != 0): a budget of
# 4 ulp = 2^-21 relative; the square root halves it and adds half an ulp, so R is held to 2^-21 with room.  cos, sin: the angle
# carries one rounding (2^-24 relative of at most pi / 4), the polynomial a few of at most 2^-24 each: 2^-22 absolute.
R_BAR, CS_BAR, Z_BAR = 2.0 ** -21, 2.0 ** -22, 2.0 ** -16


def test_radius_is_accurate_for_every_u_a():
    k = np.arange(1, 2 ** 24 + 1)
    r = N.radius(k).astype(np.float64)
    r64 = np.sqrt(-2.0 * np.log(k * 2.0 ** -24))
    assert r[-1] == 0.0 and r64[-1] == 0.0                                 # u_a = 1
    rel = np.abs(r[:-1] - r64[:-1]) / r64[:-1]
    print(f"R: max relative error 2^{math.log2(rel.max()):.2f} at k = {int(k[rel.argmax()])}")
    assert rel.max() <= R_BAR
    assert rel[-1000:].max() <= R_BAR                                      # next to u = 1: small R is not lost


def test_cos_and_sin_are_accurate_for_every_u_b():
    k = np.arange(2 ** 24)
    c, s = N.cossin(k)
    ang = 2.0 * np.pi * k * 2.0 ** -24
    ec, es = np.abs(c - np.cos(ang)).max(), np.abs(s - np.sin(ang)).max()
    print(f"C: max absolute error 2^{math.log2(ec):.2f}   S: 2^{math.log2(es):.2f}")
    assert ec <= CS_BAR and es <= CS_BAR
    assert (c[0], s[0]) == (1.0, 0.0) and (c[1 << 22], s[1 << 22]) == (0.0, 1.0) and (c[1 << 23], s[1 << 23]) == (-1.0, 0.0)
    assert np.abs(c.astype(np.float64) ** 2 + s.astype(np.float64) ** 2 - 1).max() <= 2 * CS_BAR


@pytest.fixture(scope="module")
def normals():
    """[4, 2, 512, 512]: two documents x two hypotheses at slot 0 - 2^20 values per document - and document 0 at slot 1."""
    keys = [KEY, N.key(1992, "13_2 copy.png")]
    return N.randn_keyed(keys, 2, 512, 0), N.randn_keyed(keys[:1], 2, 512, 1), N.randn_keyed(keys[:1], 2, 512, 0, pair=N.box_muller64)


def test_generated_values_against_float64(normals):
    z, z64 = normals[0][:2].reshape(-1).astype(np.float64), normals[2].reshape(-1)
    assert z.size == 2 ** 20
    err = np.abs(z - z64) / np.maximum(1.0, np.abs(z64))
    print(f"z: max error 2^{math.log2(err.max()):.2f} of max(1, |z|)")
    assert err.max() <= Z_BAR


# ---- distribution -------------------------------------------------------------------------------------------------------------
def test_distribution_of_the_normals(normals):
    from scipy.special import ndtr
    z = normals[0][:2].reshape(-1).astype(np.float64)
    n = z.size
    assert n == 2 ** 20
    mean, var = z.mean(), z.var()
    kurt = ((z - mean) ** 4).mean() / var ** 2
    cdf = ndtr(np.sort(z))
    ks = max((np.arange(1, n + 1) / n - cdf).max(), (cdf - np.arange(n) / n).max())
    print(f"mean {mean:.2e} var-1 {var - 1:.2e} kurtosis-3 {kurt - 3:.2e} KS {ks:.2e} max|z| {np.abs(z).max():.3f}")
    assert abs(mean) <= 5 / math.sqrt(n)
    assert abs(var - 1) <= 5 * math.sqrt(2 / n)
    assert abs(kurt - 3) <= 5 * math.sqrt(24 / n)
    assert ks <= 1.95 / math.sqrt(n)
    assert np.abs(z).max() <= math.sqrt(48 * math.log(2))


def _corr(x, y):
    x, y = x.reshape(-1).astype(np.float64), y.reshape(-1).astype(np.float64)
    return abs(np.corrcoef(x, y)[0, 1]), x.size


def test_streams_are_uncorrelated(normals):
    base, slot1, _ = normals
    quads = base[:2].reshape(-1, 4)
    pairs = {"document": (base[:2], base[2:]), "hypothesis": (base[0], base[1]), "slot": (base[:2], slot1),
             "z0 / z1": (np.concatenate([quads[:, 0], quads[:, 2]]), np.concatenate([quads[:, 1], quads[:, 3]]))}
    for what, (x, y) in pairs.items():
        r, n = _corr(x, y)
        print(f"{what}: |r| = {r:.2e} over {n} pairs (bar {5 / math.sqrt(n):.2e})")
        assert r <= 5 / math.sqrt(n), what
        assert not np.array_equal(x, y)


# ---- refusals -----------------------------------------------------------------------------------------------------------------
@pytest.fixture
def no_launch(monkeypatch):
    from dvd_amd import lib

    def fail(name, *args):
        raise AssertionError(f"{name} was launched")
    monkeypatch.setattr(lib, "call", fail)


def test_ops_refuse_before_any_launch(no_launch):
    from dvd_amd import ops
    for kw, match in ((dict(n_hyp=-1), "n_hyp"), (dict(n_hyp=True), "n_hyp"), (dict(n_hyp=65536), "n_hyp"), (dict(g=1), "g must"),
                      (dict(g=8193), "g must"), (dict(g=16.0), "g must"), (dict(slot=-1), "slot"), (dict(slot=2 ** 32), "slot"),
                      (dict(keys=[(1, 2, 3)]), "keys"), (dict(keys=[(1, 2 ** 32)]), "keys"), (dict(keys=[(-1, 0)]), "keys"),
                      (dict(keys=[(1.5, 2)]), "keys"), (dict(keys=7), "keys"), (dict(keys=[(1, 2), (3,)]), "keys")):
        args = dict(keys=KEYS, n_hyp=2, g=16, slot=0, device="cpu")
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            ops.randn_keyed(**args)
    with pytest.raises(ValueError, match="out must be"):
        ops.randn_keyed(KEYS, 2, 16, 0, device="cpu", out=torch.zeros(5, 2, 16, 16))
    assert tuple(ops.randn_keyed(KEYS, 0, 16, 0, device="cpu").shape) == (0, 2, 16, 16)            # nothing to draw, nothing launched
    assert tuple(ops.randn_keyed([], 2, 16, 0, device="cpu").shape) == (0, 2, 16, 16)
    with pytest.raises(ValueError, match="one .* pair per document"):
        ops.noise_keys(KEYS, 2)
    assert ops.noise_keys(KEYS, 3).tolist() == [list(k) for k in KEYS]
    a = torch.zeros(2, 2, 16, 16)
    for x, y, match in ((a[0], a[0], r"\[docs,2,g,g\]"), (a, a[:1], "a is"), (torch.zeros(1, 2, 16, 8), torch.zeros(1, 2, 16, 8), "docs,2,g,g"),
                        (torch.zeros(1, 2, 1, 1), torch.zeros(1, 2, 1, 1), "g = 1")):
        with pytest.raises(ValueError, match=match):
            ops.map_deviation(x, y)
    assert ops.map_deviation(a[:0], a[:0]) == []
    with pytest.raises(lib_error()):
        ops.map_deviation(a, a)                                                                     # host tensors: no CPU path


def lib_error():
    from dvd_amd import lib
    return lib.DvdError


def test_library_refuses_before_any_launch():
    from dvd_amd import lib
    raw = lib.raw()
    one = C.c_void_p(16)            # non-null and aligned; never dereferenced: every call below is refused or a no-op
    for args in ((None, 1, 1, 16, 0, one, None), (one, 1, 1, 16, 0, None, None), (one, 1, 1, 1, 0, one, None), (one, 1, 1, 8193, 0, one, None),
                 (one, -1, 1, 16, 0, one, None), (one, 1, -1, 16, 0, one, None), (one, 65536, 1, 16, 0, one, None),
                 (one, 65535, 65535, 8192, 0, one, None), (C.c_void_p(2), 1, 1, 16, 0, one, None)):
        assert raw.dvd_randn_keyed(*args) == -1, args
    assert raw.dvd_randn_keyed(None, 0, 4, 16, 0, None, None) == 0 and raw.dvd_randn_keyed(None, 4, 0, 16, 0, None, None) == 0
    for args in ((None, one, 1, 16, one, one, None), (one, one, 1, 16, None, one, None), (one, one, 1, 16, one, None, None),
                 (one, one, 1, 1, one, one, None), (one, one, 65536, 16, one, one, None), (one, one, 1, 16, C.c_void_p(4), one, None)):
        assert raw.dvd_map_deviation(*args) == -1, args
    assert raw.dvd_map_deviation(None, None, 0, 16, None, None, None) == 0
    assert raw.dvd_map_deviation_workspace_bytes(3, 64) == 3 * 4 * 8 and raw.dvd_map_deviation_workspace_bytes(1, 9) == 8
    assert raw.dvd_map_deviation_workspace_bytes(1, 1) == -1 and raw.dvd_map_deviation_workspace_bytes(1, 8193) == -1
    assert "dvd_map_deviation_workspace_bytes" in lib.NON_STATUS and lib.RESTYPES["dvd_map_deviation_workspace_bytes"] is C.c_long


def test_kernels_use_no_scratch_and_no_library_math(tmp_path):
    """hipcc's own report for gfx950 with the library's flags: three kernels, 0 bytes of scratch each; and the ISA calls nothing
    (a library logarithm or sine would be a call or a v_log / v_sin / v_cos instruction)."""
    import os
    import re
    import shutil
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dvd_amd", "csrc", "noise.hip")
    base = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=on", "--cuda-device-only"]
    r = subprocess.run(base + ["-c", src, "-o", str(tmp_path / "n.o"), "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True, check=True)
    use = re.findall(r"Function Name: (\S+).*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+)", r.stderr, re.S)
    print(use)
    assert len(use) == 3 and all(int(scratch) == 0 and int(vgprs) <= 64 for _, vgprs, scratch in use), use    # 64: eight waves per SIMD
    subprocess.run(base + ["-S", src, "-o", str(tmp_path / "n.s")], check=True, stderr=subprocess.DEVNULL)
    text = (tmp_path / "n.s").read_text()
    body = text[text.index("randn_keyed_kernel"):]
    body = body[:body.index(".end_amdhsa_kernel")]
    assert not re.search(r"\bv_(log|exp|sin|cos)_f32|s_swappc|__ocml", body)


# ---- from the settings to the sampling loop -----------------------------------------------------------------------------------
class _Recorder:
    def __init__(self):
        self.calls = []

    def ddim_sample_loop(self, model, shape, **kw):
        self.calls.append(dict(kw, model=model, shape=shape))
        return torch.zeros(shape), {}


def _settings(**attrs):
    import admin.settings as ws
    s = ws.Settings()
    s.name, s.seed = "pytest_noise", 5
    for k, v in attrs.items():
        setattr(s, k, v)
    return s


def _batch(grid, paths=("b.png", "a.png", "12_1 copy.png")):
    return [{"path": p, "y512": torch.zeros(3, 8, 8), "mask_cat": torch.zeros(1, 8, 8), "mask_y512": torch.zeros(1, grid, grid),
             "line_msk": torch.zeros(1, grid, grid)} for p in paths]


LOG = types.SimpleNamespace(info=lambda *a: None)


def test_flag_absent_or_false_the_sampler_is_called_as_ever():
    from dvd_amd import evaluation
    for attrs in ({}, {"keyed_noise": False}):
        s, rec = _settings(**attrs), _Recorder()
        flow = evaluation.sample_batch(s, LOG, rec, "MODEL", _batch(s.env.grid_size), s.env.grid_size, "cpu")
        call, = rec.calls
        assert call["noise"] is None and set(call["sampling_kwargs"]) == {"src_img"}
        assert call["shape"] == (3, 2, s.env.grid_size, s.env.grid_size) and tuple(flow.shape) == call["shape"]


def test_flag_set_the_keys_are_the_corruption_keys_in_batch_order():
    from dvd_amd import evaluation, ops
    s, rec = _settings(keyed_noise=True), _Recorder()
    batch = _batch(s.env.grid_size)
    evaluation.sample_batch(s, LOG, rec, "MODEL", batch, s.env.grid_size, "cpu")
    call, = rec.calls
    assert call["noise"] is None and set(call["sampling_kwargs"]) == {"src_img", "noise_keys"}
    assert call["sampling_kwargs"]["noise_keys"] == [ops.corruption_key(5, d["path"]) for d in batch]
    assert call["sampling_kwargs"]["noise_keys"] == [N.key(5, d["path"]) for d in batch]
    rec.calls.clear()
    evaluation.sample_batch(_settings(), LOG, rec, "MODEL", batch, s.env.grid_size, "cpu", keyed_noise=True)    # what the loop passes
    assert rec.calls[0]["sampling_kwargs"]["noise_keys"] == [N.key(5, d["path"]) for d in batch]
    rec.calls.clear()
    evaluation.run_sample_lr_dewarping(s, LOG, rec, "MODEL", 4, torch.zeros(1, 3, 8, 8), 16, None, None, None, None, None, None,
                                       noise_keys=[(1, 2)])
    assert rec.calls[0]["sampling_kwargs"]["noise_keys"] == [(1, 2)]
    with pytest.raises(TypeError):                                                                               # keyword only
        evaluation.run_sample_lr_dewarping(s, LOG, rec, "MODEL", 4, torch.zeros(1, 3, 8, 8), 16, None, None, None, None, None, None,
                                           None, None, None, [(1, 2)])


def _exploding_loader():
    raise AssertionError("the loader was read")
    yield                                                                          # pragma: no cover


def test_a_flag_that_is_no_bool_is_refused_before_the_loader_is_read(tmp_path, monkeypatch):
    from dvd_amd import evaluation
    monkeypatch.chdir(tmp_path)
    for flag in (1, 0, "yes", None, 1.0):
        with pytest.raises(ValueError, match="settings.keyed_noise"):
            evaluation.run_evaluation_docunet(_settings(keyed_noise=flag), LOG, _exploding_loader(), None, torch.nn.Linear(1, 1), None)
    assert list(tmp_path.iterdir()) == []
    read = evaluation.RoundOptions.from_settings
    assert read(_settings()).keyed_noise is False and read(_settings(keyed_noise=True)).keyed_noise is True


def test_the_loop_refuses_a_key_list_of_the_wrong_length_or_shape():
    from dvd_amd import script_util
    d = script_util.create_gaussian_diffusion(steps=3, noise_schedule="cosine", predict_xstart=True, rescale_timesteps=True,
                                              timestep_respacing="")
    for keys in ([(1, 2)], [(1, 2), (3, 4), (5, 6)], [(1, 2, 3), (4, 5, 6)], [(1, 2), (3, 2 ** 32)], 5, [1, 2]):
        for loop in (d.ddim_sample_loop, d.p_sample_loop):
            with pytest.raises(ValueError, match="noise_keys"):
                loop(None, (2, 2, 16, 16), model_kwargs={}, time_variant=True, sampling_kwargs={"src_img": None, "noise_keys": keys})
        with pytest.raises(ValueError, match="noise_keys"):
            next(d.ddim_sample_loop_progressive_only_mean(None, (2, 2, 16, 16), model_kwargs={}, time_variant=True,
                                                          sampling_kwargs={"noise_keys": keys}))


class _DevStub:
    """ops.map_deviation on the host, by the model."""

    def __init__(self):
        self.calls = 0

    def map_deviation(self, a, b):
        self.calls += 1
        return N.map_deviation(a.numpy(), b.numpy())


def test_clean_rounds_leave_reference_maps_and_later_rounds_are_scored(monkeypatch):
    from dvd_amd import evaluation
    stub = _DevStub()
    monkeypatch.setattr(evaluation, "ops", stub)
    lines = []
    log = types.SimpleNamespace(info=lines.append)
    s = _settings(keyed_noise=True, map_ref={}, map_dev=[])
    batch = _batch(16, ("a", "b"))
    flow = torch.from_numpy(np.random.default_rng(0).uniform(-1, 1, (2, 2, 16, 16)).astype(np.float32))
    evaluation.score_map_deviation(s, log, batch, flow, clean=True)                       # the clean round: stores, scores nothing
    assert set(s.map_ref) == {"a", "b"} and torch.equal(s.map_ref["b"], flow[1]) and s.map_dev == [] and stub.calls == 0 and not lines
    moved = flow + 0.01
    evaluation.score_map_deviation(s, log, _batch(16, ("c", "b")), moved, clean=False)    # a corrupted round: "c" was never seen clean
    (path, value), = s.map_dev
    assert path == "b" and value == N.map_deviation(flow[1:].numpy(), moved[1:].numpy())[0] and value > 0
    assert lines == [f"b map_dev {value:.6f}", "c map_dev skipped: no clean round has left a reference map"]
    assert set(s.map_ref) == {"a", "b"} and torch.equal(s.map_ref["b"], flow[1])          # a corrupted round leaves no reference
    s.map_dev = []
    evaluation.score_map_deviation(s, log, batch, flow, clean=True)                       # the clean round again: exactly 0
    assert s.map_dev == [("a", 0.0), ("b", 0.0)]


# ---- the launcher -------------------------------------------------------------------------------------------------------------
def test_rounds_by_default_and_with_the_baseline():
    import run_sampling as R
    assert R.corruption_rounds() == [(0, 0)] and R.corruption_rounds(True) == [(5, c) for c in range(15)]
    assert R.corruption_rounds(True, 3, None) == [(3, 0)] and R.corruption_rounds(False, None, 16) == [(5, 16)]
    assert R.corruption_rounds(baseline=False) == [(0, 0)] and R.corruption_rounds(baseline=True) == [(0, 0)]
    assert R.corruption_rounds(True, baseline=True) == [(0, 0)] + [(5, c) for c in range(15)]
    assert R.corruption_rounds(False, 3, 10, baseline=True) == [(0, 0), (3, 10)]
    assert R.corruption_rounds(False, 0, None, baseline=True) == [(0, 0)]
    with pytest.raises(TypeError):
        R.corruption_rounds(True, None, None, True)


def _fake_launch(monkeypatch, R, seen):
    def run(settings):
        seen.append((settings.name, settings.severity, settings.corruption_number, getattr(settings, "keyed_noise", None)))
        settings.ms_ssim = [("a", 0.5 + settings.corruption_number / 100), ("b", 0.7)]
        if getattr(settings, "keyed_noise", False) and settings.severity and settings.corruption_number != 1:
            settings.map_dev = [("a", 1.5), ("b", 2.0 + settings.corruption_number)]
    monkeypatch.setattr(R, "importlib", types.SimpleNamespace(import_module=lambda name: types.SimpleNamespace(run=run)))
    monkeypatch.setattr(R, "shutil", types.SimpleNamespace(copyfile=lambda *a: None))


def test_table_gains_map_dev_only_under_the_flag(tmp_path, monkeypatch, capsys):
    import run_sampling as R
    monkeypatch.chdir(tmp_path)
    seen = []
    _fake_launch(monkeypatch, R, seen)
    table = tmp_path / "vis_hp" / "synthetic" / "exp" / "corruption_table.txt"
    R.run_sampling("dvd", "val_TDiff", 3, "exp", corruption=True)
    plain = table.read_text()
    assert seen[0] == ("exp/c00_gaussian_noise_s5", 5, 0, None) and all(name != "exp" for name, *_ in seen)
    rows = plain.splitlines()
    assert rows[0] == "no kind severity ms_ssim" and rows[1] == "0 gaussian_noise 5 0.600000" and rows[2] == "1 shot_noise 5 0.605000"
    assert "map_dev" not in plain
    seen.clear()
    R.run_sampling("dvd", "val_TDiff", 3, "exp", corruption=True, keyed_noise=True)
    assert seen[0] == ("exp", 0, 0, True) and seen[1] == ("exp/c00_gaussian_noise_s5", 5, 0, True) and len(seen) == 1 + len(rows) - 1
    keyed = table.read_text().splitlines()
    assert keyed[0] == "no kind severity ms_ssim map_dev"
    assert keyed[1] == "0 gaussian_noise 5 0.600000 1.750000" and keyed[2] == "1 shot_noise 5 0.605000 -"       # no value: a dash
    assert [r.rsplit(" ", 1)[0] for r in keyed] == rows                                                           # the rest is the old table
    assert table.read_text() in capsys.readouterr().out
    seen.clear()
    R.run_sampling("dvd", "val_TDiff", 3, "exp", severity=3, corruption_number=10, keyed_noise=True)
    assert seen == [("exp", 0, 0, True), ("exp/c10_brightness_s3", 3, 10, True)]
    assert table.read_text() == "no kind severity ms_ssim map_dev\n10 brightness 3 0.650000 6.750000\n"
    seen.clear()
    R.run_sampling("dvd", "val_TDiff", 3, "exp", keyed_noise=True)                                               # the clean round alone
    assert seen == [("exp", 0, 0, True)]
    seen.clear()
    with pytest.raises(ValueError, match="--severity"):                                                           # before the clean round runs
        R.run_sampling("dvd", "val_TDiff", 3, "exp", severity=6, keyed_noise=True)
    with pytest.raises(ValueError, match="--corruption_number"):
        R.run_sampling("dvd", "val_TDiff", 3, "exp", corruption_number=19, keyed_noise=True)
    assert seen == []
    with pytest.raises(TypeError):
        R.run_sampling("dvd", "val_TDiff", 3, "exp", True, False, None, None, True)


def test_write_corruption_table_text_is_unchanged(tmp_path):
    import run_sampling as R
    rows = [(0, "gaussian_noise", 5, {"ms_ssim": 0.6, "ld": 4.0}), (1, "shot_noise", 5, {"ms_ssim": 0.605})]
    text = R.write_corruption_table(str(tmp_path / "t" / "table.txt"), rows, ["ms_ssim", "ld"])
    assert text == "no kind severity ms_ssim ld\n0 gaussian_noise 5 0.600000 4.000000\n1 shot_noise 5 0.605000 -\n"
    rows = [(0, "gaussian_noise", 5, {"map_dev": 1.25})]
    assert R.write_corruption_table(str(tmp_path / "t" / "table.txt"), rows, ["map_dev"]) == "no kind severity map_dev\n0 gaussian_noise 5 1.250000\n"
