"""The corruption kernels (dvd_amd/csrc/corrupt.hip) against the NumPy definition tests/corrupt_model.py: bytes,
so every comparison is array_equal.  Expected values come from the model at test time.  The shapes are the smallest that take
every path: 40 x 56 and 64 x 48 are no multiple of any tile (32 x 16 FIR tiles, 64 x 4 pixel tiles, 1024 noise elements) and
smaller than the 49-tap FIR's reach, so it reflects at both borders of one tile; 512 x 512 is the size the document loop uses
and has many tiles; a batch of three has distinct keys."""
import numpy as np
import pytest
import torch

import corrupt_model as M

pytestmark = pytest.mark.gpu

KEY = M.key(1992, "12_1 copy.png")
SMALL = ((40, 56), (64, 48))


def _run(img, kind, severity, key):
    from dvd_amd import ops
    return ops.corrupt_rgb8(torch.from_numpy(np.ascontiguousarray(img)).cuda(), kind, severity, key).cpu().numpy()


@pytest.fixture(scope="module")
def images():
    return {hw: M.sample_image(*hw, seed=hw[0]) for hw in SMALL + ((512, 512),)}


@pytest.mark.parametrize("kind", M.DELIVERED, ids=lambda k: M.NAMES[k])
def test_kernels_equal_the_model(kind, images):
    for hw, severities in ((SMALL[0], (1, 5)), (SMALL[1], range(1, 6))):
        for severity in severities:
            want = M.corrupt(images[hw], kind, severity, KEY)
            got = _run(images[hw], kind, severity, KEY)
            assert np.array_equal(got, want), (hw, severity, int((got != want).sum()))
            assert np.array_equal(_run(images[hw], M.NAMES[kind], severity, KEY), want)       # by name


@pytest.mark.parametrize("kind,severity", ((0, 5), (3, 1), (6, 5), (14, 3)), ids=lambda v: str(v))
def test_kernels_equal_the_model_at_the_loop_size(kind, severity, images):
    img = images[(512, 512)]
    want = M.corrupt(img, kind, severity, KEY)
    got = _run(img, kind, severity, KEY)
    assert np.array_equal(got, want), int((got != want).sum())


@pytest.mark.parametrize("kind", M.DELIVERED, ids=lambda k: M.NAMES[k])
def test_image_in_a_batch_equals_the_image_alone(kind):
    imgs = np.stack([M.sample_image(40, 56, seed=s) for s in range(3)])
    keys = [M.key(7, f"doc{i}") for i in range(3)]
    got = _run(imgs, kind, 4, keys)
    assert got.shape == imgs.shape
    for i in range(3):
        assert np.array_equal(got[i], _run(imgs[i], kind, 4, keys[i])), i
        assert np.array_equal(got[i], M.corrupt(imgs[i], kind, 4, keys[i])), i
    if kind in (0, 1, 2, 5, 15):                                            # the keyed kinds: another key, other bytes
        assert not np.array_equal(_run(imgs[0], kind, 4, keys[1]), got[0])


@pytest.mark.parametrize("kind", (3, 5, 16, 6, 11), ids=lambda k: M.NAMES[k])
def test_constant_image_stays_constant(kind):
    for value in (0, 1, 254, 255):
        img = np.full((40, 56, 3), value, np.uint8)
        for severity in (1, 5):
            assert np.array_equal(_run(img, kind, severity, KEY), img), (value, severity)


@pytest.mark.parametrize("kind", M.FIR_KINDS, ids=lambda k: M.NAMES[k])
def test_fir_impulse_response_is_the_weight_table(kind):
    """A single pixel of 65536 / 256 = 256 would not fit a byte: a white pixel (255) answers with (255 w + 32768) >> 16, the
    table seen through the kernel's one rounding, mirrored about the pixel (a correlation)."""
    for severity in (1, 5):
        wt = M.table(kind, severity, M.motion_angle(KEY) if kind == 5 else 0)
        side = wt.shape[0]
        r = side // 2
        img = np.zeros((64, 72, 3), np.uint8)
        img[32, 36] = 255
        got = _run(img, kind, severity, KEY).astype(np.int64)
        want = np.zeros((64, 72), np.int64)
        want[32 - r:32 + r + 1, 36 - r:36 + r + 1] = ((255 * wt + 32768) >> 16)[::-1, ::-1]
        for c in range(3):
            assert np.array_equal(got[:, :, c], want), (severity, c)


def test_black_stays_black_under_shot_and_speckle_noise():
    black = np.zeros((40, 56, 3), np.uint8)
    for kind in (1, 15):
        for severity in (1, 5):
            assert not _run(black, kind, severity, KEY).any()


def test_stage_ends_round_trip_every_byte():
    """y = k / 255 is the ingest kernel's division; rint(255 y) gives k back for every byte."""
    from dvd_amd import ops
    k = np.arange(256, dtype=np.uint8).repeat(3 * 5).reshape(1, 32, 40, 3)
    y = ops.rgb8_to_unit(torch.from_numpy(k).cuda())
    assert np.array_equal(y.cpu().numpy(), (k.astype(np.float32) / np.float32(255)).transpose(0, 3, 1, 2))
    assert np.array_equal(ops.unit_to_rgb8(y).cpu().numpy(), k)
    odd = torch.tensor([-1.0, float("nan"), 2.0, 0.5, 0.4999], device="cuda").repeat(3, 8).reshape(1, 3, 8, 5).contiguous()
    assert ops.unit_to_rgb8(odd).cpu().numpy()[0, 0].tolist() == [[0, 0, 0], [0, 0, 0], [255, 255, 255], [128, 128, 128], [127, 127, 127]]


def _settings(name, **attrs):
    import admin.settings as ws
    s = ws.Settings()
    s.env.grid_size, s.env.diffusion_steps = 16, 3
    s.env.num_synthetic_docs, s.env.batch_docs, s.env.full_res = 2, 2, (96, 80)
    s.env.visualize, s.env.use_prestage_nets = False, True
    s.name, s.seed = name, 77
    for k, v in attrs.items():
        setattr(s, k, v)
    return s


def test_run_level_corruption_reaches_the_sampler_and_severity_0_changes_nothing(tmp_path, monkeypatch):
    """G = 16, 3 steps, synthetic weights, two synthetic image documents.  With severity 5 of gaussian_noise the y512 that
    reaches run_sample_lr_dewarping is the model's bytes over 255 (of the ingest kernel's clean bytes, keyed by seed and path);
    with severity 0 the pages are byte-equal to a run whose settings lack both attributes."""
    monkeypatch.chdir(tmp_path)
    from dvd_amd import evaluation, ops, val_TDiff
    seen = []
    inner = evaluation.run_sample_lr_dewarping

    def spy(settings, logger, diffusion, model, radius, source, *rest):
        seen.append(source.clone())
        return inner(settings, logger, diffusion, model, radius, source, *rest)
    monkeypatch.setattr(evaluation, "run_sample_lr_dewarping", spy)
    torch.manual_seed(0)
    plain = val_TDiff.run(_settings("plain"))
    torch.manual_seed(0)
    zero = val_TDiff.run(_settings("zero", severity=0, corruption_number=0))
    assert len(plain) == len(zero) == 2
    for (pa, a), (pb, b) in zip(plain, zero):
        assert pa == pb and torch.equal(a, b), pa
    assert torch.equal(seen[0], seen[1])
    torch.manual_seed(0)
    s = _settings("noisy", severity=5, corruption_number=0)
    noisy = val_TDiff.run(s)
    assert [p for p, _ in noisy] == [p for p, _ in plain] and tuple(noisy[0][1].shape) == (96, 80, 3)
    docs = list(evaluation.synthetic_documents(s, range(2)))
    for j, d in enumerate(docs):
        y_clean = ops.ingest_u8(torch.from_numpy(d["image_u8"]).cuda(), swap_rb=False, out_size=512)
        y_clean = (y_clean[0] if isinstance(y_clean, tuple) else y_clean).cpu().numpy()
        assert np.array_equal(seen[0][j].cpu().numpy(), y_clean)
        k = np.clip(np.rint(np.float32(255) * y_clean), 0, 255).astype(np.uint8).transpose(1, 2, 0)
        want = M.corrupt(k, 0, 5, M.key(77, d["path"])).astype(np.float32).transpose(2, 0, 1) / np.float32(255)
        assert np.array_equal(seen[2][j].cpu().numpy(), want), j
