"""Common corruptions without a GPU: the stand-alone CPU restatement of the kernels
(dvd_amd/csrc/corrupt_host_check.cpp on corrupt_core.h), built under ASan/UBSan, against the NumPy definition
tests/corrupt_model.py byte for byte; the library's tables against float64 NumPy; what each kind MEANS, on the model; the
determinism of the key; every refusal; the document loop's route when nothing is corrupted; the launcher's rounds."""
import subprocess
import types

import numpy as np
import pytest
import torch

import corrupt_model as M
from host_check import build_host_check

KEY = M.key(1992, "12_1 copy.png")
SMALL = ((40, 56), (64, 48))


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("corrupt_host")
    exe = build_host_check("corrupt", tmp)

    def run(imgs, kind, severity, keys):
        """(status, corrupted images or None) for a batch [n,h,w,3]."""
        n, h, w = imgs.shape[:3]
        (tmp / "in.bin").write_bytes(np.array([n, h, w, kind, severity], np.int32).tobytes()
                                     + np.array(keys, np.uint32).tobytes() + np.ascontiguousarray(imgs, np.uint8).tobytes())
        r = subprocess.run([str(exe), str(tmp / "in.bin"), str(tmp / "out.bin")], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        status = int(r.stdout.strip())
        return status, (np.fromfile(tmp / "out.bin", np.uint8).reshape(imgs.shape) if status == 0 else None)
    return run


@pytest.mark.parametrize("kind", M.KERNEL_KINDS, ids=lambda k: M.NAMES[k])
def test_host_restatement_equals_the_model_under_sanitizers(host_check, kind):
    """Every kernel kind, all five severities at 40 x 56 and 64 x 48 (no multiple of any tile; the 49-tap FIR reflects at both
    borders), severities 1 and 5 at 512 x 512.  Kind 14 is the JPEG codec, whose restatements tests/test_jpeg_cpu.py and
    tests/test_jpegdec_cpu.py hold to the same models."""
    for (h, w), severities in ((SMALL[0], range(1, 6)), (SMALL[1], range(1, 6)), ((512, 512), (1, 5))):
        img = M.sample_image(h, w, seed=h)
        for severity in severities:
            status, got = host_check(img[None], kind, severity, [KEY])
            assert status == 0
            want = M.corrupt(img, kind, severity, KEY)
            assert np.array_equal(got[0], want), (h, w, severity, int((got[0] != want).sum()))
            assert not np.array_equal(want, img)


def test_host_restatement_batch_and_refusals(host_check):
    """An image in a batch of three equals the image alone; a refused call prints dvd_corrupt_rgb8's status and writes nothing."""
    imgs = np.stack([M.sample_image(40, 56, seed=s) for s in range(3)])
    keys = [M.key(7, f"doc{i}") for i in range(3)]
    for kind in (0, 5, 11):
        status, got = host_check(imgs, kind, 3, keys)
        assert status == 0
        for i in range(3):
            assert np.array_equal(got[i], M.corrupt(imgs[i], kind, 3, keys[i])), (kind, i)
    for kind in M.REFUSED + (14, 19, -1):
        assert host_check(imgs[:1], kind, 3, keys[:1])[0] == -47
    assert host_check(imgs[:1], 0, 0, keys[:1])[0] == -48 and host_check(imgs[:1], 0, 6, keys[:1])[0] == -48
    assert host_check(imgs[:1, :31], 0, 1, keys[:1])[0] == -49


# ---- tables ---------------------------------------------------------------------------------------------------------------
def _fir_cases():
    return [(3, s, 0) for s in range(1, 6)] + [(16, s, 0) for s in range(1, 6)] + [(5, s, a) for s in range(1, 6) for a in (-45, -17, 0, 1, 30, 45)]


def test_tables_are_float64_numpy_within_one_quantum():
    """One rounding of a value that is itself good to a few ulp of a double: every entry within one quantum.  The largest tap
    of a FIR table also takes the remainder, so it may move by one more quantum per tap that rounded the other way."""
    for severity in range(1, 6):
        got, ref = M.table(1, severity), M.reference_table(1, severity)
        assert got.shape == ref.shape == (256, M.PHOTONS[severity - 1])
        assert np.abs(got - ref).max() <= 1
        assert (np.diff(got, axis=1) >= 0).all() and got[0].min() == 0xffffffff       # a CDF; x = 0 never counts a photon
    for kind, severity, angle in _fir_cases():
        got, ref = M.table(kind, severity, angle), M.reference_table(kind, severity, angle)
        assert got.shape == ref.shape and got.shape[0] <= 49 and got.shape[0] % 2 == 1
        assert int(got.sum()) == 65536 and got.min() >= 0
        diff = np.abs(got - ref)
        top = np.unravel_index(int(np.argmax(ref)), ref.shape)
        others = diff.copy()
        others[top] = 0
        assert others.max() <= 1 and diff[top] <= 1 + int((others != 0).sum()), (kind, severity, angle)
    assert M.table(16, 5).shape == (49, 49) and M.table(3, 5).shape == (25, 25) and M.table(5, 5, 7).shape == (41, 41)


def test_table_export_refuses_bad_arguments():
    from dvd_amd import lib
    raw = lib.raw()
    assert raw.dvd_corrupt_table(0, 1, 0, None, 0) == -47 and raw.dvd_corrupt_table(19, 1, 0, None, 0) == -47
    assert raw.dvd_corrupt_table(16, 0, 0, None, 0) == -48 and raw.dvd_corrupt_table(16, 6, 0, None, 0) == -48
    assert raw.dvd_corrupt_table(5, 1, 46, None, 0) == -1
    buf = (lib.C.c_uint32 * 4)()
    assert raw.dvd_corrupt_table(16, 1, 0, buf, 4) == -1 and b"do not fit" in raw.dvd_last_error()
    assert [raw.dvd_corrupt_supported(k) for k in range(-1, 20)] == [0] + [1 if k in M.KERNEL_KINDS else 2 if k == 14 else 0 for k in range(19)] + [0]
    assert {"dvd_corrupt_supported", "dvd_corrupt_table"} <= lib.NON_STATUS


# ---- meaning --------------------------------------------------------------------------------------------------------------
def test_gaussian_noise_has_the_published_sigma():
    """Constant 128 at severity 1: 6 sigma = 122 does not reach the clamp, Irwin-Hall(12) has unit variance, and over 786 432
    elements the estimator's standard error is 0.08 %: the sample standard deviation lies within 1 % of 255 * 0.08."""
    out = M.corrupt(np.full((512, 512, 3), 128, np.uint8), 0, 1, KEY).astype(np.float64)
    assert out.min() > 0 and out.max() < 255
    assert abs(out.std() / (255 * 0.08) - 1) < 0.01 and abs(out.mean() - 128) < 4 * 255 * 0.08 / np.sqrt(out.size)


def test_shot_noise_is_poisson():
    """x = 128, c = 60: the photon count k = out c / 255 has mean and variance lambda = 128 * 60 / 255 within four standard
    errors (the variance estimator's: sqrt((mu4 - lambda^2) / n) with mu4 = lambda + 3 lambda^2)."""
    out = M.corrupt(np.full((512, 512, 3), 128, np.uint8), 1, 1, KEY).astype(np.int64)
    k = (out * 60 + 127) // 255                       # out = round(255 k / 60) inverts exactly below the clamp
    assert np.array_equal((2 * 255 * k + 60) // 120, out)
    lam, n = 128 * 60 / 255.0, k.size
    assert abs(k.mean() - lam) < 4 * np.sqrt(lam / n)
    assert abs(k.var() - lam) < 4 * np.sqrt((lam + 2 * lam * lam) / n)


@pytest.mark.parametrize("severity", (1, 5))
def test_impulse_noise_fractions(severity):
    p = M.IMPULSE[severity - 1] / 100
    out = M.corrupt(np.full((512, 512, 3), 128, np.uint8), 2, severity, KEY)
    se = np.sqrt(p / 2 * (1 - p / 2) / out.size)
    assert abs((out == 255).mean() - p / 2) < 4 * se and abs((out == 0).mean() - p / 2) < 4 * se
    assert ((out == 0) | (out == 255) | (out == 128)).all()


@pytest.mark.parametrize("kind", (3, 5, 16, 6, 11), ids=lambda k: M.NAMES[k])
def test_constant_image_stays_constant(kind):
    for value in (0, 1, 77, 254, 255):
        img = np.full((40, 56, 3), value, np.uint8)
        for severity in range(1, 6):
            assert np.array_equal(M.corrupt(img, kind, severity, KEY), img), (value, severity)


@pytest.mark.parametrize("kind", M.FIR_KINDS, ids=lambda k: M.NAMES[k])
def test_fir_kinds_against_scipy_correlate(kind):
    """Within 0.5 + 255 * sum |w_Q16 / 65536 - w_float64| of scipy.ndimage.correlate(mode='mirror') with the float64 weights:
    the rounding of the result plus the quantisation of the weights; the bound is computed from the model's own weights."""
    from scipy import ndimage
    img = M.sample_image(64, 48, seed=3)
    for severity in range(1, 6):
        angle = M.motion_angle(KEY) if kind == 5 else 0
        real, q16 = M.fir_real(kind, severity, angle), M.table(kind, severity, angle)
        bound = 0.5 + 255 * np.abs(q16 / 65536.0 - real).sum()
        got = M.corrupt(img, kind, severity, KEY).astype(np.float64)
        for c in range(3):
            ref = ndimage.correlate(img[:, :, c].astype(np.float64), real, mode="mirror")
            assert np.abs(got[:, :, c] - ref).max() <= bound + 1e-9, (severity, c)


def test_brightness_of_grey_and_of_colour():
    for severity, c in enumerate((.1, .2, .3, .4, .5), 1):
        grey = np.repeat(np.arange(256, dtype=np.uint8)[:, None, None], 3, axis=2).repeat(32, axis=1)      # [256,32,3]
        want = np.minimum(255, np.arange(256) + int(np.rint(255 * c)))
        assert np.array_equal(M.corrupt(grey, 10, severity, KEY)[:, 0, 0], want)
        img = M.sample_image(40, 56)
        out = M.corrupt(img, 10, severity, KEY).astype(int)
        assert np.array_equal(out.max(axis=2), np.minimum(255, img.max(axis=2).astype(int) + int(np.rint(255 * c))))
        assert (out >= img).all()                                         # hue and saturation kept: no channel falls


def test_pixelate_is_constant_on_its_cells():
    for h, w in SMALL:
        img = M.sample_image(h, w, seed=5)
        for severity in range(1, 6):
            out = M.corrupt(img, 13, severity, KEY)
            (mh, iy), (mw, ix) = M.pixelate_cells(h, severity), M.pixelate_cells(w, severity)
            assert mh == h * M.CELLS[severity - 1] // 100 and len(set(iy)) == mh and len(set(ix)) == mw
            for i in range(mh):
                for j in range(mw):
                    cell = out[iy == i][:, ix == j].reshape(-1, 3)
                    assert (cell == cell[0]).all()
    flat = np.full((40, 56, 3), 93, np.uint8)
    assert np.array_equal(M.corrupt(flat, 13, 5, KEY), flat)


def test_jpeg_compression_is_the_codec_models():
    import jpeg_model as J
    import jpegdec_model as D
    img = M.sample_image(40, 56)
    for severity, quality in enumerate((25, 18, 15, 10, 7), 1):
        assert np.array_equal(M.corrupt(img, 14, severity, KEY), D.decode(J.model_file(img, quality, "420"))[0])


def test_speckle_and_shot_keep_black():
    black = np.zeros((40, 56, 3), np.uint8)
    for kind in (1, 15):
        for severity in range(1, 6):
            assert not M.corrupt(black, kind, severity, KEY).any()


# ---- determinism ----------------------------------------------------------------------------------------------------------
def test_key_names_the_document_not_the_batch():
    import zlib
    from dvd_amd import ops
    assert ops.corruption_key(1992, "a/b.png") == M.key(1992, "a/b.png") == (1992, zlib.crc32(b"a/b.png"))
    assert ops.corruption_key(2 ** 40 + 5, "x")[0] == 5
    img = M.sample_image(40, 56)
    for kind in (0, 1, 2, 5, 15):
        a = M.corrupt(img, kind, 3, M.key(1, "doc0"))
        assert np.array_equal(a, M.corrupt(img, kind, 3, M.key(1, "doc0")))
        assert not np.array_equal(a, M.corrupt(img, kind, 3, M.key(1, "doc1")))
        assert not np.array_equal(a, M.corrupt(img, kind, 3, M.key(2, "doc0")))
    angles = {M.motion_angle(M.key(1, f"doc{i}")) for i in range(300)}
    assert len(angles) > 60 and min(angles) >= -45 and max(angles) <= 45


# ---- refusals -------------------------------------------------------------------------------------------------------------
@pytest.fixture
def no_launch(monkeypatch):
    from dvd_amd import lib

    def fail(name, *args):
        raise AssertionError(f"{name} was called")
    monkeypatch.setattr(lib, "call", fail)


def test_ops_refuse_before_any_launch(no_launch):
    from dvd_amd import lib, ops
    assert ops.CORRUPTIONS == M.NAMES and len(ops.CORRUPTIONS) == 19
    img = torch.zeros(40, 56, 3, dtype=torch.uint8)
    for kind in M.REFUSED:
        with pytest.raises(ops.CorruptionUnsupported, match=M.NAMES[kind]) as e:
            ops.corrupt_rgb8(img, kind, 3, KEY)
        assert e.value.kind == kind and e.value.name == M.NAMES[kind] and isinstance(e.value, ValueError)
        with pytest.raises(ops.CorruptionUnsupported):
            ops.corrupt_rgb8(img, M.NAMES[kind], 3, KEY)
    for severity in (6, 0, -1, True, 2.0, "5", None):
        with pytest.raises(ValueError, match="severity"):
            ops.corrupt_rgb8(img, 0, severity, KEY)
    for kind in (19, -1, True, 2.0, "gaussian", None):
        with pytest.raises(ValueError, match="kind"):
            ops.corrupt_rgb8(img, kind, 3, KEY)
    for shape in ((31, 56, 3), (40, 31, 3), (2, 31, 56, 3), (40, 56, 4), (40, 56)):
        with pytest.raises(ValueError):
            ops.corrupt_rgb8(torch.zeros(shape, dtype=torch.uint8), 0, 3, [KEY, KEY] if len(shape) == 4 else KEY)
    for key in ((1,), (1, 2, 3), (-1, 2), (1, 2 ** 32), (1.5, 2), [KEY, KEY]):
        with pytest.raises(ValueError, match="key"):
            ops.corrupt_rgb8(img, 0, 3, key)
    with pytest.raises(ValueError, match="uint8"):
        ops.corrupt_rgb8(img.float(), 0, 3, KEY)
    for kind in M.DELIVERED:                                   # a host tensor never reaches a launch
        with pytest.raises(lib.DvdError, match="device tensor"):
            ops.corrupt_rgb8(img, kind, 3, KEY)
    with pytest.raises(lib.DvdError, match="device tensor"):
        ops.unit_to_rgb8(torch.zeros(1, 3, 40, 56))
    with pytest.raises(lib.DvdError, match="device tensor"):
        ops.rgb8_to_unit(img[None])


def test_library_refuses_with_codes_of_their_own():
    from dvd_amd import lib
    raw = lib.raw()
    for kind in M.REFUSED + (14, 19, -1):
        assert raw.dvd_corrupt_rgb8(None, None, 1, 64, 64, kind, 3, None, None) == -47
    assert raw.dvd_corrupt_rgb8(None, None, 1, 64, 64, 14, 3, None, None) == -47 and b"dvd_jpeg_encode_rgb8" in raw.dvd_last_error()
    assert raw.dvd_corrupt_rgb8(None, None, 1, 64, 64, 0, 6, None, None) == -48
    assert raw.dvd_corrupt_rgb8(None, None, 1, 31, 64, 0, 3, None, None) == -49
    assert raw.dvd_corrupt_rgb8(None, None, 1, 64, 16385, 0, 3, None, None) == -49
    assert raw.dvd_corrupt_rgb8(None, None, 0, 64, 64, 0, 3, None, None) == -1
    assert raw.dvd_corrupt_rgb8(None, None, 1, 64, 64, 0, 3, None, None) == -1 and b"null" in raw.dvd_last_error()


# ---- the document loop ----------------------------------------------------------------------------------------------------
class _Stop(Exception):
    pass


def _settings(**attrs):
    import admin.settings as ws
    s = ws.Settings()
    s.name, s.seed = "pytest_corrupt", 5
    for k, v in attrs.items():
        setattr(s, k, v)
    return s


def _exploding_loader():
    raise AssertionError("the loader was read")
    yield                                                                          # pragma: no cover


def test_settings_are_refused_before_the_loader_is_read(tmp_path, monkeypatch):
    from dvd_amd import evaluation, ops
    monkeypatch.chdir(tmp_path)
    model = torch.nn.Linear(1, 1)
    log = types.SimpleNamespace(info=lambda *a: None)
    for attrs, match in (({"severity": 6}, "settings.severity"), ({"severity": -1}, "settings.severity"),
                         ({"severity": True}, "settings.severity"), ({"severity": 2.0}, "settings.severity"),
                         ({"severity": 5, "corruption_number": 19}, "settings.corruption_number"),
                         ({"severity": 1, "corruption_number": -1}, "settings.corruption_number"),
                         ({"severity": 1, "corruption_number": 1.0}, "settings.corruption_number")):
        with pytest.raises(ValueError, match=match):
            evaluation.run_evaluation_docunet(_settings(**attrs), log, _exploding_loader(), None, model, None)
    with pytest.raises(ops.CorruptionUnsupported, match="frost"):
        evaluation.run_evaluation_docunet(_settings(severity=5, corruption_number=8), log, _exploding_loader(), None, model, None)
    assert evaluation.corruption_of(_settings(severity=0, corruption_number=99)) is None      # severity 0: whatever the number
    assert evaluation.corruption_of(_settings()) is None and evaluation.corruption_of(_settings(corruption_number=3)) is None
    assert evaluation.corruption_of(_settings(severity=5)) == (0, 5)
    assert evaluation.corruption_of(_settings(severity=2, corruption_number=16)) == (16, 2)


@pytest.mark.parametrize("attrs", ({}, {"severity": 0, "corruption_number": 0}, {"severity": 0, "corruption_number": 7}))
def test_route_is_unchanged_when_nothing_is_corrupted(attrs, tmp_path, monkeypatch):
    """Severity 0, and absent attributes: run_evaluation_docunet calls prepare_conditioning exactly as before, and
    prepare_conditioning calls of `ops` exactly what it called before - no extra launch."""
    from dvd_amd import evaluation
    monkeypatch.chdir(tmp_path)
    seen, lines = [], []

    def prepare(*args, **kw):
        seen.append((args, kw))
        raise _Stop
    monkeypatch.setattr(evaluation, "prepare_conditioning", prepare)
    doc = {"path": "doc0", "image_u8": np.zeros((40, 56, 3), np.uint8)}
    s = _settings(**attrs)
    with pytest.raises(_Stop):
        evaluation.run_evaluation_docunet(s, types.SimpleNamespace(info=lines.append), [doc], None, torch.nn.Linear(1, 1), None)
    (args, kw), = seen
    assert args[1:] == (torch.device("cpu"), s.env.grid_size, None, bool(s.env.use_init_flow)) and kw == {"decode_png": False}
    assert not any("corruption" in str(line) for line in lines)


class _OpsStub:
    """Records the calls prepare_conditioning makes of `ops`."""

    def __init__(self):
        self.calls = []

    def ingest_u8(self, img, **kw):
        self.calls.append("ingest_u8")
        return torch.zeros(3, 512, 512), img

    def corruption_key(self, seed, path):
        self.calls.append(("corruption_key", seed, path))
        return M.key(seed, path)

    def unit_to_rgb8(self, y):
        self.calls.append("unit_to_rgb8")
        return torch.zeros(y.shape[0], 512, 512, 3, dtype=torch.uint8)

    def corrupt_rgb8(self, img, kind, severity, keys):
        self.calls.append(("corrupt_rgb8", tuple(img.shape), kind, severity, list(keys)))
        return img + 1

    def rgb8_to_unit(self, img):
        self.calls.append("rgb8_to_unit")
        return img.permute(0, 3, 1, 2).float()


def test_stage_sits_between_ingest_and_the_nets(monkeypatch):
    from dvd_amd import evaluation
    docs = lambda: [{"path": f"doc{i}", "image_u8": np.zeros((40, 56, 3), np.uint8)} for i in range(2)]   # noqa: E731
    stub = _OpsStub()
    monkeypatch.setattr(evaluation, "ops", stub)
    with pytest.raises(RuntimeError, match="pre-stage nets are not"):              # the nets come next, and are not loaded
        evaluation.prepare_conditioning(docs(), "cpu", 16, None)
    assert stub.calls == ["ingest_u8", "ingest_u8"]
    stub.calls.clear()
    batch = docs()
    with pytest.raises(RuntimeError, match="pre-stage nets are not"):
        evaluation.prepare_conditioning(batch, "cpu", 16, None, corrupt=(16, 5, 7))
    assert stub.calls == ["ingest_u8", "ingest_u8", ("corruption_key", 7, "doc0"), ("corruption_key", 7, "doc1"), "unit_to_rgb8",
                          ("corrupt_rgb8", (2, 512, 512, 3), 16, 5, [M.key(7, "doc0"), M.key(7, "doc1")]), "rgb8_to_unit"]
    assert all(float(d["y512"].min()) == 1.0 and tuple(d["y512"].shape) == (3, 512, 512) for d in batch)   # the nets see the stage's output
    assert all(not d["src_u8"].any() for d in batch)                                                       # the page's source stays clean
    with pytest.raises(TypeError):
        evaluation.prepare_conditioning(docs(), "cpu", 16, None, False, False, (16, 5, 7))                 # keyword-only


def test_documents_with_ready_conditioning_cannot_be_corrupted(monkeypatch):
    from dvd_amd import evaluation
    monkeypatch.setattr(evaluation, "ops", _OpsStub())
    ready = {k: np.zeros((1, 2, 2), np.float32) for k in ("y512", "mask_cat", "mask_y512", "line_msk")}
    with pytest.raises(ValueError, match="synthetic_00003"):
        evaluation.prepare_conditioning([dict(ready, path="synthetic_00003")], "cpu", 16, None, corrupt=(0, 5, 0))
    assert evaluation.ops.calls == []


# ---- the launcher ---------------------------------------------------------------------------------------------------------
def test_launcher_rounds_names_skips_and_table(tmp_path, monkeypatch, capsys):
    import run_sampling as R
    monkeypatch.chdir(tmp_path)
    assert R.corruption_rounds() == [(0, 0)] and R.corruption_rounds(True) == [(5, c) for c in range(15)]
    assert R.corruption_rounds(True, 3, None) == [(3, 0)] and R.corruption_rounds(False, None, 16) == [(5, 16)]
    assert R.corruption_rounds(True, 2, 11) == [(2, 11)]
    seen = []

    def run(settings):
        seen.append((settings.name, settings.severity, settings.corruption_number))
        settings.ms_ssim = [("a", 0.5 + settings.corruption_number / 100), ("b", 0.7)]
        if settings.corruption_number % 2 == 0:
            settings.ld = [("a", 4.0)]
    monkeypatch.setattr(R, "importlib", types.SimpleNamespace(import_module=lambda name: types.SimpleNamespace(run=run)))
    monkeypatch.setattr(R, "shutil", types.SimpleNamespace(copyfile=lambda *a: None))
    R.run_sampling("dvd", "val_TDiff", 3, "exp", corruption=True)
    out = capsys.readouterr().out
    delivered = [k for k in range(15) if k in M.DELIVERED]
    assert seen == [(f"exp/c{k:02d}_{M.NAMES[k]}_s5", 5, k) for k in delivered]
    for k in range(15):
        assert (f"corruption {k} ({M.NAMES[k]}): no device kernel, round skipped" in out) == (k in M.REFUSED)
    table = (tmp_path / "vis_hp" / "synthetic" / "exp" / "corruption_table.txt").read_text()
    assert table in out
    rows = table.splitlines()
    assert rows[0] == "no kind severity ms_ssim ld" and len(rows) == 1 + len(delivered)
    assert rows[1] == "0 gaussian_noise 5 0.600000 4.000000" and rows[2] == "1 shot_noise 5 0.605000 -"
    seen.clear()
    R.run_sampling("dvd", "val_TDiff", 3, "exp", corruption=False)                     # the clean run, as ever
    R.run_sampling("dvd", "val_TDiff", 3, "exp", severity=2, corruption_number=16)     # one chosen round
    R.run_sampling("dvd", "val_TDiff", 3, "exp", corruption_number=8)
    assert seen == [("exp", 0, 0), ("exp/c16_gaussian_blur_s2", 2, 16)]
    assert "corruption 8 (frost): no device kernel, round skipped" in capsys.readouterr().out
    with pytest.raises(ValueError, match="--severity"):
        R.run_sampling("dvd", "val_TDiff", 3, "exp", severity=6)
    with pytest.raises(ValueError, match="--corruption_number"):
        R.run_sampling("dvd", "val_TDiff", 3, "exp", corruption_number=19)
