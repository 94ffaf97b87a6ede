"""The JPEG encoder's format, bounds, argument checks and settings without a GPU (format: DESIGN.md 4.5; kernels:
tests/test_gpu_jpeg.py).  The model (tests/jpeg_model.py) is held to PIL here - its files decode, its tables are PIL's, its
fidelity and size are PIL's within measured bars - and the CPU restatement of the kernels' arithmetic, built under ASan/UBSan,
is held to the model byte for byte."""
import ctypes as C
import io
import os
import subprocess

import numpy as np
import pytest
import torch
from PIL import Image

import jpeg_model as J
from host_check import build_host_check
from dvd_amd import lib, ops

ROOT = J.ROOT
SS = ("420", "444")
PIL_SUBSAMPLING = {"420": 2, "444": 0}


def _pil_file(img, quality, subsampling, **kw):
    out = io.BytesIO()
    Image.fromarray(img).save(out, format="JPEG", quality=quality, subsampling=PIL_SUBSAMPLING[subsampling], optimize=False, **kw)
    return out.getvalue()


def _psnr(a, b):
    return 10 * np.log10(255.0 ** 2 / np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))


# ---- 1. the model's files decode ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("subsampling", SS)
@pytest.mark.parametrize("h,w", J.SHAPES, ids=lambda v: str(v))
def test_model_file_decodes_with_pil(h, w, subsampling):
    """check_jpeg: marker order, tables, DRI, RST sequence, stuffing, every interval Huffman-decoded back to the model's
    coefficients ending on 1-bit padding, PIL's mode and size.  Then PIL's pixels: at quality 100 in 4:4:4 the decoded image is
    the input within the rounding of the colour transform and Q = 1 (measured: at most 4 levels on noise)."""
    img = J.noise_image(h, w, seed=h * 131 + w)
    data = J.model_file(img, 100, subsampling)
    intervals = J.check_jpeg(data, img, 100, subsampling)
    assert len(data) <= J.bound(h, w, subsampling)
    if (h, w, subsampling) == (80, 8, "444"):
        assert len(intervals) == 10 and b"\xff\xd7" + intervals[8] + b"\xff\xd0" + intervals[9] + b"\xff\xd9" in data
    if (h, w, subsampling) == (8, 4104, "444"):
        assert len(intervals) == 1 and J.geometry(h, w, subsampling)[1] == 513
    if subsampling == "444":
        got = np.asarray(Image.open(io.BytesIO(data)).convert("RGB")).astype(int)
        assert np.abs(got - img).max() <= 6


def test_model_tables_are_pils():
    """The quantisation tables at every tested quality and the four Huffman tables are the ones PIL (libjpeg: Annex K, the usual
    quality rule) writes into its own files."""
    img = J.noise_image(16, 16, seed=1)
    for quality in (1, 30, 49, 50, 75, 90, 100):
        ours = J.parse_tables(J.split_file(J.model_file(img, quality, "420"))[0])
        pil = J.parse_tables(J.split_file(_pil_file(img, quality, "420", restart_marker_rows=1))[0])
        assert ours[0] == pil[0], quality
        assert ours[1] == pil[1] and len(ours[1]) == 4


# ---- 2. stuffing, ZRL, EOB ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("subsampling", SS)
def test_stress_inputs_exercise_stuffing_zrl_and_eob(subsampling):
    cases = J.stress_cases()
    img, quality = cases["noise_q100"]
    stats = {}
    data = J.model_file(img, quality, subsampling, stats)
    assert stats["stuffed"] >= 1 and stats["zrl"] >= 1, stats
    assert data.count(b"\xff\x00") >= stats["stuffed"]
    J.check_jpeg(data, img, quality, subsampling)
    img, quality = cases["smooth_q30"]
    stats = {}
    data = J.model_file(img, quality, subsampling, stats)
    blocks = np.prod(J.coefficients(img, quality, subsampling).shape[:3])
    assert stats["eob"] >= 0.9 * blocks, (stats, blocks)          # nearly every block ends in a long zero run
    J.check_jpeg(data, img, quality, subsampling)


# ---- 3. the CPU restatement of the kernels' arithmetic, under AddressSanitizer and UBSan --------------------------------------
@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    """dvd_amd/csrc/jpeg_host_check.cpp: jpeg.hip's transform, tiles, emitter, stuffing, layout and gather on the shared
    jpeg_core.h, as a stand-alone program with exact-size buffers."""
    return build_host_check("jpeg", tmp_path_factory.mktemp("jpeg_host"))


def _host_encode(exe, img, quality, subsampling, tmp_path):
    h, w, _ = img.shape
    img.tofile(tmp_path / "in.rgb")
    r = subprocess.run([str(exe), str(h), str(w), str(quality), subsampling, str(tmp_path / "in.rgb"), str(tmp_path / "out.jpg")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return (tmp_path / "out.jpg").read_bytes()


@pytest.mark.parametrize("subsampling", SS)
def test_host_restatement_equals_the_model_under_sanitizers(host_check, tmp_path, subsampling):
    inputs = {f"{h}x{w}": J.noise_image(h, w, seed=h * 131 + w) for h, w in J.SHAPES}
    inputs.update({name: img for name, (img, _) in J.stress_cases().items()})
    raw = lib.raw()
    for name, img in inputs.items():
        h, w, _ = img.shape
        for quality in J.QUALITIES:
            data = _host_encode(host_check, img, quality, subsampling, tmp_path)
            assert data == J.model_file(img, quality, subsampling), (name, quality)
            assert len(data) <= raw.dvd_jpeg_bound(h, w, J.SUBSAMPLINGS[subsampling])
    for name, (img, quality) in J.stress_cases().items():
        assert _host_encode(host_check, img, quality, subsampling, tmp_path) == J.model_file(img, quality, subsampling), name


# ---- 4. bounds, scratch sizes, argument refusals ------------------------------------------------------------------------------
def test_bound_is_the_models_and_covers_every_file():
    raw = lib.raw()
    for subsampling, flag in J.SUBSAMPLINGS.items():
        for h, w in J.SHAPES + [(120, 100), (700, 500), (3508, 2480), (65535, 8), (8, 65535)]:
            assert raw.dvd_jpeg_bound(h, w, flag) == J.bound(h, w, subsampling) == ops.jpeg_bound(h, w, subsampling)
        # the closed form at 1 x 1: the header, one interval of 6 / 3 blocks at 1723 bits rounded up to words, stuffed, EOI
        blocks = 6 if subsampling == "420" else 3
        assert raw.dvd_jpeg_bound(1, 1, flag) == 613 + 2 * ((blocks * 1723 + 31) // 32 * 4) + 2
        for name, (img, quality) in J.stress_cases().items():
            assert len(J.model_file(img, quality, subsampling)) <= J.bound(img.shape[0], img.shape[1], subsampling)
    assert J.BLOCK_BITS_MAX == 1723
    assert max(length for t in J.DC_CODES for _, length in t.values()) == 11
    assert max(length for t in J.AC_CODES for _, length in t.values()) == 16


def test_size_queries_and_argument_checks_need_no_gpu():
    raw = lib.raw()
    err = lambda: raw.dvd_last_error().decode()  # noqa: E731
    for fn in (raw.dvd_jpeg_bound, raw.dvd_jpeg_scratch_bytes):
        for flag in (lib.JPEG_420, lib.JPEG_444):
            assert fn(0, 5, flag) == -1 and fn(5, 0, flag) == -1 and fn(-3, 5, flag) == -1
            assert fn(65536, 8, flag) == -1 and fn(8, 65536, flag) == -1 and "65535" in err()
            assert fn(26768, 26768, flag) == -1 and "2^31" in err()          # 3 * 26768^2 = 2^31 + 2.1e6
            assert fn(26768, 26736, flag) > 0                                # 3 * 26768 * 26736 = 2^31 - 4.8e5
            assert fn(2 ** 31 - 1, 2 ** 31 - 1, flag) == -1                  # no overflow on the way to the answer
            assert fn(65535, 8, flag) > 0 and fn(8, 65535, flag) > 0
        assert fn(8, 8, 2) == -1 and "subsampling" in err()
        assert fn(8, 8, -1) == -1 and "subsampling" in err()
    # coefficients (2 bytes each) and, per interval, a slot of twice its worst-case bytes
    assert raw.dvd_jpeg_scratch_bytes(3508, 2480, lib.JPEG_420) >= 220 * 155 * 6 * 128 + 220 * 2 * (155 * 6 * 1723 // 8)
    fake = C.c_void_p(1 << 20)                     # never dereferenced: every check below fails before a launch
    odd = C.c_void_p((1 << 20) + 8)
    enc = lambda *a: raw.dvd_jpeg_encode_rgb8(*a)  # noqa: E731
    bound = raw.dvd_jpeg_bound(4, 4, lib.JPEG_420)
    for args in ((None, 4, 4, 90, 0, fake, bound, fake, fake, None), (fake, 4, 4, 90, 0, None, bound, fake, fake, None),
                 (fake, 4, 4, 90, 0, fake, bound, None, fake, None), (fake, 4, 4, 90, 0, fake, bound, fake, None, None)):
        assert enc(*args) == -1 and "null" in err()
    assert enc(fake, 0, 4, 90, 0, fake, bound, fake, fake, None) == -1 and "h >= 1" in err()
    assert enc(fake, 4, 0, 90, 0, fake, bound, fake, fake, None) == -1 and "w >= 1" in err()
    assert enc(fake, 26768, 26768, 90, 0, fake, 1 << 40, fake, fake, None) == -1 and "too large" in err()
    assert enc(fake, 65536, 4, 90, 0, fake, 1 << 40, fake, fake, None) == -1 and "too large" in err()
    for quality in (0, 101, -5):
        assert enc(fake, 4, 4, quality, 0, fake, bound, fake, fake, None) == -1 and "quality" in err()
    assert enc(fake, 4, 4, 90, 2, fake, bound, fake, fake, None) == -1 and "subsampling" in err()
    assert enc(fake, 4, 4, 90, 0, fake, bound - 1, fake, fake, None) == -1 and "cap" in err() and "dvd_jpeg_bound" in err()
    assert enc(fake, 4, 4, 90, 0, fake, 0, fake, fake, None) == -1 and "cap" in err()
    assert enc(fake, 4, 4, 90, 0, fake, bound, fake, odd, None) == -1 and "aligned" in err()


def test_ops_jpeg_encode_rejects_bad_input_with_valueerror():
    good = torch.zeros(4, 5, 3, dtype=torch.uint8)
    for bad in (good.float(), good[:, ::2], good.permute(1, 0, 2), torch.zeros(4, 5, 4, dtype=torch.uint8),
                torch.zeros(4, 5, dtype=torch.uint8), torch.zeros(0, 5, 3, dtype=torch.uint8)):
        with pytest.raises(ValueError):
            ops.jpeg_encode(bad)
        with pytest.raises(ValueError):
            ops.jpeg_encode_to_file(bad, "never_written.jpg")
    for kw in ({"quality": 0}, {"quality": 101}, {"quality": 90.0}, {"quality": True}, {"subsampling": "422"}, {"subsampling": 420}):
        with pytest.raises(ValueError):
            ops.jpeg_encode(good, **kw)
        with pytest.raises(ValueError):
            ops.jpeg_encode_to_file(good, "never_written.jpg", **kw)
    assert not os.path.exists("never_written.jpg")


# ---- 5. fidelity and size against PIL -----------------------------------------------------------------------------------------
# Measured on these twelve cases: the model's PSNR against the source is below PIL's by at most 0.0598 dB
# (smooth page, quality 90; on the bars and noisy pages between -0.008 and +0.003 dB), and its file is at most 1.0248 x PIL's
# with restart_marker_rows=1 (smooth page, quality 90, 4:2:0; bars and noisy pages 0.9995 .. 1.0047).  The pipelines are not
# coefficient-identical (libjpeg's DCT keeps other intermediate precision and its 2 x 2 average alternates its rounding bias),
# so the bars are the issue's rule: twice the measured deficit, and the measured ratio plus 1 %.
PSNR_BAR_DB = 2 * 0.0598
SIZE_BAR = 1.0248 + 0.01


@pytest.fixture(scope="module")
def pages():
    return {kind: J.synthetic_page(kind) for kind in ("smooth", "bars", "noisy")}


@pytest.mark.parametrize("subsampling", SS)
@pytest.mark.parametrize("quality", (75, 90))
@pytest.mark.parametrize("kind", ("smooth", "bars", "noisy"))
def test_fidelity_and_size_against_pil(pages, kind, quality, subsampling):
    img = pages[kind]
    assert img.shape == (700, 500, 3)
    ours = J.model_file(img, quality, subsampling)
    pil = _pil_file(img, quality, subsampling, restart_marker_rows=1)
    assert pil.count(b"\xff\xd0") >= 1                            # PIL did write restart markers
    psnr_ours = _psnr(np.asarray(Image.open(io.BytesIO(ours)).convert("RGB")), img)
    psnr_pil = _psnr(np.asarray(Image.open(io.BytesIO(pil)).convert("RGB")), img)
    print(f"{kind} q{quality} {subsampling}: PSNR {psnr_ours:.4f} dB (PIL {psnr_pil:.4f}, deficit {psnr_pil - psnr_ours:+.4f}), "
          f"{len(ours)} bytes (PIL {len(pil)}, ratio {len(ours) / len(pil):.5f})")
    assert psnr_pil - psnr_ours <= PSNR_BAR_DB
    assert len(ours) <= SIZE_BAR * len(pil)


# ---- 6. settings --------------------------------------------------------------------------------------------------------------
def test_defaults_write_the_same_png_as_before(tmp_path, monkeypatch):
    """page_format 'png' is the code as it was: warped_<stem>.png holds Image.save's bytes and nothing else is written."""
    import admin.settings as ws
    from utils_flow.visualization_utils import visualize_dewarping
    monkeypatch.chdir(tmp_path)
    s = ws.Settings()
    s.name = "pytest_jpeg"
    page = J.noise_image(40, 56, seed=3)
    ret = visualize_dewarping(s, None, None, 0, None, ["/x/page_7.jpg"], warped_u8=page)
    want = io.BytesIO()
    Image.fromarray(page).save(want, format="PNG")
    out_dir = tmp_path / "vis_hp" / s.env.eval_dataset_name / "pytest_jpeg" / "dewarped_pred"
    assert [p.name for p in out_dir.iterdir()] == ["warped_page_7.png"]
    assert (out_dir / "warped_page_7.png").read_bytes() == want.getvalue()
    assert isinstance(ret, np.ndarray) and np.array_equal(ret, page)
