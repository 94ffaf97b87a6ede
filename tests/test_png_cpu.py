"""The PNG encoder's container, bounds and argument checks without a GPU (format: DESIGN.md 4.4; kernels: tests/test_gpu_png.py)."""
import ctypes as C
import os
import subprocess
import zlib

import numpy as np
import pytest
import torch

import png_model as P
from host_check import build_host_check
from dvd_amd import lib, ops

ROOT = P.ROOT
S = P.header_segment()


W_BIG = 15447
H_BIG = -(-2 ** 31 // (3 * W_BIG + 1))           # the least h with h * (3w + 1) >= 2^31 at this width


def _rand(h, w, seed=0, hi=256):
    return np.random.RandomState(seed).randint(0, hi, (h, w, 3)).astype(np.uint8)


def test_segment_constant_is_single_sourced():
    assert S == lib.PNG_SEGMENT and 64 <= S <= 32768


@pytest.mark.parametrize("h,w,segment", [(1, 1, S), (2, 2, S), (7, 5, 16), (7, 5, 17), (33, 21, 100), (120, 100, S)],
                         ids=lambda v: str(v))
def test_model_file_of_literal_segments_decodes(h, w, segment):
    """Segmenting, the empty stored blocks between segments, one IDAT per segment and the folded Adler-32 give a file that PIL
    and zlib accept - with segments far smaller than the real one, cut inside rows and inside a filter byte's row."""
    img = _rand(h, w, seed=h * 131 + w)
    img[h // 2:] //= 3                            # literals on both sides of 144: 8-bit and 9-bit codes
    data = P.model_file(img, segment)
    P.check_png(data, img, segment, limit=P.bound(h, w, segment))


def test_model_bound_is_the_literal_file_with_9_bits_for_every_byte():
    """The literal-only file's length is known exactly from the stream: per segment 10 + 8 n8 + 9 n9 bits rounded up to bytes,
    then the stored block.  The bound is that expression with every byte at 9 bits and the stored block at its longest (5
    bytes), so no literal-only file exceeds it - and the library's bound is the model's."""
    for h, w in ((1, 1), (1, 7), (1, 12000), (97, 131), (200, 333), (3508, 2480)):
        assert lib.raw().dvd_png_bound(h, w) == P.bound(h, w, S)
    img = _rand(3, 12000, seed=9)
    img[:, ::2] |= 0x90                           # many bytes of 144 and above
    data = P.model_file(img, S)
    P.check_png(data, img, S, limit=P.bound(3, 12000, S))
    stream = np.frombuffer(P.filter_rows(img)[1], np.uint8)
    want, nseg = 8 + 25 + 12 + 2 + 2 + 4, -(-len(stream) // S)
    for k in range(nseg):
        seg = stream[k * S:(k + 1) * S]
        bits = 10 + 8 * int((seg < 144).sum()) + 9 * int((seg >= 144).sum())
        want += 12 + -(-(bits + 3) // 8) + 4      # the stored block's 3 header bits, padded, then 00 00 FF FF
    assert len(data) == want and int((stream >= 144).sum()) > len(stream) // 3


def test_adler_folding_matches_zlib_on_random_splits():
    rng = np.random.RandomState(5)
    for trial in range(40):
        n = int(rng.randint(1, 200000))
        data = (np.full(n, 255, np.uint8) if trial % 4 == 0 else rng.randint(0, 256, n).astype(np.uint8)).tobytes()
        cuts = sorted(set(rng.randint(0, n + 1, int(rng.randint(0, 12))).tolist() + [0, n]))
        if trial % 3 == 0:
            cuts = sorted(set(cuts + [1, n - 1]) & set(range(n + 1)))            # segments of length 1 at both ends
        segs = [data[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
        assert b"".join(segs) == data
        assert P.adler_of_segments(segs) == zlib.adler32(data)
    # sums that wrap 65521 inside one fold: 70 000 bytes of 255 in three segments, one of them a single byte
    data = b"\xff" * 70000
    assert P.adler_of_segments([data[:1], data[1:65522], data[65522:]]) == zlib.adler32(data)


def test_size_queries_and_argument_checks_need_no_gpu():
    raw = lib.raw()
    err = lambda: raw.dvd_last_error().decode()  # noqa: E731
    for fn in (raw.dvd_png_bound, raw.dvd_png_scratch_bytes):
        assert fn(0, 5) == -1 and fn(5, 0) == -1 and fn(-3, 5) == -1
        assert fn(H_BIG, W_BIG) == -1 and "2^31" in err()
        assert fn(H_BIG - 1, W_BIG) > 0
        assert fn(2 ** 31 - 1, 2 ** 31 - 1) == -1                    # no overflow on the way to the answer
    assert raw.dvd_png_bound(1, 1) == 8 + 25 + 12 + (10 + 9 * 4 + 7) // 8 + 5 + 2 + 2 + 4 + 12
    assert raw.dvd_png_scratch_bytes(3508, 2480) >= 3508 * 7441
    fake = C.c_void_p(1 << 20)                     # never dereferenced: every check below fails before a launch
    enc = lambda *a: raw.dvd_png_encode_rgb8(*a)  # noqa: E731
    bound = raw.dvd_png_bound(4, 4)
    for args in ((None, 4, 4, fake, bound, fake, fake, None), (fake, 4, 4, None, bound, fake, fake, None),
                 (fake, 4, 4, fake, bound, None, fake, None), (fake, 4, 4, fake, bound, fake, None, None)):
        assert enc(*args) == -1 and "null" in err()
    assert enc(fake, 0, 4, fake, bound, fake, fake, None) == -1 and "h >= 1" in err()
    assert enc(fake, 4, 0, fake, bound, fake, fake, None) == -1 and "w >= 1" in err()
    assert enc(fake, H_BIG, W_BIG, fake, 1 << 40, fake, fake, None) == -1 and "too large" in err()
    assert enc(fake, 4, 4, fake, bound - 1, fake, fake, None) == -1 and "cap" in err() and "dvd_png_bound" in err()
    assert enc(fake, 4, 4, fake, 0, fake, fake, None) == -1 and "cap" in err()


def test_ops_png_encode_rejects_bad_input_with_valueerror():
    good = torch.zeros(4, 5, 3, dtype=torch.uint8)
    for bad in (good.float(), good[:, ::2], good.permute(1, 0, 2), torch.zeros(4, 5, 4, dtype=torch.uint8),
                torch.zeros(4, 5, dtype=torch.uint8), torch.zeros(0, 5, 3, dtype=torch.uint8)):
        with pytest.raises(ValueError):
            ops.png_encode(bad)
        with pytest.raises(ValueError):
            ops.png_encode_to_file(bad, "never_written.png")
    assert not os.path.exists("never_written.png")
    assert ops.png_bound(4, 5) == P.bound(4, 5, S)


def test_pil_route_writes_image_save_bytes(tmp_path, monkeypatch):
    """'pil' is the code as it was: the file holds Image.save's bytes."""
    import io
    from PIL import Image
    import admin.settings as ws
    from utils_flow.visualization_utils import visualize_dewarping
    monkeypatch.chdir(tmp_path)
    s = ws.Settings()
    s.name = "pytest_png"
    page = _rand(40, 56, seed=3)
    ret = visualize_dewarping(s, None, None, 0, None, ["/x/page_7.jpg"], warped_u8=page)
    want = io.BytesIO()
    Image.fromarray(page).save(want, format="PNG")
    path = tmp_path / "vis_hp" / s.env.eval_dataset_name / "pytest_png" / "dewarped_pred" / "warped_page_7.png"
    assert path.read_bytes() == want.getvalue() and isinstance(ret, np.ndarray) and np.array_equal(ret, page)


# ---- the CPU restatement of the kernels' arithmetic, under AddressSanitizer and UBSan ------------------------------------------
@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    """dvd_amd/csrc/png_host_check.cpp: png.hip's filter, segment compressor, bit writer, layout and CRC tree on the shared
    png_core.h, as a stand-alone program with exact-size buffers."""
    return build_host_check("png", tmp_path_factory.mktemp("png_host"))


def _host_encode(exe, img, tmp_path):
    h, w, _ = img.shape
    img.tofile(tmp_path / "in.rgb")
    r = subprocess.run([str(exe), str(h), str(w), str(tmp_path / "in.rgb"), str(tmp_path / "out.png")], capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return (tmp_path / "out.png").read_bytes()


def _stream_shape(nbytes):
    """(h, w) with h * (3w + 1) == nbytes, the widest such image."""
    for w in range((nbytes - 1) // 3, 0, -1):
        if nbytes % (3 * w + 1) == 0:
            return nbytes // (3 * w + 1), w
    raise AssertionError(nbytes)


def test_host_restatement_under_sanitizers(host_check, tmp_path):
    """Every shape class of the GPU file at once: tiny images, a stream of S - 1 / S / S + 1 bytes, matches across segment
    boundaries (period 5), the incompressible case against the bound, an all-zero image under the 2 % cap."""
    cases = {f"rand{h}x{w}": _rand(h, w, seed=h + w) for h, w in ((1, 1), (1, 7), (7, 1), (2, 2), (97, 131))}
    for n in (S - 1, S, S + 1):
        h, w = _stream_shape(n)
        cases[f"stream{n}"] = _rand(h, w, seed=n, hi=4)
    cases["period5"] = (np.arange(200 * 333 * 3) % 5 * 50).astype(np.uint8).reshape(200, 333, 3)
    cases["zeros"] = np.zeros((256, 256, 3), np.uint8)
    for name, img in cases.items():
        data = _host_encode(host_check, img, tmp_path)
        P.check_png(data, img, S, limit=lib.raw().dvd_png_bound(img.shape[0], img.shape[1]))
        if name == "zeros":
            assert len(data) <= 0.02 * img.size, len(data)
