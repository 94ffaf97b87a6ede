"""The JPEG decoder without a GPU (definition: DESIGN.md 4.6; kernels: tests/test_gpu_jpegdec.py).  The model
(tests/jpegdec_model.py) is held to PIL byte for byte; the CPU restatement of the kernels' arithmetic
(dvd_amd/csrc/jpegdec_host_check.cpp on jpegdec_core.h), built under ASan/UBSan, is held to the model - pixels and fixpoint
iterations - and must end with a status, never a sanitizer report, on damaged scans; the header check's refusals, the
argument checks, the setting and the loader need no GPU either."""
import ctypes as C
import io
import os
import struct
import subprocess

import numpy as np
import pytest
import torch
from PIL import Image

import jpeg_model as J
import jpegdec_model as M
from host_check import build_host_check
from dvd_amd import lib, ops

ROOT = J.ROOT


@pytest.fixture(scope="module")
def grid():
    """name -> (file, PIL's pixels, the model's pixels, the model's iterations): computed once, shared and left unchanged"""
    out = {}
    for name, data in M.grid().items():
        px, iters = M.decode(data)
        out[name] = (data, M.pil_pixels(data), px, iters)
    return out


# ---- 1. the model is PIL ------------------------------------------------------------------------------------------------------
def test_model_equals_pil_on_the_grid(grid):
    """9 sizes x noise / page x (quality 5..100, 4:4:4 / 4:2:2 / 4:2:0 / gray, optimize, restart rows, restart blocks)"""
    assert len(grid) == 126
    for name, (data, want, got, iters) in grid.items():
        assert got.shape == want.shape and np.array_equal(got, want), name
        assert iters >= 1


@pytest.mark.parametrize("h,w", [(17, 5), (37, 53)])
def test_model_orientations(h, w):
    img = M.content("noise", h, w)
    for o in range(1, 9):
        data = M.oriented_file(img, o)
        assert ops.jpeg_probe(data)["orientation"] == o
        want = M.pil_pixels(data)
        assert want.shape == ((w, h, 3) if o >= 5 else (h, w, 3))
        assert np.array_equal(M.decode(data)[0], want), o
    for order in ("<", ">"):                                # both byte orders, written by hand
        tiff = (b"II*\0" if order == "<" else b"MM\0*") + struct.pack(order + "IH", 8, 1) + struct.pack(order + "HHIHH", 0x0112, 3, 1, 6, 0) + b"\0\0\0\0"
        plain = M.pil_file(img, 90, 2)
        app1 = b"\xff\xe1" + struct.pack(">H", 2 + 6 + len(tiff)) + b"Exif\0\0" + tiff
        data = plain[:2] + app1 + plain[2:]
        assert ops.jpeg_probe(data)["orientation"] == 6
        assert np.array_equal(M.decode(data)[0], M.pil_pixels(data))


@pytest.mark.parametrize("subsampling", ("420", "444"))
def test_model_decodes_the_encoder_models_files(subsampling):
    """This project's own encoder (one restart interval per MCU row, Annex K tables)"""
    for h, w in ((9, 17), (33, 47), (80, 8)):
        data = J.model_file(J.noise_image(h, w, seed=h + w), 90, subsampling)
        assert np.array_equal(M.decode(data)[0], M.pil_pixels(data)), (h, w)


def test_fixpoint_synchronises_within_64_iterations():
    """The page the GPU test uses: hundreds of subsequences start from guesses and fall into step; the states the fixpoint
    ends in give the blocks of one sequential walk."""
    data = M.sync_page()
    hd = M.parse(data)
    E, iters = M.fixpoint(hd)
    print(f"300 x 400 noisy page, q90, 4:2:0: {len(hd['scan'])} scan bytes, {len(E) - 1} subsequences, {iters} iterations")
    assert len(E) - 1 > 300 and 1 < iters <= 64
    assert np.array_equal(M.coefficients(hd, E), M.coefficients(hd, None))
    assert M.fixpoint(hd, max_iters=2) == (None, 2)
    assert np.array_equal(M.decode(data)[0], M.pil_pixels(data))
    for make in (M.sync_noise, M.flat_file):
        data = make()
        px, iters = M.decode(data)
        print(f"{make.__name__}: {iters} iterations")
        assert np.array_equal(px, M.pil_pixels(data)) and 1 < iters <= 64


# ---- 2. the CPU restatement of the kernels' arithmetic, under AddressSanitizer and UBSan --------------------------------------
@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    return build_host_check("jpegdec", tmp_path_factory.mktemp("jpegdec_host"))


def _host_decode(exe, data, tmp_path, max_iters=None):
    """(status, iterations, pixels or None); a sanitizer report ends the program with another exit status and fails here"""
    (tmp_path / "in.jpg").write_bytes(data)
    args = [str(exe), str(tmp_path / "in.jpg"), str(tmp_path / "out.rgb")] + ([str(max_iters)] if max_iters else [])
    r = subprocess.run(args, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    status, iters, oh, ow = (int(v) for v in r.stdout.split())
    if status:
        return status, iters, None
    return status, iters, np.fromfile(tmp_path / "out.rgb", dtype=np.uint8).reshape(oh, ow, 3)


def test_host_restatement_equals_the_model_under_sanitizers(host_check, tmp_path, grid):
    for name, (data, _, want, want_iters) in grid.items():
        status, iters, got = _host_decode(host_check, data, tmp_path)
        assert status == 0 and got.shape == want.shape and np.array_equal(got, want), name
        assert iters == want_iters, name
    img = M.content("noise", 17, 5)
    for o in range(1, 9):
        data = M.oriented_file(img, o)
        assert np.array_equal(_host_decode(host_check, data, tmp_path)[2], M.decode(data)[0]), o
    for data in (M.sync_page(), M.flat_file(), J.model_file(J.noise_image(33, 47, seed=5), 90, "420")):
        want, want_iters = M.decode(data)
        status, iters, got = _host_decode(host_check, data, tmp_path)
        assert status == 0 and iters == want_iters and np.array_equal(got, want)
    assert _host_decode(host_check, M.sync_page(), tmp_path, max_iters=2)[:2] == (-34, 2)       # DVD_E_JPEG_NOSYNC


def test_host_restatement_survives_damaged_scans(host_check, tmp_path):
    """Truncated at every 97th byte of the scan, and 200 seeded random byte flips (100 in a plain file, 100 in one with
    restart markers, one byte each; then all of a file's at once): a status every time - 0 where the damage still decodes,
    DATA mostly - and never a sanitizer report.  CPU only: no GPU test feeds corrupt data."""
    plain = M.pil_file(M.content("noise", 37, 53), 90, 2)
    rst = M.pil_file(M.content("page", 64, 49), 90, 1, restart_marker_blocks=3)
    seen = set()
    for data in (plain, rst):
        info = ops.jpeg_probe(data)
        lo, n = info["scan_offset"], info["scan_bytes"]
        for cut in range(lo, lo + n, 97):
            seen.add(_host_decode(host_check, data[:cut], tmp_path)[0])
        rng = np.random.RandomState(len(data))
        all_flips = bytearray(data)
        for _ in range(100):
            pos, val = lo + int(rng.randint(n)), int(rng.randint(256))
            one = bytearray(data)
            one[pos] = all_flips[pos] = val
            seen.add(_host_decode(host_check, bytes(one), tmp_path)[0])
        seen.add(_host_decode(host_check, bytes(all_flips), tmp_path)[0])
    print("statuses seen:", sorted(seen))
    assert seen <= {0} | set(lib.JPEG_DECODE_CODES) and -35 in seen


# ---- 3. the header check: refusals, the probe, argument checks ----------------------------------------------------------------
def _segments(data):
    """[(marker, payload)] up to and including SOS, and the rest of the file (scan + EOI)"""
    segs, i = [], 2
    while True:
        m, n = data[i + 1], struct.unpack(">H", data[i + 2:i + 4])[0]
        segs.append((m, data[i + 4:i + 2 + n]))
        i += 2 + n
        if m == 0xDA:
            return segs, data[i:]


def _join(segs, rest):
    return b"\xff\xd8" + b"".join(b"\xff" + bytes([m]) + struct.pack(">H", len(p) + 2) + p for m, p in segs) + rest


def _patched(data, marker, fn, which=0):
    """the file with fn(payload) in place of the payload of the which-th segment `marker` (None: the segment is dropped)"""
    segs, rest = _segments(data)
    idx = [i for i, (m, _) in enumerate(segs) if m == marker][which]
    new = fn(bytearray(segs[idx][1]))
    segs = segs[:idx] + ([(marker, bytes(new))] if new is not None else []) + segs[idx + 1:]
    return _join(segs, rest)


def _set(index, value):
    def fn(p):
        p[index] = value
        return p
    return fn


def _refusal_cases():
    img = M.content("page", 33, 48)
    base = M.pil_file(img, 90, 2)
    segs, rest = _segments(base)
    cases = {}
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, format="JPEG", progressive=True)
    cases["progressive (PIL)"] = (buf.getvalue(), "PROGRESSIVE")
    buf = io.BytesIO()
    Image.fromarray(img).convert("CMYK").save(buf, format="JPEG")
    cases["CMYK (PIL)"] = (buf.getvalue(), "COMPONENTS")
    for keyword, luma in (("4:4:0", 0x12), ("4:1:1", 0x41)):
        if keyword == "4:4:0":                              # Pillow's "4:1:1" keyword writes 4:2:0 (kept "for compatibility")
            try:
                cases[f"{keyword} (PIL)"] = (M.pil_file(img, 90, keyword), "SAMPLING")
            except (ValueError, TypeError, KeyError, OSError):
                pass
        cases[f"{keyword} (SOF patched)"] = (_patched(base, 0xC0, _set(7, luma)), "SAMPLING")
    cases["luma below chroma"] = (_patched(_patched(base, 0xC0, _set(7, 0x11)), 0xC0, _set(10, 0x21)), "SAMPLING")
    for marker, code in ((0xC1, "EXTENDED"), (0xC3, "LOSSLESS"), (0xC9, "ARITHMETIC"), (0xCA, "ARITHMETIC")):
        cases[f"SOF{marker - 0xC0}"] = (_join([(marker if m == 0xC0 else m, p) for m, p in segs], rest), code)
    cases["12-bit samples"] = (_patched(base, 0xC0, _set(0, 12)), "PRECISION")
    cases["3 h w >= 2^31"] = (_patched(base, 0xC0, lambda p: p[:1] + struct.pack(">HH", 30000, 30000) + p[5:]), "SIZE")
    adobe = (0xEE, b"Adobe" + struct.pack(">HHHB", 100, 0, 0, 0))
    cases["Adobe transform 0"] = (_join([adobe] + segs, rest), "ADOBE")
    no_jfif = [(m, p) for m, p in segs if m != 0xE0]
    rgb_ids = _join(no_jfif, rest)
    for k, cid in enumerate(b"RGB"):
        rgb_ids = _patched(_patched(rgb_ids, 0xC0, _set(6 + 3 * k, cid)), 0xDA, _set(1 + 2 * k, cid))
    cases["ids R G B without JFIF"] = (rgb_ids, "COMPONENTS")
    second = b"\xff\xda" + struct.pack(">H", 8) + bytes([1, 1, 0x00, 0, 63, 0]) + b"\x12\x34"
    cases["two scans"] = (base[:-2] + second + b"\xff\xd9", "SCANS")
    cases["a scan of one component of three"] = (_patched(base, 0xDA, lambda p: bytes([1]) + p[1:3] + p[7:]), "SCANS")
    cases["16-bit quantisation table"] = (_patched(base, 0xDB, lambda p: bytes([0x10 | p[0]]) + b"".join(b"\0" + bytes([v]) for v in p[1:65]) + p[65:]), "QUANT16")
    dqt = [i for i, (m, _) in enumerate(segs) if m == 0xDB]
    n_dht = sum(1 for m, _ in segs if m == 0xC4)
    cases["a missing quantisation table"] = (_patched(base, 0xDB, lambda p: None if len(dqt) > 1 else p[:65], which=len(dqt) - 1), "TABLE")
    cases["a missing Huffman table"] = (_patched(base, 0xC4, lambda p: None if n_dht > 1 else p[:17 + sum(p[1:17])], which=n_dht - 1), "TABLE")
    cases["a truncated header"] = (base[:200], "HEADER")
    cases["not a JPEG"] = (b"\x89PNG\r\n\x1a\n" + bytes(40), "HEADER")
    return cases


REFUSALS = _refusal_cases()


@pytest.mark.parametrize("name", list(REFUSALS))
def test_refusals_are_decided_on_the_host(name):
    """Each with its own code, from the probe and from the decode entry point alike - the latter with device pointers that are
    never dereferenced: nothing is launched."""
    data, code = REFUSALS[name]
    number = {v: k for k, v in lib.JPEG_DECODE_CODES.items()}[code]
    raw = lib.raw()
    host = np.frombuffer(bytearray(data), dtype=np.uint8)
    info = lib.JpegDecInfo()
    assert raw.dvd_jpegdec_probe(C.c_void_p(host.ctypes.data), host.size, C.byref(info)) == number
    assert b"refused" in raw.dvd_last_error()
    fake = C.c_void_p(1 << 20)
    iters = C.c_int(-1)
    assert raw.dvd_jpeg_decode_rgb8(C.c_void_p(host.ctypes.data), fake, host.size, fake, 1 << 40, 0, C.byref(iters), fake, None) == number
    with pytest.raises(ops.JpegUnsupported, match=code) as e:
        ops.jpeg_probe(data)
    assert e.value.code == code and isinstance(e.value, ValueError)
    with pytest.raises(ops.JpegUnsupported, match=code):
        ops.jpeg_decode(data)                               # refused before a device is looked for


def test_refusal_codes_are_distinct():
    codes = {code for _, code in REFUSALS.values()}
    assert {"PROGRESSIVE", "EXTENDED", "LOSSLESS", "ARITHMETIC", "PRECISION", "COMPONENTS", "ADOBE", "SAMPLING", "SCANS", "QUANT16",
            "TABLE", "HEADER", "SIZE"} <= codes
    assert len(set(lib.JPEG_DECODE_CODES)) == len(set(lib.JPEG_DECODE_CODES.values())) == 16
    text = open(os.path.join(ROOT, "include", "dvd_hip.h")).read()
    for number, name in lib.JPEG_DECODE_CODES.items():
        assert f"#define DVD_E_JPEG_{name} ({number})" in text


def test_probe_reads_the_header():
    img = M.content("page", 37, 53)
    for ss, (hs, vs, bpm) in {0: (1, 1, 3), 1: (2, 1, 4), 2: (2, 2, 6)}.items():
        data = M.pil_file(img, 90, ss, restart_marker_rows=1)
        info = ops.jpeg_probe(data)
        mx, my = -(-53 // (8 * hs)), -(-37 // (8 * vs))
        assert (info["h"], info["w"], info["out_h"], info["out_w"], info["components"], info["hs"], info["vs"]) == (37, 53, 37, 53, 3, hs, vs)
        assert info["restart_interval"] == mx and info["blocks"] == mx * my * bpm and info["orientation"] == 1
        lo, n = info["scan_offset"], info["scan_bytes"]
        assert data[lo - 14:lo - 12] == b"\xff\xda" and data[lo + n:] == b"\xff\xd9" and info["scratch_bytes"] >= info["blocks"] * 128
        assert ops.jpeg_probe(torch.from_numpy(np.frombuffer(bytearray(data), dtype=np.uint8))) == info
    gray = ops.jpeg_probe(M.pil_file(img, 90, "gray"))
    assert (gray["components"], gray["hs"], gray["vs"], gray["blocks"]) == (1, 1, 1, 7 * 5)
    rotated = ops.jpeg_probe(M.oriented_file(img, 6))
    assert (rotated["h"], rotated["w"], rotated["out_h"], rotated["out_w"], rotated["orientation"]) == (37, 53, 53, 37, 6)
    xmp = b"\xff\xe1" + struct.pack(">H", 2 + 29 + 30) + b"http://ns.adobe.com/xap/1.0/\0" + b'<x tiff:Orientation="6"/>'.ljust(30)
    data = M.pil_file(img, 90, 2)
    with pytest.raises(ops.JpegUnsupported, match="ORIENTATION"):        # PIL would turn this one; the decoder reads EXIF only
        ops.jpeg_probe(data[:2] + xmp + data[2:])


def test_argument_checks_need_no_gpu():
    raw = lib.raw()
    err = lambda: raw.dvd_last_error().decode()  # noqa: E731
    data = M.pil_file(M.content("page", 16, 16), 90, 2)
    host = np.frombuffer(bytearray(data), dtype=np.uint8)
    file_host, n = C.c_void_p(host.ctypes.data), host.size
    fake, odd = C.c_void_p(1 << 20), C.c_void_p((1 << 20) + 8)
    info = lib.JpegDecInfo()
    assert raw.dvd_jpegdec_probe(None, n, C.byref(info)) == -1 and "null" in err()
    assert raw.dvd_jpegdec_probe(file_host, n, None) == -1 and "null" in err()
    assert raw.dvd_jpegdec_probe(file_host, 0, C.byref(info)) == -1 and "length" in err()
    dec = lambda *a: raw.dvd_jpeg_decode_rgb8(*a)  # noqa: E731
    cap = 3 * 16 * 16
    for args in ((None, fake, n, fake, cap, 0, None, fake, None), (file_host, None, n, fake, cap, 0, None, fake, None),
                 (file_host, fake, n, None, cap, 0, None, fake, None), (file_host, fake, n, fake, cap, 0, None, None, None)):
        assert dec(*args) == -1 and "null" in err()
    assert dec(file_host, fake, 0, fake, cap, 0, None, fake, None) == -1 and "length" in err()
    assert dec(file_host, fake, n, fake, cap - 1, 0, None, fake, None) == -1 and "cap" in err() and "3 h w" in err()
    assert dec(file_host, fake, n, fake, 0, 0, None, fake, None) == -1 and "cap" in err()
    assert dec(file_host, fake, n, fake, cap, -1, None, fake, None) == -1 and "max_iters" in err()
    assert dec(file_host, fake, n, fake, cap, 0, None, odd, None) == -1 and "aligned" in err()
    for bad in (torch.zeros(4, 4, dtype=torch.uint8), torch.zeros(8, dtype=torch.float32), torch.zeros(0, dtype=torch.uint8), "x.jpg", b""):
        with pytest.raises(ValueError):
            ops.jpeg_probe(bad)
        with pytest.raises(ValueError):
            ops.jpeg_decode(bad)
    for bad in (0, -1, 2.0, True):
        with pytest.raises(ValueError, match="max_iters"):
            ops.jpeg_decode(data, max_iters=bad)


# ---- 4. the setting and the loader --------------------------------------------------------------------------------------------
def test_env_validation(tmp_path):
    """The loader's own check of `decode` (the run's check of env.image_decoder: tests/test_run_options_cpu.py)."""
    import admin.settings as ws
    import datasets
    assert ws.Settings().env.image_decoder == "pil"
    for bad in ("cuda", "", None, "HIP"):
        with pytest.raises(ValueError, match="decode"):
            datasets.Doc_benchmark(str(tmp_path), None, decode=bad)
    assert list(tmp_path.iterdir()) == []


def test_loader_items(tmp_path):
    """Default settings: the items of before (decoded in the loader).  decode='hip': a .jpg / .jpeg item carries the file,
    other extensions behave as before; documents_of takes both item shapes, alone and behind a DataLoader."""
    from torch.utils.data import DataLoader
    import datasets
    from dvd_amd.evaluation import documents_of
    from utils_data.image_transforms import ArrayToTensor
    img = M.content("page", 37, 53)
    (tmp_path / "a.jpg").write_bytes(M.oriented_file(img, 6))
    (tmp_path / "b.JPEG").write_bytes(M.pil_file(img[:20], 75, 0))
    Image.fromarray(img).save(tmp_path / "c.png")
    tf = ArrayToTensor(get_float=False)
    for ds in (datasets.Doc_benchmark(str(tmp_path), tf), datasets.Doc_benchmark(str(tmp_path), tf, "pil"),
               datasets.Doc_benchmark(str(tmp_path), tf, decode="pil")):
        assert ds.decode == "pil" and len(ds) == 3
        for i, name in enumerate(("a.jpg", "b.JPEG", "c.png")):
            item = ds[i]
            want = M.pil_pixels((tmp_path / name).read_bytes())
            assert set(item) == {"source_image_ori", "path"} and item["path"] == str(tmp_path / name)
            assert torch.equal(item["source_image_ori"], tf(want))
    ds = datasets.Doc_benchmark(str(tmp_path), tf, decode="hip")
    for i, name in enumerate(("a.jpg", "b.JPEG")):
        item = ds[i]
        assert set(item) == {"file_bytes", "path"} and item["path"] == str(tmp_path / name)
        assert item["file_bytes"].dtype == torch.uint8 and item["file_bytes"].numpy().tobytes() == (tmp_path / name).read_bytes()
        assert documents_of(item) == [item]
    assert set(ds[2]) == {"source_image_ori", "path"} and torch.equal(ds[2]["source_image_ori"], tf(img))
    items = list(DataLoader(ds, batch_size=1, shuffle=False, num_workers=0))
    docs = [d for item in items for d in documents_of(item)]
    assert [d["path"] for d in docs] == [str(tmp_path / n) for n in ("a.jpg", "b.JPEG", "c.png")]
    assert docs[0]["file_bytes"].numpy().tobytes() == (tmp_path / "a.jpg").read_bytes() and "source_vis" in docs[2]
