"""PNG decoder, CPU side: the NumPy / Python model against Pillow, the stand-alone C++ restatement of the
kernels (dvd_amd/csrc/pngdec_host_check.cpp, built under ASan / UBSan) against the model in pixels and statistics, one
crafted file per refusal, files this project's own encoder layout gives, the loader items and the setting."""
import io
import subprocess

import numpy as np
import pytest
import torch
from PIL import Image, ImageOps

import pngdec_model as M
from dvd_amd import lib, ops
from host_check import build_host_check

CODE_OF = {name: rc for rc, name in lib.PNG_DECODE_CODES.items()}


def pil_rgb(data):
    return np.array(ImageOps.exif_transpose(Image.open(io.BytesIO(data))).convert("RGB"), dtype=np.uint8)


@pytest.fixture(scope="module")
def corpus():
    return M.corpus()


@pytest.fixture(scope="module")
def modelled(corpus):
    return {name: M.decode(data) for name, data, _ in corpus}


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("pngdec_host_check")
    exe = build_host_check("pngdec", tmp)

    def run(data, max_work=None):
        (tmp / "in.png").write_bytes(data)
        cmd = [str(exe), str(tmp / "in.png"), str(tmp / "out.rgb")] + ([str(max_work)] if max_work else [])
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        status, cand, segs, rounds, bands, h, w = (int(v) for v in r.stdout.split())
        rgb = np.fromfile(tmp / "out.rgb", dtype=np.uint8).reshape(h, w, 3) if status == 0 else None
        return dict(status=status, candidates=cand, segments=segs, rounds=rounds, bands=bands, rgb=rgb)
    return run


# ---- 1. the model --------------------------------------------------------------------------------------------------------------
def test_corpus_holds_what_it_is_for(corpus, modelled):
    """The corpus exercises what its names promise: every block type in one stream, chains through several segments, false
    candidates, the doubling bound, one band and many."""
    names = [n for n, _, _ in corpus]
    assert len(set(names)) == len(names)
    assert modelled["mem2"]["segments"] >= 10 and modelled["mem3"]["segments"] >= 10
    assert modelled["mem5_120x88"]["segments"] >= 8
    for one in ("level0", "fixed"):
        assert modelled[one]["segments"] == 1 and modelled[one]["candidates"] == 1
    hidden = modelled["headers_in_stored"]
    assert hidden["segments"] == 1 and hidden["candidates"] >= 10           # the inner stream's true block starts, all false here
    flat = modelled["flat_40x600"]
    n = 600 * 121
    assert flat["rounds"] >= int(np.ceil(np.log2(n))) - 2 and flat["rounds"] <= int(np.ceil(np.log2(n))) + 1
    assert modelled["all_paeth"]["bands"] == 1 and modelled["all_up"]["bands"] == 1
    assert modelled["filter1_ct2"]["bands"] == 23 and modelled["mixed_ct2"]["bands"] > 5


def test_model_equals_pillow_on_the_corpus(corpus, modelled):
    for name, data, want in corpus:
        got = modelled[name]
        assert got["status"] == "OK", name
        assert np.array_equal(got["rgb"], want), name
        assert np.array_equal(pil_rgb(data), want), name


@pytest.mark.parametrize("mode", ["RGB", "RGBA", "L"])
@pytest.mark.parametrize("optimize", [False, True])
def test_model_equals_pillow_on_pillow_files(mode, optimize):
    c = {"RGB": 3, "RGBA": 4, "L": 1}[mode]
    for h, w in ((1, 1), (17, 33), (90, 70)):
        buf = io.BytesIO()
        Image.fromarray(M.content(h, w, c, seed=h), mode).save(buf, "PNG", optimize=optimize)
        got = M.decode(buf.getvalue())
        assert got["status"] == "OK" and np.array_equal(got["rgb"], pil_rgb(buf.getvalue())), (mode, optimize, h, w)


# ---- 2. the C++ restatement of the kernels -------------------------------------------------------------------------------------
def test_host_check_equals_model_on_the_corpus(corpus, modelled, host_check):
    for name, data, want in corpus:
        got, ref = host_check(data), modelled[name]
        assert got["status"] == 0, name
        assert np.array_equal(got["rgb"], want), name
        for key in ("candidates", "segments", "rounds", "bands"):
            assert got[key] == ref[key], (name, key, got[key], ref[key])


def test_host_check_equals_pillow_on_a_pillow_page(host_check):
    buf = io.BytesIO()
    Image.fromarray(M.content(220, 300, seed=3)).save(buf, "PNG")
    got = host_check(buf.getvalue())
    assert got["status"] == 0 and np.array_equal(got["rgb"], pil_rgb(buf.getvalue()))
    assert got["segments"] >= 2 and got["bands"] >= 2


# ---- 3. refusals ---------------------------------------------------------------------------------------------------------------
def test_every_refusal_has_its_own_code(host_check):
    cases = M.refusals()
    assert {c for _, _, c in cases} == set(lib.PNG_DECODE_CODES.values()) - {"NOSPLIT"}
    assert len(set(CODE_OF.values())) == len(CODE_OF) == 11 and max(CODE_OF.values()) == -36      # behind the JPEG codes
    for name, data, code in cases:
        assert M.decode(data)["status"] == code, name
        got = host_check(data)
        assert got["status"] == CODE_OF[code] and got["rgb"] is None, (name, got["status"])
        if code not in ("DATA",):                                   # decided on the host: the probe says so without a device
            with pytest.raises(ops.PngUnsupported) as e:
                ops.png_probe(data)
            assert e.value.code == code, name
        else:
            assert ops.png_probe(data)["h"] == 9


def test_pillow_refuses_or_agrees_on_damaged_data():
    """Where the decoder says DATA, PIL raises (or, for a wrong IDAT CRC or trailing bytes, may decode): never other pixels."""
    for name, data, code in M.refusals():
        if code == "DATA" and name in ("flipped_bit", "adler", "too_short", "distance"):
            with pytest.raises(Exception):
                pil_rgb(data)


def test_work_budget_is_nosplit(corpus, host_check):
    data = dict((n, d) for n, d, _ in corpus)
    for name in ("level0", "fixed", "mem3"):
        got = host_check(data[name], max_work=50)
        assert got["status"] == CODE_OF["NOSPLIT"] and got["rgb"] is None, name
        assert M.decode(data[name], max_work=50)["status"] == "NOSPLIT"
    assert host_check(data["mem3"], max_work=4000)["status"] == 0


def test_files_in_this_projects_segment_layout_decode_or_are_refused(host_check):
    """The 'fixed' encoder's layout (tests/png_model.py: one fixed block and an empty stored block per IDAT) is one segment
    for the finder: it decodes when small and is NOSPLIT when it exceeds the budget - never wrong."""
    import png_model
    img = M.content(40, 50, seed=6)
    data = png_model.model_file(img, 1024)
    got = host_check(data)
    assert got["status"] == 0 and got["segments"] == 1 and np.array_equal(got["rgb"], img)
    assert np.array_equal(M.decode(data)["rgb"], img)
    assert host_check(data, max_work=1000)["status"] == CODE_OF["NOSPLIT"]


def test_files_this_projects_encoder_writes_decode_or_are_refused(host_check, tmp_path):
    """The encoder's CPU restatement (png_host_check), fixed and dynamic blocks: a dynamic file of several 32 KiB segments is a
    chain of candidates; a fixed one is a single segment - decoded when small, NOSPLIT at a small budget.  Never other pixels."""
    exe = build_host_check("png", tmp_path)
    img = M.content(150, 100, seed=8, noise=30)                          # 45 150 stream bytes: two segments
    img.tofile(tmp_path / "in.rgb")
    for mode in ((), ("dynamic",)):
        r = subprocess.run([str(exe), "150", "100", str(tmp_path / "in.rgb"), str(tmp_path / "enc.png"), *mode], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        data = (tmp_path / "enc.png").read_bytes()
        assert np.array_equal(pil_rgb(data), img)
        got = host_check(data)
        assert got["status"] == 0 and np.array_equal(got["rgb"], img), mode
        assert got["segments"] == (2 if mode else 1), (mode, got["segments"])
        small = host_check(data, max_work=2000)
        assert small["status"] == CODE_OF["NOSPLIT"] and small["rgb"] is None, mode


def test_probe_and_argument_checks():
    data = M.make_png(M.content(9, 8, 4), 6, idat_cuts=[3, 3])
    info = ops.png_probe(data)
    assert (info["h"], info["w"], info["colour_type"], info["bpp"], info["idat_chunks"]) == (9, 8, 6, 4, 3)
    assert info["payload_bytes"] == len(M.zlib_stream_of(data)) and info["scratch_bytes"] >= 5 * 9 * 33
    assert info == ops.png_probe(torch.frombuffer(bytearray(data), dtype=torch.uint8))
    for bad in (b"", "x.png", np.zeros((2, 2), np.uint8)):
        with pytest.raises(ValueError):
            ops.png_probe(bad)
    for bad in (0, -1, 2.0, True):
        with pytest.raises(ValueError, match="max_work"):
            ops.png_decode(data, max_work=bad)
    raw = lib.raw()
    assert raw.dvd_png_decode_rgb8(None, None, 10, None, 0, 0, None, None, None) == -1 and b"null" in raw.dvd_last_error()


# ---- 4. the setting and the loader --------------------------------------------------------------------------------------------
def test_env_validation(tmp_path):
    """The loader's own check of `decode_png` (the run's check of env.png_decoder: tests/test_run_options_cpu.py)."""
    import admin.settings as ws
    import datasets
    assert ws.Settings().env.png_decoder == "pil"
    for bad in ("cuda", "", None, "HIP"):
        with pytest.raises(ValueError, match="decode_png"):
            datasets.Doc_benchmark(str(tmp_path), None, decode_png=bad)
    assert list(tmp_path.iterdir()) == []


def test_loader_items(tmp_path):
    """decode_png='hip': a .png item carries the file; decode='hip' alone leaves .png items as they are."""
    from torch.utils.data import DataLoader
    import datasets
    from dvd_amd.evaluation import documents_of
    from utils_data.image_transforms import ArrayToTensor
    img = M.content(37, 53)
    Image.fromarray(img).save(tmp_path / "a.jpg", quality=90)
    (tmp_path / "b.png").write_bytes(M.make_png(img))
    (tmp_path / "c.PNG").write_bytes(M.make_png(img[:20, :, 0], 0))
    tf = ArrayToTensor(get_float=False)
    for ds in (datasets.Doc_benchmark(str(tmp_path), tf), datasets.Doc_benchmark(str(tmp_path), tf, decode="hip")):
        assert ds.decode_png == "pil"
        for i in (1, 2):
            assert set(ds[i]) == {"source_image_ori", "path"}
        assert torch.equal(ds[1]["source_image_ori"], tf(img))
    for decode in ("pil", "hip"):
        ds = datasets.Doc_benchmark(str(tmp_path), tf, decode=decode, decode_png="hip")
        assert set(ds[0]) == ({"file_bytes", "path"} if decode == "hip" else {"source_image_ori", "path"})
        for i, name in ((1, "b.png"), (2, "c.PNG")):
            item = ds[i]
            assert set(item) == {"file_bytes", "path"} and item["path"] == str(tmp_path / name)
            assert item["file_bytes"].dtype == torch.uint8 and item["file_bytes"].numpy().tobytes() == (tmp_path / name).read_bytes()
            assert documents_of(item) == [item]
    docs = [d for item in DataLoader(ds, batch_size=1, shuffle=False, num_workers=0) for d in documents_of(item)]
    assert [d["path"] for d in docs] == [str(tmp_path / n) for n in ("a.jpg", "b.png", "c.PNG")]
    assert docs[1]["file_bytes"].numpy().tobytes() == (tmp_path / "b.png").read_bytes()


def test_decode_image_default_is_unchanged():
    """Without png=True a PNG file takes the 'pil' route with the JPEG decoder's HEADER line, with no device in sight."""
    import inspect
    assert inspect.signature(ops.decode_image).parameters["png"].default is False
    assert issubclass(ops.PngUnsupported, ValueError) and ops.PngUnsupported("DATA", "x").code == "DATA"
