"""The JPEG decoder's kernels (dvd_amd/csrc/jpegdec.hip) on the GPU: the page the library makes must EQUAL PIL's
(ImageOps.exif_transpose(Image.open(f)).convert("RGB")) byte for byte - the model (tests/jpegdec_model.py) and the sanitized CPU
restatement are held to the same bytes by tests/test_jpegdec_cpu.py.  The sizes are the smallest at which each part can go
wrong: images below one MCU, partial MCUs, chroma planes of width <= 2 (replication instead of the triangle filter), one
subsequence and hundreds that have to synchronise, restart markers, optimised tables; one full page for the sizes no small image
reaches.  No test here feeds corrupt scan data."""
import io
import os

import numpy as np
import pytest
import torch
from PIL import Image

import jpeg_model as J
import jpegdec_model as M
from dvd_amd import lib, ops

pytestmark = pytest.mark.gpu


def _decode(data, **kw):
    img = ops.jpeg_decode(data, **kw)
    out = img[0] if isinstance(img, tuple) else img
    assert out.is_cuda and out.dtype == torch.uint8 and out.dim() == 3 and out.shape[2] == 3 and out.is_contiguous()
    return (out.cpu().numpy(), img[1]) if isinstance(img, tuple) else out.cpu().numpy()


@pytest.mark.parametrize("h,w", M.SIZES, ids=lambda v: str(v))
def test_pixels_equal_pil_on_the_grid(h, w):
    """noise and a page x (quality 5..100, 4:4:4 / 4:2:2 / 4:2:0 / gray, optimize, restart rows, restart blocks)"""
    for kind in M.CONTENTS:
        img = M.content(kind, h, w)
        for quality, ss, kw in M.SETTINGS:
            data = M.pil_file(img, quality, ss, **kw)
            want = M.pil_pixels(data)
            got = _decode(data)
            assert got.shape == want.shape and np.array_equal(got, want), (kind, quality, ss, kw)


@pytest.mark.parametrize("make", (M.sync_page, M.sync_noise), ids=lambda f: f.__name__)
def test_hundreds_of_subsequences_synchronise(make):
    """The 300 x 400 noisy 4:2:0 page (model: 13 iterations) and 160 x 200 noise at quality 95 (model: 35): every lane but
    the first starts from a guess.  The kernel's lanes may read a state written in the same iteration, so its count is at
    most the model's, not equal to it."""
    data = make()
    assert ops.jpeg_probe(data)["scan_bytes"] > 290 * lib.JPEGDEC_SUBSEQ          # 329 and 296 subsequences
    got, iters = _decode(data, return_iters=True)
    print(f"{make.__name__}: {iters} iterations")
    assert np.array_equal(got, M.pil_pixels(data))
    assert 1 < iters < 64


def test_exactly_flat_image():
    """400 x 600 of one colour: runs that never self-synchronise - the truth crosses them one subsequence per iteration"""
    data = M.flat_file()
    got, iters = _decode(data, return_iters=True)
    print(f"flat: {iters} iterations for {ops.jpeg_probe(data)['scan_bytes']} scan bytes")
    assert np.array_equal(got, M.pil_pixels(data))


@pytest.mark.parametrize("subsampling", ("420", "444"))
def test_round_trip_through_the_encoder(subsampling):
    """ops.jpeg_encode's file (one restart interval per MCU row) never leaves the device on its way into ops.jpeg_decode"""
    img = J.synthetic_page("noisy", 120, 333, seed=10)
    file_dev = ops.jpeg_encode(torch.from_numpy(img).cuda(), 90, subsampling)
    got = ops.jpeg_decode(file_dev)
    assert got.device == file_dev.device
    assert np.array_equal(got.cpu().numpy(), M.pil_pixels(file_dev.cpu().numpy().tobytes()))


@pytest.mark.parametrize("h,w", [(17, 5), (37, 53)])
def test_orientations(h, w):
    img = M.content("noise", h, w)
    for o in range(1, 9):
        data = M.oriented_file(img, o)
        want = M.pil_pixels(data)
        got = _decode(data)
        assert got.shape == want.shape == ((w, h, 3) if o >= 5 else (h, w, 3)) and np.array_equal(got, want), o


def test_output_at_an_odd_address():
    data = M.pil_file(M.content("page", 33, 48), 90, 2)
    buf = torch.full((3 * 33 * 48 + 64,), 7, dtype=torch.uint8, device="cuda")
    off = 1 if buf.data_ptr() % 2 == 0 else 2
    view = buf[off:off + 3 * 33 * 48]
    assert view.data_ptr() % 2 == 1
    got = ops.jpeg_decode(data, out=view)
    assert got.data_ptr() == view.data_ptr() and np.array_equal(got.cpu().numpy(), M.pil_pixels(data))
    assert bool((buf[:off] == 7).all()) and bool((buf[off + 3 * 33 * 48:] == 7).all())
    # cap below 3 h w: refused before anything is launched
    raw, host = lib.raw(), np.frombuffer(bytearray(data), dtype=np.uint8)
    file_dev = torch.from_numpy(host).cuda()
    scratch = torch.empty(ops.jpeg_probe(data)["scratch_bytes"], dtype=torch.uint8, device="cuda")
    buf.fill_(7)
    rc = raw.dvd_jpeg_decode_rgb8(host.ctypes.data, lib.ptr(file_dev), host.size, lib.ptr(buf), 3 * 33 * 48 - 1, 0, None,
                                  lib.ptr(scratch), lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == -1 and b"cap" in raw.dvd_last_error() and bool((buf == 7).all())


def test_two_decodes_on_a_side_stream():
    """... in one scratch buffer that the other file has just used, beside a decode on the default stream"""
    a, b = M.pil_file(M.content("page", 64, 49), 90, 2), M.pil_file(M.content("noise", 37, 53), 75, 1, restart_marker_rows=1)
    need = max(ops.jpeg_probe(a)["scratch_bytes"], ops.jpeg_probe(b)["scratch_bytes"])
    scratch = torch.full((need,), 0xA5, dtype=torch.uint8, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got_a = ops.jpeg_decode(a, scratch=scratch)
        got_b = ops.jpeg_decode(b, scratch=scratch)
    beside = ops.jpeg_decode(a)
    side.synchronize()
    torch.cuda.synchronize()
    assert np.array_equal(got_a.cpu().numpy(), M.pil_pixels(a)) and np.array_equal(got_b.cpu().numpy(), M.pil_pixels(b))
    assert np.array_equal(beside.cpu().numpy(), M.pil_pixels(a))


def test_iteration_cap_falls_back_to_pil():
    data = M.sync_page()
    with pytest.raises(ops.JpegUnsupported, match="NOSYNC") as e:
        ops.jpeg_decode(data, max_iters=2)
    assert e.value.code == "NOSYNC"
    lines = []
    img, route = ops.decode_image(data, "cuda", max_iters=2, log=lines.append)
    assert route == "pil" and img.is_cuda and np.array_equal(img.cpu().numpy(), M.pil_pixels(data))
    assert len(lines) == 1 and "NOSYNC" in lines[0]
    img, route = ops.decode_image(data, "cuda", log=lines.append)
    assert route == "hip" and np.array_equal(img.cpu().numpy(), M.pil_pixels(data)) and len(lines) == 1


def test_refused_files_take_the_pil_route(tmp_path):
    img = M.content("page", 37, 53)
    files = {}
    for name, kw in (("PROGRESSIVE", {"progressive": True}), ("COMPONENTS", {"cmyk": True})):
        buf = io.BytesIO()
        (Image.fromarray(img).convert("CMYK") if kw.pop("cmyk", False) else Image.fromarray(img)).save(buf, format="JPEG", **kw)
        files[name] = buf.getvalue()
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, format="PNG")
    files["HEADER"] = buf.getvalue()
    for code, data in files.items():
        lines = []
        got, route = ops.decode_image(data, "cuda", log=lines.append)
        assert route == "pil" and np.array_equal(got.cpu().numpy(), M.pil_pixels(data))
        assert len(lines) == 1 and code in lines[0], lines
    path = tmp_path / "page.jpg"
    path.write_bytes(M.oriented_file(img, 8))
    got, route = ops.decode_image(str(path), "cuda")
    assert route == "hip" and np.array_equal(got.cpu().numpy(), M.pil_pixels(path.read_bytes()))
    assert torch.equal(ops.jpeg_decode_from_file(str(path)), got)


def _page_dir(path):
    """two JPEGs of different sizes (one turned by EXIF) and one PNG"""
    from dvd_amd import synth
    os.makedirs(path)
    arrays = []
    for i, (h, w) in enumerate(((120, 88), (104, 80), (120, 88))):
        img = synth.smooth_image(f"jpegdec{i}/image", h, w, seed=1234)
        arrays.append(np.ascontiguousarray((img.transpose(1, 2, 0) * 255.0).astype(np.uint8)))
    with open(os.path.join(path, "doc_0.jpg"), "wb") as f:
        f.write(M.oriented_file(arrays[0], 6))
    with open(os.path.join(path, "doc_1.jpeg"), "wb") as f:
        f.write(M.pil_file(arrays[1], 90, 0))
    Image.fromarray(arrays[2]).save(os.path.join(path, "doc_2.png"))


def test_loader_and_decode_step_give_the_pil_routes_bytes(tmp_path):
    from torch.utils.data import DataLoader
    import datasets
    from dvd_amd.evaluation import _source_u8, decode_documents, documents_of
    from utils_data.image_transforms import ArrayToTensor
    _page_dir(str(tmp_path / "pages"))
    docs = {}
    for decode in ("pil", "hip"):
        loader = DataLoader(datasets.Doc_benchmark(str(tmp_path / "pages"), ArrayToTensor(get_float=False), decode=decode),
                            batch_size=1, shuffle=False, num_workers=0)
        docs[decode] = [d for item in loader for d in documents_of(item)]
        decode_documents(docs[decode], "cuda")
    assert [d.get("decode_route") for d in docs["hip"]] == ["hip", "hip", None]
    assert [d.get("decode_route") for d in docs["pil"]] == [None, None, None]
    for a, b in zip(docs["pil"], docs["hip"]):
        assert a["path"] == b["path"]
        want = _source_u8(a, "cuda")
        got = b["image_u8"] if "image_u8" in b else _source_u8(b, "cuda")
        assert got.is_cuda and got.dtype == torch.uint8 and torch.equal(got, want), a["path"]
    assert tuple(docs["hip"][0]["image_u8"].shape) == (88, 120, 3)                       # turned


def test_run_writes_the_same_pages_under_pil_and_hip(tmp_path, monkeypatch):
    """val_TDiff.run on a directory (Doc_benchmark behind a DataLoader, run_evaluation_docunet): env.image_decoder changes who
    decodes, not a byte of what is written."""
    import admin.settings as ws
    from dvd_amd import val_TDiff
    monkeypatch.chdir(tmp_path)
    _page_dir("pages")
    pages = {}
    for decoder in ("pil", "hip"):
        s = ws.Settings()
        s.env.grid_size, s.env.diffusion_steps, s.env.batch_docs = 16, 3, 2
        s.name, s.seed, s.severity, s.corruption_number = f"pytest_jpegdec_{decoder}", 0, 0, 0
        s.env.eval_dataset_name, s.env.eval_dataset = "docunet", "pages"
        s.env.use_prestage_nets, s.env.synthetic_weights_if_missing, s.env.visualize = True, True, True
        s.env.image_decoder = decoder
        torch.manual_seed(0)
        got = val_TDiff.run(s)
        out_dir = tmp_path / "vis_hp" / "docunet" / s.name / "dewarped_pred"
        pages[decoder] = ([(p, img.cpu()) for p, img in got], {f.name: f.read_bytes() for f in sorted(out_dir.iterdir())})
    assert len(pages["pil"][1]) == 3 and "warped_doc_0.png" in pages["pil"][1]
    assert pages["pil"][1] == pages["hip"][1]
    for (pa, a), (pb, b) in zip(*(pages[k][0] for k in ("pil", "hip"))):
        assert pa == pb and torch.equal(a, b), pa


def test_full_page():
    """3508 x 2480, quality 90, 4:2:0, as PIL writes it (no restart markers): tens of thousands of subsequences, 204 600
    blocks, 799 chunks of the DC sum"""
    h, w = 3508, 2480
    data = M.pil_file(J.synthetic_page("noisy", h, w, seed=5), 90, 2)
    info = ops.jpeg_probe(data)
    assert info["blocks"] == 220 * 155 * 6 and info["restart_interval"] == 0
    img, iters = ops.jpeg_decode(data, return_iters=True)
    print(f"3508 x 2480 noisy page, quality 90, 4:2:0: {len(data)} bytes, {info['scan_bytes'] // lib.JPEGDEC_SUBSEQ + 1} subsequences, "
          f"{iters} iterations")
    assert np.array_equal(img.cpu().numpy(), M.pil_pixels(data))
