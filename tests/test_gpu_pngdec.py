"""The PNG decoder's kernels (dvd_amd/csrc/pngdec.hip) on the GPU: the page the library makes must EQUAL PIL's
(ImageOps.exif_transpose(Image.open(f)).convert("RGB")) and the model's (tests/pngdec_model.py) byte for byte, and report the
model's statistics where they are deterministic (the in-place doubling may take fewer rounds than the model's synchronous
ones, never more).  The corpus is the CPU suite's: small files that go wrong where pages do; one full page for the sizes
no small image reaches.  Damaged files are refused with `out` untouched; nothing here can fault the device - the walk and
the sinks check every index."""
import io
import os

import numpy as np
import pytest
import torch
from PIL import Image, ImageOps

import pngdec_model as M
from dvd_amd import ops

pytestmark = pytest.mark.gpu


def pil_rgb(data):
    return np.array(ImageOps.exif_transpose(Image.open(io.BytesIO(data))).convert("RGB"), dtype=np.uint8)


@pytest.fixture(scope="module")
def corpus():
    return M.corpus()


def test_kernels_equal_model_and_pil_on_the_corpus(corpus):
    for name, data, want in corpus:
        img, stats = ops.png_decode(data, return_stats=True)
        assert img.is_cuda and img.dtype == torch.uint8 and img.is_contiguous() and tuple(img.shape) == want.shape, name
        assert np.array_equal(img.cpu().numpy(), want), name
        if not name.startswith("cut_") or name in ("cut_0", "cut_bytes", "cut_empty"):      # the model is slow; the cuts share one stream
            ref = M.decode(data)
            assert np.array_equal(ref["rgb"], want) and np.array_equal(pil_rgb(data), want), name
            for key in ("candidates", "segments", "bands"):
                assert stats[key] == ref[key], (name, key, stats[key], ref[key])
            assert 1 <= stats["rounds"] <= ref["rounds"], (name, stats["rounds"], ref["rounds"])


@pytest.mark.parametrize("mode", ["RGB", "RGBA", "L"])
def test_pillow_files(mode):
    c = {"RGB": 3, "RGBA": 4, "L": 1}[mode]
    for h, w in ((1, 1), (17, 33), (220, 300)):
        for optimize in (False, True):
            buf = io.BytesIO()
            Image.fromarray(M.content(h, w, c, seed=h), mode).save(buf, "PNG", optimize=optimize)
            got = ops.png_decode(buf.getvalue())
            assert np.array_equal(got.cpu().numpy(), pil_rgb(buf.getvalue())), (mode, h, w, optimize)


def test_refusals_leave_out_untouched(corpus):
    files = dict((n, d) for n, d, _ in corpus)
    cases = [(name, data, code, None) for name, data, code in M.refusals()]
    cases += [("budget_" + n, files[n], "NOSPLIT", 50) for n in ("level0", "fixed", "mem3")]
    for name, data, code, max_work in cases:
        out = torch.full((3 * 9 * 8 + 3 * 49 * 64,), 0xA5, dtype=torch.uint8, device="cuda")
        with pytest.raises(ops.PngUnsupported) as e:
            ops.png_decode(data, out=out, max_work=max_work)
        assert e.value.code == code, (name, e.value.code)
        assert bool((out == 0xA5).all()), name


def test_out_at_an_odd_address_and_scratch_reuse(corpus):
    files = {n: (d, want) for n, d, want in corpus}
    need = max(ops.png_probe(files[n][0])["scratch_bytes"] for n in ("mem2", "mixed_ct6", "filter4_ct0"))
    scratch = torch.full((need,), 0xFF, dtype=torch.uint8, device="cuda")
    for name in ("mem2", "mixed_ct6", "filter4_ct0", "mem2"):
        data, want = files[name]
        for shift in (1, 3):
            buf = torch.full((want.size + 16,), 0x5A, dtype=torch.uint8, device="cuda")
            got = ops.png_decode(data, scratch=scratch, out=buf[shift:])
            assert got.data_ptr() == buf.data_ptr() + shift and np.array_equal(got.cpu().numpy(), want), (name, shift)
            assert bool((buf[:shift] == 0x5A).all()) and bool((buf[shift + want.size:] == 0x5A).all()), (name, shift)
    with pytest.raises(ValueError, match="scratch"):
        ops.png_decode(files["mem2"][0], scratch=scratch[:1024])


def test_decode_image_routes(corpus, tmp_path):
    data, want = next((d, w) for n, d, w in corpus if n == "mem3")
    lines = []
    img, route = ops.decode_image(data, png=True, log=lines.append)
    assert route == "hip" and lines == [] and np.array_equal(img.cpu().numpy(), want)
    (tmp_path / "a.png").write_bytes(data)
    img, route = ops.decode_image(str(tmp_path / "a.png"), png=True, log=lines.append)
    assert route == "hip" and lines == [] and np.array_equal(img.cpu().numpy(), want)
    assert torch.equal(ops.png_decode_from_file(str(tmp_path / "a.png")), img)
    img, route = ops.decode_image(data, log=lines.append)                     # the default: as before this decoder existed
    assert route == "pil" and len(lines) == 1 and "HEADER" in lines[0] and np.array_equal(img.cpu().numpy(), want)
    buf = io.BytesIO()
    Image.fromarray(want).convert("P").save(buf, "PNG")                        # a palette file: refused, PIL decodes it
    lines.clear()
    img, route = ops.decode_image(buf.getvalue(), png=True, log=lines.append)
    assert route == "pil" and len(lines) == 1 and "COLOUR" in lines[0]
    assert img.is_cuda and np.array_equal(img.cpu().numpy(), pil_rgb(buf.getvalue()))
    damaged = next(d for n, d, c in M.refusals() if n == "adler")
    lines.clear()
    with pytest.raises(Exception):                                             # PIL refuses the file too: nobody invents pixels
        ops.decode_image(damaged, png=True, log=lines.append)
    assert len(lines) == 1 and "DATA" in lines[0]


def _page_dir(path):
    """two PNGs of different sizes (one RGBA) and one JPEG"""
    os.makedirs(path)
    Image.fromarray(M.content(120, 88, seed=11)).save(os.path.join(path, "doc_0.png"))
    Image.fromarray(M.content(104, 80, 4, seed=12), "RGBA").save(os.path.join(path, "doc_1.png"))
    Image.fromarray(M.content(120, 88, seed=13)).save(os.path.join(path, "doc_2.jpg"), quality=90)


def test_loader_and_decode_step_give_the_pil_routes_bytes(tmp_path):
    from torch.utils.data import DataLoader
    import datasets
    from dvd_amd.evaluation import _source_u8, decode_documents, documents_of
    from utils_data.image_transforms import ArrayToTensor
    _page_dir(str(tmp_path / "pages"))
    docs = {}
    for decode in ("pil", "hip"):
        ds = datasets.Doc_benchmark(str(tmp_path / "pages"), ArrayToTensor(get_float=False), decode=decode, decode_png=decode)
        docs[decode] = [d for item in DataLoader(ds, batch_size=1, shuffle=False, num_workers=0) for d in documents_of(item)]
        decode_documents(docs[decode], "cuda", png=decode == "hip")
    assert [d.get("decode_route") for d in docs["hip"]] == ["hip", "hip", "hip"]
    assert [d.get("decode_route") for d in docs["pil"]] == [None, None, None]
    for a, b in zip(docs["pil"], docs["hip"]):
        assert a["path"] == b["path"]
        got = b["image_u8"]
        assert got.is_cuda and got.dtype == torch.uint8 and torch.equal(got, _source_u8(a, "cuda")), a["path"]


def test_run_writes_the_same_pages_and_scores_under_pil_and_hip(tmp_path, monkeypatch, capsys):
    """val_TDiff.run on a directory with env.gt_dir: env.png_decoder changes who decodes the photographs and the scans, not a
    byte of what is written and not a bit of ms_ssim / ld / ad."""
    import admin.settings as ws
    from dvd_amd import val_TDiff
    monkeypatch.chdir(tmp_path)
    _page_dir("pages")
    os.makedirs("gt")
    Image.fromarray(M.content(200, 150, seed=21)).save("gt/doc_0.png")
    Image.fromarray(M.content(190, 260, 1, seed=22), "L").save("gt/doc_1.png")
    Image.fromarray(M.content(200, 150, seed=23)).convert("P").save("gt/doc_2.png")      # refused: PIL decodes it
    runs = {}
    for decoder in ("pil", "hip"):
        s = ws.Settings()
        s.env.grid_size, s.env.diffusion_steps, s.env.batch_docs = 16, 3, 2
        s.name, s.seed, s.severity, s.corruption_number = f"pytest_pngdec_{decoder}", 0, 0, 0
        s.env.eval_dataset_name, s.env.eval_dataset = "docunet", "pages"
        s.env.use_prestage_nets, s.env.synthetic_weights_if_missing, s.env.visualize = True, True, True
        s.env.gt_dir, s.env.gt_metrics, s.env.gt_ad = "gt", "ms_ssim,ld", True
        s.env.png_decoder = s.env.image_decoder = decoder
        torch.manual_seed(0)
        capsys.readouterr()
        got = val_TDiff.run(s)
        log = capsys.readouterr().out
        out_dir = tmp_path / "vis_hp" / "docunet" / s.name / "dewarped_pred"
        runs[decoder] = ([(p, img.cpu()) for p, img in got], {f.name: f.read_bytes() for f in sorted(out_dir.iterdir())},
                         (s.ms_ssim, s.ld, s.ad), log)
    assert len(runs["pil"][1]) == 3 and len(runs["pil"][2][0]) == 3
    assert runs["pil"][1] == runs["hip"][1]
    assert runs["pil"][2] == runs["hip"][2]
    for (pa, a), (pb, b) in zip(runs["pil"][0], runs["hip"][0]):
        assert pa == pb and torch.equal(a, b), pa
    assert "COLOUR" not in runs["pil"][3] and runs["hip"][3].count("COLOUR") == 1


def test_full_page():
    """3508 x 2480 RGB, noisy with flat margins, as PIL writes it at its default level."""
    h, w = 3508, 2480
    rng = np.random.RandomState(5)
    img = np.full((h, w, 3), 255, np.uint8)
    yy, xx = np.mgrid[0:h - 400, 0:w - 300]
    img[200:h - 200, 150:w - 150] = ((yy // 7 + xx // 5)[..., None] + rng.randint(0, 48, (h - 400, w - 300, 3))).astype(np.uint8)
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, "PNG")
    data = buf.getvalue()
    got, stats = ops.png_decode(data, return_stats=True)
    print(f"3508 x 2480 page: {len(data)} bytes, {stats}")
    assert stats["segments"] > 100 and stats["bands"] > 100
    assert np.array_equal(got.cpu().numpy(), img)
