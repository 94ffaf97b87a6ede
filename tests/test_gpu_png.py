"""The PNG encoder's kernels (dvd_amd/csrc/png.hip) on the GPU: every file is taken apart by png_model.check_png (signature,
chunk order, every CRC-32, IHDR, zlib.decompress with its Adler-32, the filter byte of every row against the NumPy restatement,
PIL's decode against the input, the length against dvd_png_bound).  The shapes are the smallest at which each part can go
wrong; S = DVD_PNG_SEGMENT.  Not yet run on an MI355X (DESIGN.md 4.4 records the figures once it has)."""
import io

import numpy as np
import pytest
import torch

import png_model as P
from dvd_amd import lib, ops

pytestmark = pytest.mark.gpu
S = P.header_segment()


def _rand(h, w, seed=0, hi=256):
    return np.random.RandomState(seed).randint(0, hi, (h, w, 3)).astype(np.uint8)


def _stream_shape(nbytes):
    """(h, w) with h * (3w + 1) == nbytes, the widest such image."""
    for w in range((nbytes - 1) // 3, 0, -1):
        if nbytes % (3 * w + 1) == 0:
            return nbytes // (3 * w + 1), w
    raise AssertionError(nbytes)


def _ramp(kind, h=70, w=90):
    x, y = np.arange(w)[None, :, None], np.arange(h)[:, None, None]
    v = {"horizontal": 2 * x + 0 * y, "vertical": 0 * x + 3 * y, "diagonal": 2 * x + 3 * y}[kind]
    return np.ascontiguousarray(np.broadcast_to(v % 256, (h, w, 3)).astype(np.uint8))


def _of_stream(n, seed):
    h, w = _stream_shape(n)
    return _rand(h, w, seed=seed, hi=4)           # few values: matches of every length


CASES = {
    "1x1": lambda: _rand(1, 1, 1), "1x7": lambda: _rand(1, 7, 2), "7x1": lambda: _rand(7, 1, 3), "2x2": lambda: _rand(2, 2, 4),
    "stream_S-1": lambda: _of_stream(S - 1, 5), "stream_S": lambda: _of_stream(S, 6), "stream_S+1": lambda: _of_stream(S + 1, 7),
    "7_segments_200x333": lambda: _rand(200, 333, 8, hi=16),
    "period5": lambda: (np.arange(200 * 333 * 3) % 5 * 50).astype(np.uint8).reshape(200, 333, 3),
    "random_97x131": lambda: _rand(97, 131, 9),
    "ramp_horizontal": lambda: _ramp("horizontal"), "ramp_vertical": lambda: _ramp("vertical"),
    "ramp_diagonal": lambda: _ramp("diagonal"),
}


def _encode(img, **kw):
    data = ops.png_encode(torch.from_numpy(img).cuda(), **kw)
    assert data.is_cuda and data.dtype == torch.uint8 and data.dim() == 1
    return data.cpu().numpy().tobytes()


@pytest.mark.parametrize("name", list(CASES))
def test_file_decodes_to_the_input(name):
    img = CASES[name]()
    h, w, _ = img.shape
    if name == "7_segments_200x333":
        assert -(-(h * (3 * w + 1)) // S) == 7 or S != 32768
    filters = P.check_png(_encode(img), img, S, limit=lib.raw().dvd_png_bound(h, w))
    # The ramps.  check_png has already held every row to the NumPy restatement's choice; these are its winners, reasoned:
    # rows that repeat (horizontal ramp) cost 0 under Up, and row 0 has only Sub to flatten it; a ramp down the column or along
    # both axes is predicted exactly by Paeth (a + b - c), whose first pixel (a = c = 0, so it predicts b) beats Sub's, except on
    # the rows where the ramp wraps past 255.
    if name == "ramp_horizontal":
        assert filters[0] == 1 and (filters[1:] == 2).all()
    if name in ("ramp_vertical", "ramp_diagonal"):
        assert (filters[1:] == 4).sum() >= len(filters) - 3


def test_all_zero_image_is_compressed_by_matches():
    """A 258-byte match costs 13 bits in the fixed code (0.6 %): an encoder of literals or stored blocks cannot get here."""
    img = np.zeros((512, 512, 3), np.uint8)
    data = _encode(img)
    P.check_png(data, img, S, limit=lib.raw().dvd_png_bound(512, 512))
    print(f"all-zero 512 x 512: {len(data)} bytes = {100.0 * len(data) / img.size:.3f} % of the raw bytes")
    assert len(data) <= 0.02 * img.size


def test_bytes_depend_on_the_image_only():
    """Twice, on another stream, and in a scratch buffer that another image has just used (stale LDS / stale scratch)."""
    img = _rand(120, 333, 10, hi=8)
    other = _rand(150, 400, 11)
    first = _encode(img)
    P.check_png(first, img, S)
    assert _encode(img) == first
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        on_side = _encode(img)
    side.synchronize()
    assert on_side == first
    need = max(ops._size_query("dvd_png_scratch_bytes", 120, 333), ops._size_query("dvd_png_scratch_bytes", 150, 400))
    scratch = torch.full((need,), 0xA5, dtype=torch.uint8, device="cuda")
    P.check_png(_encode(other, scratch=scratch), other, S)
    assert _encode(img, scratch=scratch) == first


def test_cap_below_the_bound_is_refused_before_any_launch():
    img = torch.zeros(8, 8, 3, dtype=torch.uint8, device="cuda")
    cap = ops.png_bound(8, 8)
    out = torch.full((cap,), 7, dtype=torch.uint8, device="cuda")
    n = torch.zeros(1, dtype=torch.int64, device="cuda")
    scratch = torch.empty(ops._size_query("dvd_png_scratch_bytes", 8, 8), dtype=torch.uint8, device="cuda")
    rc = lib.raw().dvd_png_encode_rgb8(lib.ptr(img), 8, 8, lib.ptr(out), cap - 1, lib.ptr(n), lib.ptr(scratch), lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == -1 and b"cap" in lib.raw().dvd_last_error() and int(n.item()) == 0 and bool((out == 7).all())


def _settings(tmp_path, monkeypatch, encoder):
    import admin.settings as ws
    monkeypatch.chdir(tmp_path)
    s = ws.Settings()
    s.name, s.env.png_encoder = "pytest_png", encoder
    return s, tmp_path / "vis_hp" / s.env.eval_dataset_name / "pytest_png" / "dewarped_pred"


def test_visualize_dewarping_hip_and_pil(tmp_path, monkeypatch):
    """'hip' writes dewarped_pred/warped_<stem>.png from the device page and returns the device tensor; 'pil' writes
    Image.save's bytes, as before; both files hold the page."""
    from PIL import Image
    from utils_flow.visualization_utils import visualize_dewarping
    page = _rand(40, 56, 12)
    dev = torch.from_numpy(page).cuda()
    s, out_dir = _settings(tmp_path, monkeypatch, "hip")
    ret = visualize_dewarping(s, None, None, 0, None, ["/data/crop/page_3.jpg"], warped_u8=dev)
    assert torch.is_tensor(ret) and ret.is_cuda and torch.equal(ret, dev)
    data = (out_dir / "warped_page_3.png").read_bytes()
    P.check_png(data, page, S, limit=lib.raw().dvd_png_bound(40, 56))
    assert np.array_equal(np.asarray(Image.open(out_dir / "warped_page_3.png")), page)
    s.env.png_encoder = "pil"
    ret = visualize_dewarping(s, None, None, 1, None, ["/data/crop/page_4.jpg"], warped_u8=dev)
    want = io.BytesIO()
    Image.fromarray(page).save(want, format="PNG")
    assert (out_dir / "warped_page_4.png").read_bytes() == want.getvalue() and np.array_equal(ret, page)


def test_visualize_dewarping_hip_in_the_reference_call_form(tmp_path, monkeypatch):
    """warped_u8=None: the reg_model_bilin result is truncated to uint8 on the device and encoded there - the same pixels as
    the 'pil' route writes."""
    from PIL import Image
    from utils_flow.visualization_utils import visualize_dewarping
    h, w = 40, 56
    src = torch.from_numpy(_rand(h, w, 13).transpose(2, 0, 1)[None].astype(np.float32))
    ys, xs = torch.meshgrid(torch.linspace(-1, 1, h), torch.linspace(-1, 1, w), indexing="ij")
    sample = (torch.stack([xs, ys])[None] * 0.9 + 0.03).cuda().contiguous()
    s, out_dir = _settings(tmp_path, monkeypatch, "hip")
    ret = visualize_dewarping(s, sample, None, 0, src, ["doc_1.png"], None)
    s.env.png_encoder = "pil"
    ref = visualize_dewarping(s, sample, None, 1, src, ["doc_2.png"], None)
    assert ret.is_cuda and ret.dtype == torch.uint8 and np.array_equal(ret.cpu().numpy(), ref)
    P.check_png((out_dir / "warped_doc_1.png").read_bytes(), ref, S)
    assert np.array_equal(np.asarray(Image.open(out_dir / "warped_doc_1.png")), np.asarray(Image.open(out_dir / "warped_doc_2.png")))
