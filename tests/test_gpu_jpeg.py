"""The JPEG encoder's kernels (dvd_amd/csrc/jpeg.hip) on the GPU: the library's file must EQUAL the integer model's
(tests/jpeg_model.py, itself held to PIL and to the sanitized CPU restatement by tests/test_jpeg_cpu.py) byte for byte.  The
shapes are the smallest at which each part can go wrong: images below one MCU, sizes that are no multiple of it, ten intervals
(RST wraps), 257 intervals (two to a lane of the layout scan), 513 MCUs in one interval (more than one tile of 256 blocks per
interval, a strip boundary every 256 pixels), stuffed 0xFF bytes, ZRL and EOB; one full page for the sizes no small image
reaches."""
import numpy as np
import pytest
import torch

import jpeg_model as J
from dvd_amd import lib, ops

pytestmark = pytest.mark.gpu
SS = ("420", "444")


def _inputs():
    cases = {f"{h}x{w}": (J.noise_image(h, w, seed=h * 131 + w), J.QUALITIES) for h, w in J.SHAPES}
    for name, (img, quality) in J.stress_cases().items():
        cases[name] = (img, tuple(sorted(set(J.QUALITIES + (quality,)))))
    return cases


INPUTS = _inputs()


def _encode(img, quality=90, subsampling="420", **kw):
    dev = img if torch.is_tensor(img) else torch.from_numpy(img).cuda()
    data = ops.jpeg_encode(dev, quality, subsampling, **kw)
    assert data.is_cuda and data.dtype == torch.uint8 and data.dim() == 1
    return data.cpu().numpy().tobytes()


@pytest.mark.parametrize("subsampling", SS)
@pytest.mark.parametrize("name", list(INPUTS))
def test_file_equals_the_model(name, subsampling):
    img, qualities = INPUTS[name]
    h, w, _ = img.shape
    for quality in qualities:
        data = _encode(img, quality, subsampling)
        want = J.model_file(img, quality, subsampling)
        assert data == want, (quality, len(data), len(want), next((i for i, (a, b) in enumerate(zip(data, want)) if a != b), None))
        assert len(data) <= lib.raw().dvd_jpeg_bound(h, w, J.SUBSAMPLINGS[subsampling])
    J.check_jpeg(data, img, qualities[-1], subsampling)


def test_257_intervals_two_to_a_lane_of_the_layout_scan():
    """2056 x 8 in 4:4:4 = 257 restart intervals: a lane of jpeg_layout_kernel's scan over the interval lengths owns two."""
    img = J.noise_image(2056, 8, seed=2056 * 131 + 8)
    for quality in J.QUALITIES:
        data = _encode(img, quality, "444")
        want = J.model_file(img, quality, "444")
        assert data == want, (quality, len(data), len(want), next((i for i, (a, b) in enumerate(zip(data, want)) if a != b), None))
        assert len(data) <= lib.raw().dvd_jpeg_bound(2056, 8, J.SUBSAMPLINGS["444"])
    J.check_jpeg(data, img, J.QUALITIES[-1], "444")


@pytest.mark.parametrize("subsampling", SS)
def test_image_at_an_odd_address(subsampling):
    """A view whose first byte lies at an odd address inside a larger buffer (rows start at any alignment anyway: 3 w bytes)."""
    img = J.noise_image(33, 47, seed=21)
    buf = torch.zeros(img.size + 64, dtype=torch.uint8, device="cuda")
    off = 1 if buf.data_ptr() % 2 == 0 else 2
    view = buf[off:off + img.size].view(33, 47, 3)
    view.copy_(torch.from_numpy(img))
    assert view.data_ptr() % 2 == 1 and view.is_contiguous()
    assert _encode(view, 90, subsampling) == J.model_file(img, 90, subsampling)


def test_batch_loop_on_a_side_stream():
    """Three 120 x 100 documents of a batch, encoded one after the other on a non-default stream."""
    batch = np.stack([J.noise_image(120, 100, seed=30 + k) // (k + 1) for k in range(3)])
    dev = torch.from_numpy(batch).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        files = [ops.jpeg_encode(dev[k], 90, "420") for k in range(3)]
    side.synchronize()
    for k in range(3):
        assert files[k].cpu().numpy().tobytes() == J.model_file(batch[k], 90, "420"), k


def test_bytes_depend_on_the_image_and_settings_only():
    """Twice, beside another encode on a second stream, and in a scratch buffer that another image has just used."""
    img = J.synthetic_page("noisy", 120, 333, seed=10)
    other = J.noise_image(150, 400, seed=11)
    first = _encode(img)
    assert first == J.model_file(img, 90, "420")
    assert _encode(img) == first
    dev, dev_other = torch.from_numpy(img).cuda(), torch.from_numpy(other).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = ops.jpeg_encode(dev_other, 100, "444")
    beside = ops.jpeg_encode(dev, 90, "420")
    side.synchronize()
    torch.cuda.synchronize()
    assert beside.cpu().numpy().tobytes() == first
    assert on_side.cpu().numpy().tobytes() == J.model_file(other, 100, "444")
    need = max(ops._size_query("dvd_jpeg_scratch_bytes", 120, 333, lib.JPEG_420),
               ops._size_query("dvd_jpeg_scratch_bytes", 150, 400, lib.JPEG_444))
    scratch = torch.full((need,), 0xA5, dtype=torch.uint8, device="cuda")
    assert _encode(other, 100, "444", scratch=scratch) == J.model_file(other, 100, "444")
    assert _encode(img, scratch=scratch) == first


def test_cap_below_the_bound_is_refused_before_any_launch():
    img = torch.zeros(8, 8, 3, dtype=torch.uint8, device="cuda")
    cap = ops.jpeg_bound(8, 8, "420")
    out = torch.full((cap,), 7, dtype=torch.uint8, device="cuda")
    n = torch.zeros(1, dtype=torch.int64, device="cuda")
    scratch = torch.empty(ops._size_query("dvd_jpeg_scratch_bytes", 8, 8, lib.JPEG_420), dtype=torch.uint8, device="cuda")
    rc = lib.raw().dvd_jpeg_encode_rgb8(lib.ptr(img), 8, 8, 90, lib.JPEG_420, lib.ptr(out), cap - 1, lib.ptr(n), lib.ptr(scratch),
                                        lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == -1 and b"cap" in lib.raw().dvd_last_error() and int(n.item()) == 0 and bool((out == 7).all())


def _settings(tmp_path, monkeypatch, **env):
    import admin.settings as ws
    monkeypatch.chdir(tmp_path)
    s = ws.Settings()
    s.name = "pytest_jpeg"
    for key, value in env.items():
        setattr(s.env, key, value)
    return s, tmp_path / "vis_hp" / s.env.eval_dataset_name / "pytest_jpeg" / "dewarped_pred"


def test_visualize_dewarping_jpeg_and_png(tmp_path, monkeypatch):
    """'jpeg' writes dewarped_pred/warped_<stem>.jpg - the model's bytes for that tensor at the env's quality and subsampling -
    and returns the device tensor, whatever png_encoder says; 'png' behaves as before on both of its routes."""
    import io
    from PIL import Image
    import png_model as P
    from utils_flow.visualization_utils import visualize_dewarping
    page = J.synthetic_page("bars", 40, 56, seed=12)
    dev = torch.from_numpy(page).cuda()
    s, out_dir = _settings(tmp_path, monkeypatch, page_format="jpeg", jpeg_quality=75, jpeg_subsampling="444", png_encoder="pil")
    ret = visualize_dewarping(s, None, None, 0, None, ["/data/crop/page_3.png"], warped_u8=dev)
    assert torch.is_tensor(ret) and ret.is_cuda and torch.equal(ret, dev)
    assert (out_dir / "warped_page_3.jpg").read_bytes() == J.model_file(page, 75, "444")
    s.env.jpeg_quality, s.env.jpeg_subsampling, s.env.png_encoder = 90, "420", "hip"
    visualize_dewarping(s, None, None, 1, None, ["/data/crop/page_4.png"], warped_u8=dev)
    assert (out_dir / "warped_page_4.jpg").read_bytes() == J.model_file(page, 90, "420")
    assert sorted(p.name for p in out_dir.iterdir()) == ["warped_page_3.jpg", "warped_page_4.jpg"]
    s.env.page_format, s.env.png_encoder = "png", "pil"
    ret = visualize_dewarping(s, None, None, 2, None, ["/data/crop/page_5.jpg"], warped_u8=dev)
    want = io.BytesIO()
    Image.fromarray(page).save(want, format="PNG")
    assert (out_dir / "warped_page_5.png").read_bytes() == want.getvalue() and np.array_equal(ret, page)
    s.env.png_encoder = "hip"
    ret = visualize_dewarping(s, None, None, 3, None, ["/data/crop/page_6.jpg"], warped_u8=dev)
    assert ret.is_cuda and torch.equal(ret, dev)
    P.check_png((out_dir / "warped_page_6.png").read_bytes(), page, P.header_segment(), limit=lib.raw().dvd_png_bound(40, 56))


def test_visualize_dewarping_jpeg_in_the_reference_call_form(tmp_path, monkeypatch):
    """warped_u8=None: the reg_model_bilin result is truncated to uint8 on the device and encoded there - the pixels the 'png'
    route writes."""
    from utils_flow.visualization_utils import visualize_dewarping
    h, w = 40, 56
    src = torch.from_numpy(J.noise_image(h, w, seed=13).transpose(2, 0, 1)[None].astype(np.float32))
    ys, xs = torch.meshgrid(torch.linspace(-1, 1, h), torch.linspace(-1, 1, w), indexing="ij")
    sample = (torch.stack([xs, ys])[None] * 0.9 + 0.03).cuda().contiguous()
    s, out_dir = _settings(tmp_path, monkeypatch, page_format="jpeg")
    ret = visualize_dewarping(s, sample, None, 0, src, ["doc_1.png"], None)
    s.env.page_format = "png"
    ref = visualize_dewarping(s, sample, None, 1, src, ["doc_2.png"], None)
    assert ret.is_cuda and ret.dtype == torch.uint8 and np.array_equal(ret.cpu().numpy(), ref)
    assert (out_dir / "warped_doc_1.jpg").read_bytes() == J.model_file(ref, 90, "420")


def test_full_page():
    """3508 x 2480, quality 90, 4:2:0: 220 intervals of 930 blocks (four tiles each), ten strips per MCU row.  The whole file
    goes through check_jpeg (every marker, the RST sequence, stuffing, PIL's decode); the model is too slow for a byte comparison
    of the whole page, so the first and last three intervals are compared with the model run on those MCU rows alone - intervals
    are independent (predictors restart, padding ends them), which is what makes that the same bytes."""
    h, w = 3508, 2480
    img = J.synthetic_page("noisy", h, w, seed=5)
    data = _encode(img, 90, "420")
    assert len(data) <= lib.raw().dvd_jpeg_bound(h, w, lib.JPEG_420)
    which = [0, 1, 2, 217, 218, 219]
    intervals = J.check_jpeg(data, img, 90, "420", decode=which)
    assert len(intervals) == 220
    for i in which:
        assert intervals[i] == J.model_intervals(img[16 * i:16 * i + 16], 90, "420")[0], i
    print(f"3508 x 2480 noisy page, quality 90, 4:2:0: {len(data)} bytes = {100.0 * len(data) / img.size:.2f} % of the raw bytes")
