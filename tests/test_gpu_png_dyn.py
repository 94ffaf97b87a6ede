"""The PNG encoder's dynamic-Huffman route (png_compress_dyn_kernel) on the GPU.  Every case of
png_dyn_model.DIGEST_CASES is encoded with huffman='dynamic', taken apart by png_model.check_png and compared BYTE FOR BYTE (length and
SHA-256) with tests/golden/png_dynamic_digests.json, which the CPU restatement png_host_check wrote: the GPU computes what the
restatement computes.  huffman='fixed' and the old entry point are held to tests/golden/png_fixed_digests.json, written by the
host program as it was before the dynamic route existed: the fixed route's bytes have not changed."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import png_dyn_model as D
import png_model as P
from dvd_amd import lib, ops

pytestmark = pytest.mark.gpu
S = D.S
DYNAMIC = json.load(open(os.path.join(D.GOLDEN, "png_dynamic_digests.json")))
FIXED = json.load(open(os.path.join(D.GOLDEN, "png_fixed_digests.json")))


def _dev(img):
    return torch.from_numpy(np.array(img)).cuda()


def _encode(img, **kw):
    data = ops.png_encode(_dev(img), **kw)
    assert data.is_cuda and data.dtype == torch.uint8 and data.dim() == 1
    return data.cpu().numpy().tobytes()


def _digest(data):
    return {"length": len(data), "sha256": hashlib.sha256(data).hexdigest()}


def _want(table, name):
    return {k: table[name][k] for k in ("length", "sha256")}


@pytest.mark.parametrize("name", list(D.DIGEST_CASES))
def test_dynamic_file_is_the_host_restatements(name):
    img = D.case(name)
    h, w, _ = img.shape
    data = _encode(img, huffman="dynamic")
    P.check_png(data, img, S, limit=lib.raw().dvd_png_bound(h, w))
    assert _digest(data) == _want(DYNAMIC, name)
    assert len(data) <= FIXED[name]["length"]


@pytest.mark.parametrize("name", list(D.DIGEST_CASES))
def test_fixed_route_writes_the_bytes_it_wrote_before(name):
    img = D.case(name)
    h, w, _ = img.shape
    assert _digest(_encode(img, huffman="fixed")) == _want(FIXED, name)
    assert _digest(_encode(img)) == _want(FIXED, name)
    dev = _dev(img)
    cap = ops.png_bound(h, w)
    out = torch.empty(cap, dtype=torch.uint8, device="cuda")
    n = torch.zeros(1, dtype=torch.int64, device="cuda")
    scratch = torch.empty(ops._size_query("dvd_png_scratch_bytes", h, w), dtype=torch.uint8, device="cuda")
    lib.call("dvd_png_encode_rgb8", lib.ptr(dev), h, w, lib.ptr(out), cap, lib.ptr(n), lib.ptr(scratch), lib.stream_ptr())
    assert _digest(out[:int(n.item())].cpu().numpy().tobytes()) == _want(FIXED, name)


def test_dynamic_bytes_depend_on_the_image_only():
    """Twice, on another stream, and in a scratch buffer prefilled with 0xA5 that another image has just used (stale LDS, stale
    tokens, stale slots)."""
    img = D.case("7_segments_200x333")
    other = D.case("random_97x131")
    first = _encode(img, huffman="dynamic")
    assert _digest(first) == _want(DYNAMIC, "7_segments_200x333")
    assert _encode(img, huffman="dynamic") == first
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        on_side = _encode(img, huffman="dynamic")
    side.synchronize()
    assert on_side == first
    need = max(ops._size_query("dvd_png_scratch_bytes_huff", *i.shape[:2], lib.PNG_HUFFMAN_DYNAMIC) for i in (img, other))
    assert need > ops._size_query("dvd_png_scratch_bytes", *img.shape[:2])
    scratch = torch.full((need,), 0xA5, dtype=torch.uint8, device="cuda")
    assert _digest(_encode(other, scratch=scratch, huffman="dynamic")) == _want(DYNAMIC, "random_97x131")
    assert _encode(img, scratch=scratch, huffman="dynamic") == first


def test_bad_cap_and_bad_huffman_are_refused_before_any_launch():
    img = torch.zeros(8, 8, 3, dtype=torch.uint8, device="cuda")
    cap = ops.png_bound(8, 8)
    out = torch.full((cap,), 7, dtype=torch.uint8, device="cuda")
    n = torch.zeros(1, dtype=torch.int64, device="cuda")
    scratch = torch.empty(ops._size_query("dvd_png_scratch_bytes_huff", 8, 8, lib.PNG_HUFFMAN_DYNAMIC), dtype=torch.uint8,
                          device="cuda")
    raw = lib.raw()
    args = lambda cap_, huff: (lib.ptr(img), 8, 8, lib.ptr(out), cap_, lib.ptr(n), lib.ptr(scratch), huff, lib.stream_ptr())  # noqa: E731
    assert raw.dvd_png_encode_rgb8_huff(*args(cap - 1, lib.PNG_HUFFMAN_DYNAMIC)) == -1 and b"cap" in raw.dvd_last_error()
    for bad in (2, -1, 7):
        assert raw.dvd_png_encode_rgb8_huff(*args(cap, bad)) == -1 and b"huffman" in raw.dvd_last_error()
    torch.cuda.synchronize()
    assert int(n.item()) == 0 and bool((out == 7).all())
    with pytest.raises(ValueError, match="'fixed' or 'dynamic'"):
        ops.png_encode(img, huffman="best")
    assert bool((out == 7).all())


def test_visualize_dewarping_dynamic_and_fixed(tmp_path, monkeypatch):
    """env.png_huffman reaches the encoder: 'dynamic' writes a file that decodes to the page and is no longer than the 'fixed'
    one, and 'fixed' writes the digest file."""
    import admin.settings as ws
    from PIL import Image
    from utils_flow.visualization_utils import visualize_dewarping
    name = "random_97x131"
    page = np.array(D.case(name))
    dev = torch.from_numpy(page).cuda()
    monkeypatch.chdir(tmp_path)
    s = ws.Settings()
    s.name, s.env.png_encoder, s.env.png_huffman = "pytest_png_dyn", "hip", "dynamic"
    out_dir = tmp_path / "vis_hp" / s.env.eval_dataset_name / "pytest_png_dyn" / "dewarped_pred"
    ret = visualize_dewarping(s, None, None, 0, None, ["/data/crop/page_3.jpg"], warped_u8=dev)
    assert torch.is_tensor(ret) and ret.is_cuda and torch.equal(ret, dev)
    dyn = (out_dir / "warped_page_3.png").read_bytes()
    P.check_png(dyn, page, S, limit=lib.raw().dvd_png_bound(*page.shape[:2]))
    assert np.array_equal(np.asarray(Image.open(out_dir / "warped_page_3.png")), page)
    assert _digest(dyn) == _want(DYNAMIC, name)
    s.env.png_huffman = "fixed"
    visualize_dewarping(s, None, None, 1, None, ["/data/crop/page_4.jpg"], warped_u8=dev)
    fixed = (out_dir / "warped_page_4.png").read_bytes()
    assert _digest(fixed) == _want(FIXED, name) and len(dyn) <= len(fixed)
