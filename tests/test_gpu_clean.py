"""Scan-like pages on the device: the kernels of clean.hip against tests/clean_model.py - whole buffers, byte for
byte, between guard bytes, inputs untouched, counts equal - equivalent calls against each other, and the command-line tools end
to end.  Every test runs once; a fault ends the file's run."""
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clean_fixtures as X  # noqa: E402
import clean_model as M  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 64                     # bytes on either side of an output, pre-filled
SIZES = X.SIZES + ((500, 700),)


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()                  # a copy: the fixtures are read-only


def _guarded(shape, dtype, shift=0):
    """(the whole byte buffer, a tensor of `shape` inside it that begins `shift` bytes past a 256-byte boundary)."""
    n = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
    whole = torch.full((256 + shift + n + GUARD,), 0x5a, dtype=torch.uint8, device="cuda")
    lead = (-whole.data_ptr()) % 256 + shift
    if lead < GUARD:
        lead += 256
    return whole, whole[lead:lead + n].view(dtype).view(*shape), lead, n


def _guards_untouched(whole, lead, n):
    raw = whole.cpu().numpy()
    return (raw[:lead] == 0x5a).all() and (raw[lead + n:] == 0x5a).all()


@functools.lru_cache(maxsize=None)
def _page(size):
    return X.text_page()["page"] if size == (500, 700) else X.page_of(size, "noise" if size[0] * size[1] < 4000 else "text")


@functools.lru_cache(maxsize=None)
def _background(size, cell, close, smooth, neutral):
    return M.background(_page(size), cell, close, smooth, neutral)


def _check_flatten(ops, size, cell=16, close=2, smooth=2, neutral=True, white=255, shifts=(0, 1)):
    img = _page(size)
    bg = _background(size, cell, close, smooth, neutral)
    want, want_stats = M.flatten(img, bg, cell, white=white)
    d_img = _dev(img)
    got_bg = ops.page_background(d_img, cell, close, smooth, neutral)
    assert np.array_equal(got_bg.cpu().numpy(), bg), "background"
    for shift in shifts:                                          # the page on a dword, and one byte past it
        whole, out, lead, n = _guarded((*size, 3), torch.uint8, shift)
        page, stats = ops.page_flatten(d_img, cell, close, smooth, neutral, white, out=out, return_stats=True)
        assert page is out and _guards_untouched(whole, lead, n)
        assert np.array_equal(page.cpu().numpy(), want), ("flatten", shift)                     # byte for byte
        assert stats == want_stats
    assert np.array_equal(d_img.cpu().numpy(), img)               # the input is not written
    return d_img, got_bg, want


def _check_binarize(ops, size, radius=15, kq=51, shifts=(0, 1)):
    img = _page(size)
    want, want_stats = M.binarize(img, radius, kq)
    d_img = _dev(img)
    for shift in shifts:
        whole, out, lead, n = _guarded(size, torch.uint8, shift)
        plane, stats = ops.page_binarize(d_img, radius, kq / 256.0, out=out, return_stats=True)
        assert plane is out and _guards_untouched(whole, lead, n)
        assert np.array_equal(plane.cpu().numpy(), want), ("binarize", shift)
        assert stats == want_stats
    assert np.array_equal(d_img.cpu().numpy(), img)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_kernels_equal_the_model_at_every_size(size):
    from dvd_amd import ops
    _check_flatten(ops, size)
    _check_binarize(ops, size)


@pytest.mark.parametrize("cell", [4, 16, 64])
@pytest.mark.parametrize("close,smooth", [(0, 0), (2, 2), (8, 8), (0, 8), (8, 0)])
def test_background_and_flatten_parameters(cell, close, smooth):
    """33 x 31 is a single cell at s = 64 and a plane narrower than every window at s = 16; 130 x 257 has several tiles of every
    kernel and rows that begin off a dword."""
    from dvd_amd import ops
    for size in ((33, 31), (130, 257)):
        for neutral, white in ((True, 255), (False, 200)):
            _check_flatten(ops, size, cell, close, smooth, neutral, white, shifts=(0,))
    _check_flatten(ops, (97, 61), cell, close, smooth, False, 255, shifts=(1,))
    _check_flatten(ops, (97, 61), cell, close, smooth, True, 200, shifts=(1,))


@pytest.mark.parametrize("radius", [1, 15, 63])
@pytest.mark.parametrize("kq", [0, 51, 256])
def test_binarize_parameters(radius, kq):
    """r = 63 is larger than 33 x 31 and than 64 x 16: every window is the whole page there."""
    from dvd_amd import ops
    for size in ((33, 31), (64, 16), (130, 257)):
        _check_binarize(ops, size, radius, kq, shifts=(0,))
    _check_binarize(ops, (97, 61), radius, kq, shifts=(1,))


def test_constant_pages():
    from dvd_amd import ops
    for v, white in ((0, 200), (255, 255), (77, 255), (77, 131)):
        img = X.constant(65, 17, v)
        want, want_stats = M.flatten(img, white=white)
        got, stats = ops.page_flatten(_dev(img), white=white, return_stats=True)
        assert np.array_equal(got.cpu().numpy(), want) and stats == want_stats
        assert (want == (white if v else 0)).all() and stats["floored"] == (0 if v else 3 * 65 * 17)


def test_equivalent_calls_agree():
    from dvd_amd import ops
    size = (130, 257)
    img = _page(size)
    d_img = _dev(img)
    single = ops.page_flatten(d_img, cell=8, white=240)
    # a given background equals the estimated one
    bg = ops.page_background(d_img, cell=8)
    given, stats = ops.page_flatten(d_img, cell=8, white=240, background=bg, return_stats=True)
    assert torch.equal(given, single) and np.array_equal(bg.cpu().numpy(), _background(size, 8, 2, 2, True))
    # the chain equals the single calls, with and without either stage, and the model
    plane, ink = ops.page_binarize(single, radius=7, k=0.3, return_stats=True)
    page, st = ops.page_clean(d_img, cell=8, white=240, return_stats=True)
    assert torch.equal(page, single) and st == {**stats, "ink": 0}
    both, st = ops.page_clean(d_img, binarize=True, cell=8, white=240, radius=7, k=0.3, return_stats=True)
    assert torch.equal(both, plane) and st == {**stats, **ink}
    want, want_st = M.clean(img, True, True, cell=8, white=240, radius=7, kq=77)
    assert np.array_equal(both.cpu().numpy(), want) and st == want_st
    only, st = ops.page_clean(d_img, flatten=False, binarize=True, radius=7, k=0.3, return_stats=True)
    direct, ink = ops.page_binarize(d_img, radius=7, k=0.3, return_stats=True)
    assert torch.equal(only, direct) and st == {"saturated": 0, "floored": 0, **ink}
    assert torch.equal(ops.page_clean(d_img, binarize=True, cell=8, white=240, radius=7, k=0.3), plane)   # without the counts
    # a gray plane [H,W] equals the gray page [H,W,3]
    gray = torch.from_numpy(M.gray(img)).cuda()
    as_page = gray[:, :, None].expand(*size, 3).contiguous()
    a, b = ops.page_binarize(gray, return_stats=True), ops.page_binarize(as_page, return_stats=True)
    assert torch.equal(a[0], b[0]) and a[1] == b[1] == M.binarize(M.gray(img))[1]
    assert np.array_equal(d_img.cpu().numpy(), img)


def test_tools_end_to_end(tmp_path, capsys):
    from PIL import Image
    from dvd_amd import apply_map, clean_pages, ops
    pages = tmp_path / "pages"
    pages.mkdir()
    imgs = {"a": _page((97, 61)), "b 2": _page((130, 257)), "c": _page((33, 31))}
    for stem, img in imgs.items():
        Image.fromarray(img).save(pages / f"{stem}.png")
    lines = []
    man = clean_pages.clean_pages(str(pages), str(tmp_path / "flat"), cell=8, log=lines.append)
    assert json.loads((tmp_path / "flat" / "manifest.json").read_text()) == man and [d["stem"] for d in man["pages"]] == sorted(imgs)
    for d in man["pages"]:
        want, stats = M.clean(imgs[d["stem"]], True, False, cell=8)
        assert np.array_equal(np.asarray(Image.open(tmp_path / "flat" / d["page"])), want)
        assert {k: d[k] for k in M.STATS} == stats and d["size"] == list(want.shape[:2])
    man = clean_pages.clean_pages(str(pages), str(tmp_path / "bw"), binarize=True, radius=7, k=0.3, log=lines.append)
    for d in man["pages"]:
        want, stats = M.clean(imgs[d["stem"]], True, True, radius=7, kq=77)
        got = np.asarray(Image.open(tmp_path / "bw" / d["page"]))
        assert got.shape == (*want.shape, 3) and all(np.array_equal(got[..., c], want) for c in range(3))
        assert {k: d[k] for k in M.STATS} == stats
    # apply_map --clean flatten on a saved map: the flattened native page
    import sized_fixtures as Z
    flow, src = Z.smooth_flow(8, seed=7), _page((97, 61))
    np.save(tmp_path / "flow_a.npy", flow)
    capsys.readouterr()
    apply_map.main([str(tmp_path / "flow_a.npy"), str(pages / "a.png"), str(tmp_path / "page.png"), "--clean", "flatten"])
    want, stats = ops.page_flatten(ops.unwarp_u8(_dev(flow)[None], _dev(src)), return_stats=True)
    assert np.array_equal(np.asarray(Image.open(tmp_path / "page.png")), want.cpu().numpy())
    assert f"saturated {stats['saturated']}, floored {stats['floored']}, ink 0" in capsys.readouterr().out
