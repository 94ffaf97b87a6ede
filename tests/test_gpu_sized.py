"""Pages at a chosen size on the device: the kernels of sized.hip against tests/sized_model.py - whole buffers,
byte for byte, between guard bytes, inputs untouched - the ragged launch against the single calls, the bound against the native
u8 tail, and the two command-line tools end to end."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sized_model as Z  # noqa: E402
import sized_fixtures as X  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 64                     # bytes on either side of an output, pre-filled
F = np.float32


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


@pytest.mark.parametrize("name", list(X.CASES))
def test_kernels_equal_the_model(name):
    from dvd_amd import ops
    c = X.case(name)
    hp, wp = c["size"]
    flow, src = _dev(c["flow"]), _dev(c["src"])
    for shift in (0, 1):                                          # the page on a dword, and one byte past it
        whole, out, lead, n = _guarded((hp, wp, 3), torch.uint8, shift)
        page, stats = ops.unwarp_u8_sized(flow, src, (hp, wp), scale=c["scale"], max_radius=c["max_radius"], out=out, return_stats=True)
        assert page is out and _guards_untouched(whole, lead, n)
        assert np.array_equal(page.cpu().numpy(), c["page"]), shift                             # byte for byte
        assert stats == c["stats"]
    whole, out, lead, n = _guarded((hp, wp), torch.int16)
    foot = ops.sized_footprint(flow, c["src"].shape[:2], (hp, wp), scale=c["scale"], max_radius=c["max_radius"], out=out)
    assert foot is out and _guards_untouched(whole, lead, n)
    assert np.array_equal(foot.cpu().numpy().view(np.uint16), c["foot"])
    assert np.array_equal(src.cpu().numpy(), c["src"]) and np.array_equal(flow.cpu().numpy().view(np.uint32), c["flow"].view(np.uint32))
    assert torch.equal(ops.unwarp_u8_sized(flow, src, (hp, wp), scale=c["scale"], max_radius=c["max_radius"]), page)   # without the counts


def test_ragged_equals_the_single_calls():
    from dvd_amd import lib, ops
    names = ["smooth_g8_97x61_to_33x130_s0.987_r16", "nan_g8_48x64_to_65x17_s0.987_r16", "smooth_g8_400x300_to_20x15_s0.987_r16",
             "wild_g8_1x1_to_17x65_s0.987_r16"]
    cs = [X.case(n) for n in names]
    assert len({c["src"].shape for c in cs}) == 4 and len({c["size"] for c in cs}) == 4
    flow = _dev(np.stack([c["flow"] for c in cs]))
    srcs = [_dev(c["src"]) for c in cs]
    pages, stats = ops.unwarp_u8_sized_ragged(flow, srcs, [c["size"] for c in cs], return_stats=True)
    for c, page, st in zip(cs, pages, stats):
        assert np.array_equal(page.cpu().numpy(), c["page"]) and st == c["stats"]
    assert ops.unwarp_u8_sized_ragged(flow[:0], [], []) == [] and ops.unwarp_u8_sized_ragged(flow[:0], [], [], return_stats=True) == ([], [])
    # more documents than one launch takes: cut as unwarp_u8_ragged cuts it
    n = lib.RAGGED_CAP + 1
    small = [X.case("smooth_g8_97x61_to_1x5_s0.987_r16"), X.case("smooth_g8_97x61_to_5x1_s0.987_r16"), X.case("smooth_g8_97x61_to_49x31_s0.987_r16")]
    pick = [small[d % 3] for d in range(n)]
    flow = _dev(np.stack([c["flow"] for c in pick]))
    srcs = [_dev(c["src"]) for c in small]
    pages, stats = ops.unwarp_u8_sized_ragged(flow, [srcs[d % 3] for d in range(n)], [c["size"] for c in pick], return_stats=True)
    assert len(pages) == len(stats) == n
    for c, page, st in zip(pick, pages, stats):
        assert np.array_equal(page.cpu().numpy(), c["page"]) and st == c["stats"]


def test_native_tail_bound():
    """At the photograph's own size with max_radius = 1 the sized page is the native u8 tail up to rounding: truncation against
    rounding is below 1 level, the Q8 position is within 1/512 px per axis and bilinear is 255-Lipschitz per axis (below 1
    level), the final rounding adds 0.5: below 2.5, so the integers differ by at most 2."""
    from dvd_amd import ops
    h, w = 97, 61
    flow, src = _dev(X.smooth_flow(8, seed=5)), _dev(X.photograph(h, w, seed=5))
    native = ops.unwarp_u8(flow[None], src).cpu().numpy().astype(int)
    sized, stats = ops.unwarp_u8_sized(flow, src, (h, w), max_radius=1, return_stats=True)
    diff = np.abs(sized.cpu().numpy().astype(int) - native)
    print("sized against the native tail: max", diff.max(), "mean", diff.mean(), stats)
    assert stats["outside"] == 0 and stats["invalid"] == 0
    assert diff.max() <= 2


def test_tools_end_to_end(tmp_path, capsys):
    from PIL import Image
    from dvd_amd import apply_map, render_pages
    h, w = 97, 61
    maps, photos = tmp_path / "pred_flow", tmp_path / "img"
    maps.mkdir()
    photos.mkdir()
    docs = {"12_1 copy": (X.smooth_flow(8, seed=7), X.photograph(h, w, seed=7), "12.png"),
            "b": (X.smooth_flow(8, seed=8), X.photograph(48, 64, seed=8), "b.png")}
    for stem, (flow, src, image) in docs.items():
        np.save(maps / f"flow_{stem}.npy", flow)
        Image.fromarray(src).save(photos / image)
    flow, src, image = docs["12_1 copy"]
    apply_map.main([str(maps / "flow_12_1 copy.npy"), str(photos / image), str(tmp_path / "page.png"), "--size", "long:40"])
    want, stats = Z.unwarp(flow, src, (40, 25))
    got = np.asarray(Image.open(tmp_path / "page.png"))
    assert got.shape == (40, 25, 3) and np.array_equal(got, want)
    line = capsys.readouterr().out
    assert f"capped {stats['capped']}, outside {stats['outside']}, invalid {stats['invalid']}" in line and "40 x 25" in line
    lines = []
    man = render_pages.render_pages(str(maps), str(photos), str(tmp_path / "out"), "x0.5", batch=8, log=lines.append)
    assert json.loads((tmp_path / "out" / "manifest.json").read_text()) == man and len(man["documents"]) == 2
    assert sorted(os.listdir(tmp_path / "out")) == ["12_1 copy.png", "b.png", "manifest.json"]
    for d in man["documents"]:
        flow, src, image = docs[d["stem"]]
        size = (max(1, int(np.floor(src.shape[0] * 0.5 + 0.5))), max(1, int(np.floor(src.shape[1] * 0.5 + 0.5))))
        want, stats = Z.unwarp(flow, src, size)
        assert tuple(d) == render_pages.MANIFEST_KEYS and d["image"] == image
        assert d["photo_size"] == list(src.shape[:2]) and d["page_size"] == list(size)
        assert {k: d[k] for k in Z.STATS} == stats
        assert np.array_equal(np.asarray(Image.open(tmp_path / "out" / d["page"])), want)
