"""Pages at a chosen size on the CPU: tests/sized_model.py - the definition - against what it must satisfy
exactly (identity, no aliasing, constancy), against torch's grid_sample and against float64; the sanitised restatement
sized_host_check.cpp against the model byte for byte; and what the library, ops and the two command-line tools do without a
device."""
import json
import os
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sized_model as Z  # noqa: E402
import sized_fixtures as X  # noqa: E402
from host_check import build_host_check  # noqa: E402

F = np.float32
ZERO = np.zeros((2, 8, 8), F)


# ---- the definition ------------------------------------------------------------------------------------------------------------------
def test_tent_weights_and_bounds():
    """The weights of an integer half-width add up to exactly 256 r^2 at every sub-pixel offset, negative positions included, so
    65536 rx^2 ry^2 is the weight sum of all taps; at radius 16 a row's sum stays within 2^24 and q2 within 65536."""
    for r in (1, 2, 3, 16):
        s = np.arange(-256 * 3, 256 * 3)
        cols, wgt, inside = Z.tent_taps(s, r, 4)
        assert wgt.shape == (len(s), 2 * r) and (wgt >= 0).all() and (wgt.sum(axis=1) == 256 * r * r).all(), r
        assert np.array_equal(inside, (cols >= 0) & (cols < 4))
    assert 256 * 16 * 16 * 255 < 2 ** 24 and 16 ** 4 == 65536 and 65536 * 16 ** 4 * 255 < 2 ** 40
    white = np.full((40, 40, 3), 255, np.uint8)                                              # the largest accumulator there is
    assert (Z.sample(white, np.array([256 * 20 + 77]), np.array([256 * 19 + 200]), np.array([16]), np.array([16])) == 255).all()


def test_definition_details():
    # the Q8 position: floor(256 x + 1/2), clamped 17 pixels outside; x = (g + 1) ((n - 1) / 2)
    g = np.array([-1, 1, 0, -1.5, 3, 5, 1e30, -1e30, np.inf], F)
    valid = np.isfinite(g)
    assert Z.q8_of(g, 11, valid).tolist() == [0, 2560, 1280, -640, 5120, 256 * 27, 256 * 27, -256 * 17, 0]
    assert Z.q8_of(np.array([0.5], F), 1, np.array([True])).tolist() == [0]                   # a photograph of one pixel
    # radii: a half rounds down, never below 1, capped at max_radius - and the cap is reported
    assert Z.radius_raw(np.array([0, 768, 769, 512 * 16 + 256, 512 * 40]), np.zeros(5, int)).tolist() == [1, 1, 2, 16, 40]
    # the same grid as the native tail at the photograph's own size
    import mapinv_model as MI
    flow = X.smooth_flow(8, seed=1)
    qx, qy, valid = Z.positions(flow, (37, 29), (37, 29))
    x, y = MI.positions(flow, 37, 29)
    assert valid.all() and np.abs(qx / 256 - x).max() <= 1 / 512 + 1e-4 and np.abs(qy / 256 - y).max() <= 1 / 512 + 1e-4
    # an invalid pixel is black, counted, and its neighbours' differences go without it
    flow = ZERO.copy()
    flow[0, 0, 0] = np.nan
    src = np.full((16, 16, 3), 200, np.uint8)
    page, stats = Z.unwarp(flow, src, (16, 16), scale=0.9)
    foot = Z.footprint(flow, (16, 16), (16, 16), scale=0.9)
    dead = foot == 0
    assert stats == dict(capped=0, outside=0, invalid=int(dead.sum())) and 0 < dead.sum() < 20
    assert (page[dead] == 0).all() and (page[~dead] == 200).all() and (foot[~dead] == 1 | 1 << 8).all()


@pytest.mark.parametrize("side", [1, 2, 3, 17, 64, 97, 255, 256])
def test_identity(side):
    """flow = 0, scale = 1, the page of the photograph's size: every Q8 position is a multiple of 256 (the f32 position is off by
    about 1e-4 px at these sizes, against the 1/512 that would flip the rounding), every radius 1: the page IS the photograph."""
    for h, w in ((side, side), (side, max(1, 257 - side)), (max(1, side // 2), side)):
        src = X.photograph(h, w, seed=side)
        qx, qy, valid = Z.positions(ZERO, (h, w), (h, w), scale=1.0)
        assert valid.all() and np.array_equal(qx, np.broadcast_to(256 * np.arange(w)[None, :], (h, w))) and \
            np.array_equal(qy, np.broadcast_to(256 * np.arange(h)[:, None], (h, w))), (h, w)
        page, stats = Z.unwarp(ZERO, src, (h, w), scale=1.0)
        assert np.array_equal(page, src) and stats == dict(capped=0, outside=0, invalid=0), (h, w)


@pytest.mark.parametrize("axis", [1, 0])
def test_no_aliasing(axis):
    """One-pixel stripes 0 / 255 at half the size.  Derived on paper: the derivative across the stripes is 63 / 31, so the radius
    is 2, and a tent of half-width 2 over period-2 stripes weighs even and odd lines 2 : 2 at every phase - the mean 127.5
    rounds to 128 at every pixel at least two pixels from the two edges the stripes run towards.  ALONG the stripes the tent
    of the first and the last page line reaches one line outside the photograph, which holds 256 of the 1024 weights and
    contributes zero (padding_mode='zeros'): those two lines are exactly 127.5 * 3 / 4 = 95.625 -> 96, every other line 128.
    With max_radius = 1 the same call is point-sampled bilinear: a moire ramp 255 frac(2.032 j)."""
    src = np.zeros((64, 64, 3), np.uint8)
    if axis == 1:
        src[:, 1::2] = 255                                                                    # vertical stripes
    else:
        src[1::2, :] = 255
    assert (Z.footprint(ZERO, (64, 64), (32, 32), scale=1.0) == (2 | 2 << 8)).all()
    page, stats = Z.unwarp(ZERO, src, (32, 32), scale=1.0)
    across = page if axis == 1 else page.transpose(1, 0, 2)                                   # [along, across, 3]
    assert (across[1:-1, 2:-2] == 128).all() and stats == dict(capped=0, outside=0, invalid=0)
    assert (across[[0, -1], 2:-2] == 96).all()
    point, stats = Z.unwarp(ZERO, src, (32, 32), scale=1.0, max_radius=1)
    ramp = (point if axis == 1 else point.transpose(1, 0, 2))[5, :, 0].astype(int)
    assert ramp.max() - ramp.min() >= 200 and stats["capped"] == 32 * 32
    want = 255 * np.modf(np.arange(32) * 63 / 31 / 2)[0] * 2                                  # 255 frac(2.032 j / 2) 2: the stripe's phase
    assert np.abs(ramp - np.where(want > 255, 510 - want, want)).max() <= 2


@pytest.mark.parametrize("size", [(61, 47), (30, 23), (12, 9)])
def test_constancy(size):
    """A constant photograph under a smooth map that stays inside the frame gives exactly that constant wherever the footprint
    lies inside the photograph: the weights add up to the divisor exactly."""
    H, W = 61, 47
    flow = X.smooth_flow(8, seed=4)
    rx, ry, _, _, qx, qy, valid = Z.footprint(flow, (H, W), size, detail=True)
    inside = valid & ((qx >> 8) - rx + 1 >= 0) & ((qx >> 8) + rx <= W - 1) & ((qy >> 8) - ry + 1 >= 0) & ((qy >> 8) + ry <= H - 1)
    assert inside.mean() > 0.5 and max(rx.max(), ry.max()) == {(61, 47): 1, (30, 23): 2, (12, 9): 6}[size]
    for c in (1, 77, 254, 255):
        page, _ = Z.unwarp(flow, np.full((H, W, 3), c, np.uint8), size)
        assert (page[inside] == c).all(), c


def test_against_the_native_tail():
    """Page size = photograph size, max_radius = 1: against torch's CPU grid_sample of the native tail's grid, truncated as the
    native u8 tail truncates.  Truncation against rounding is below 1 level; the Q8 position is within 1/512 px per axis and
    bilinear is 255-Lipschitz per axis, below 1 level; the final rounding adds 0.5: below 2.5, so the integers differ by at
    most 2."""
    import mapinv_model as MI
    h, w = 97, 61
    flow, src = X.smooth_flow(8, seed=5), X.photograph(h, w, seed=5)
    gx, gy = MI.grid(flow, h, w)
    grid = torch.from_numpy(np.stack([gx, gy], axis=-1))[None]
    img = torch.from_numpy(src.astype(F)).permute(2, 0, 1)[None]
    native = torch.nn.functional.grid_sample(img, grid, mode="bilinear", padding_mode="zeros", align_corners=True)[0].permute(1, 2, 0)
    native = native.numpy().astype(np.uint8).astype(int)
    sized, stats = Z.unwarp(flow, src, (h, w), max_radius=1)
    diff = np.abs(sized.astype(int) - native)
    print("sized against the truncated grid_sample: max", diff.max(), "mean", diff.mean())
    assert stats["outside"] == 0 and stats["invalid"] == 0 and diff.max() <= 2


# measured on this model (maximum, mean) in levels, recorded in DESIGN 4.16; the bar is 4 x the maximum
FLOAT64_MEASURED = {"mild": (1.0175, 0.268), "minify_2": (0.6217, 0.250), "minify_5": (0.5344, 0.248)}
FLOAT64_MAPS = {"mild": ((97, 61), (97, 61)), "minify_2": ((97, 61), (49, 31)), "minify_5": ((200, 150), (40, 30))}


@pytest.mark.parametrize("name", list(FLOAT64_MAPS))
def test_against_float64(name):
    """The model against the same tent - the same integer radii - evaluated in float64 at positions that were never quantised
    (sized_model.positions64: exact rational coordinates), on random bytes.  What differs is the Q8 position, up to 1/512 px
    per axis, and the one rounding."""
    src_hw, size = FLOAT64_MAPS[name]
    flow, src = X.smooth_flow(8, seed=11), X.photograph(*src_hw, seed=3)
    page, stats = Z.unwarp(flow, src, size)
    rx, ry, _, _, qx, qy, valid = Z.footprint(flow, src_hw, size, detail=True)
    x, y = Z.positions64(flow, src_hw, size)
    assert valid.all() and np.abs(qx / 256 - x).max() <= 1 / 512 + 2e-4 and np.abs(qy / 256 - y).max() <= 1 / 512 + 2e-4
    want = Z.tent64(src, x.ravel(), y.ravel(), rx.ravel(), ry.ravel()).reshape(*size, 3)
    diff = np.abs(page.astype(np.float64) - want)
    print(name, "radii", np.unique(rx).tolist(), np.unique(ry).tolist(), "max", diff.max(), "mean", diff.mean(), "recorded", FLOAT64_MEASURED[name])
    assert {"mild": 1, "minify_2": 2, "minify_5": 5}[name] in np.unique(rx)
    assert diff.max() <= 4 * FLOAT64_MEASURED[name][0]


def test_hostile_maps():
    """NaN and infinite entries, a page thrown off the photograph, derivatives far above the cap: black pixels and exact counts,
    and never more than (2 * 16)^2 taps per pixel."""
    c = X.case("nan_g8_48x64_to_65x17_s0.987_r16")
    import mapinv_model as MI
    gx, gy = MI.grid(c["flow"], 65, 17)
    dead = ~(np.isfinite(gx) & np.isfinite(gy))
    assert 0 < dead.sum() < dead.size and c["stats"]["invalid"] == int(dead.sum())
    assert (c["page"][dead] == 0).all() and (c["foot"][dead] == 0).all() and (c["foot"][~dead] != 0).all()
    c = X.case("off_g8_48x64_to_17x65_s0.987_r16")
    assert c["stats"] == dict(capped=0, outside=17 * 65, invalid=0) and (c["page"] == 0).all()
    c = X.case("steep_g16_400x300_to_20x15_s0.987_r4")
    rx, ry, ux, uy, _, _, valid = Z.footprint(c["flow"], (400, 300), (20, 15), max_radius=4, detail=True)
    assert valid.all() and max(ux.max(), uy.max()) > 40 and rx.max() == ry.max() == 4
    assert c["stats"]["capped"] == int(((ux > 4) | (uy > 4)).sum()) == 300
    for name in X.CASES:
        foot = X.case(name)["foot"]
        assert (foot & 255).max() <= X.case(name)["max_radius"] and (foot >> 8).max() <= X.case(name)["max_radius"] <= Z.MAX_RADIUS


def test_cases_cover_what_they_are_named_for():
    radii = lambda name: set(np.unique(X.case(name)["foot"] & 255)) | set(np.unique(X.case(name)["foot"] >> 8))   # noqa: E731
    assert radii("smooth_g8_48x64_to_97x131_s0.987_r16") == {1} and radii("smooth_g8_97x61_to_49x31_s0.987_r16") == {2}
    assert radii("smooth_g16_97x61_to_33x21_s0.987_r16") == {3} and radii("zero_g2_400x300_to_25x19_s0.987_r16") == {16}
    assert X.case("zero_g2_400x300_to_25x19_s0.987_r16")["stats"]["capped"] == 0 and X.case("zero_g2_400x300_to_20x15_s0.987_r16")["stats"]["capped"] == 300
    sizes = {c[3] for c in X.CASES.values()}
    assert {(1, 1), (1, 5), (7, 1), (3, 2), (15, 63), (16, 64), (17, 65), (33, 130), (63, 15), (64, 16), (65, 17), (130, 33)} <= sizes
    assert {c[2] for c in X.CASES.values()} >= {(1, 1), (2, 2), (48, 64), (97, 61)} and {c[1] for c in X.CASES.values()} == {2, 8, 16}
    assert {c[5] for c in X.CASES.values()} == {1, 4, 16}
    assert any(sum(c[3]) <= 128 for c in X.CASES.values()) and any(sum(c[3]) > 128 for c in X.CASES.values())
    assert {w for _, w in sizes} >= {1, 2, 3, 5, 7} and {(3 * w) % 4 for h, w in sizes if h > 1 and w >= 4} == {0, 1, 2, 3}


# ---- the sanitised CPU restatement ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("sized_host_check")
    exe = build_host_check("sized", tmp)

    def run(flow, src, size, scale, max_radius, dims=None, alias=0):
        g, hs, ws, hp, wp = dims if dims else (flow.shape[-1], *src.shape[:2], *size)
        head = struct.pack("<7if", g, hs, ws, hp, wp, max_radius, alias, scale)
        (tmp / "in.bin").write_bytes(head + np.ascontiguousarray(flow, F).tobytes() + np.ascontiguousarray(src, np.uint8).tobytes())
        out = tmp / "out.bin"
        if out.exists():
            out.unlink()
        p = subprocess.run([str(exe), str(tmp / "in.bin"), str(out)], capture_output=True, text=True)
        assert p.returncode == 0 and p.stderr == "", (p.returncode, p.stderr[-2000:])          # a status, never a sanitizer report
        return int(p.stdout), (out.read_bytes() if out.exists() else None)
    return run


@pytest.mark.parametrize("name", list(X.CASES))
def test_host_check_equals_the_model(host_check, name):
    c = X.case(name)
    hp, wp = c["size"]
    n = hp * wp
    status, out = host_check(c["flow"], c["src"], c["size"], c["scale"], c["max_radius"])
    assert status == 0 and len(out) == 5 * n + 24
    assert np.array_equal(np.frombuffer(out, np.uint8, 3 * n).reshape(hp, wp, 3), c["page"])               # byte for byte
    assert np.array_equal(np.frombuffer(out[3 * n:5 * n], np.uint16).reshape(hp, wp), c["foot"])
    assert np.frombuffer(out[5 * n:], np.uint64).tolist() == [c["stats"][k] for k in Z.STATS]


def test_host_check_refuses_with_a_status(host_check):
    flow, src = np.zeros((2, 4, 4), F), np.zeros((5, 5, 3), np.uint8)
    for dims in ((4, 0, 5, 3, 3), (4, 5, 16385, 3, 3), (4, 5, 5, 0, 3), (4, 5, 5, 3, 16385), (1, 5, 5, 3, 3), (8193, 5, 5, 3, 3), (4, -1, 5, 3, 3)):
        assert host_check(flow, src, None, 0.987, 16, dims) == (-59, None)
    for scale, max_radius in ((np.nan, 16), (np.inf, 16), (0.987, 0), (0.987, 17), (0.987, -1)):
        assert host_check(flow, src, (3, 3), scale, max_radius) == (-60, None)
    assert host_check(flow, src, (3, 3), 0.987, 16, alias=1) == (-1, None)                     # the page over the photograph
    status, out = host_check(flow, src, (3, 3), 0.987, 1)
    assert status == 0 and len(out) == 45 + 24


# ---- the library's and the wrappers' refusals: before any HIP call, so they run here ------------------------------------------------
def test_entry_points_refuse_before_any_launch():
    import ctypes as C
    from dvd_amd import lib
    raw = lib.raw()
    buf = (C.c_char * 4096)()
    base = (C.addressof(buf) + 63) & ~63                                                      # host memory: never dereferenced
    flow, src, out, stats = base, base + 1024, base + 2048, base + 3072
    sized = lambda g=4, hs=5, ws=5, hp=3, wp=3, scale=0.987, r=16, f=flow, s=src, o=out: raw.dvd_unwarp_u8_sized(   # noqa: E731
        f, g, s, hs, ws, o, hp, wp, C.c_float(scale), r, stats, None)
    foot = lambda g=4, hs=5, ws=5, hp=3, wp=3, scale=0.987, r=16, f=flow, o=out: raw.dvd_sized_footprint(   # noqa: E731
        f, g, hs, ws, hp, wp, C.c_float(scale), r, o, None)
    for bad in (dict(hs=0), dict(ws=16385), dict(hp=0), dict(wp=16385), dict(g=1), dict(g=8193)):
        assert sized(**bad) == -59 and b"unwarp_u8_sized" in raw.dvd_last_error() and b"sides 1..16384" in raw.dvd_last_error()
        assert foot(**bad) == -59 and b"sized_footprint" in raw.dvd_last_error()
    for bad in (dict(scale=float("nan")), dict(scale=float("inf")), dict(r=0), dict(r=17)):
        assert sized(**bad) == -60 and b"max_radius 1..16" in raw.dvd_last_error()
        assert foot(**bad) == -60
    for bad in (dict(f=None), dict(s=None), dict(o=None)):
        assert sized(**bad) == -1 and b"null" in raw.dvd_last_error()
    assert foot(f=None) == -1 and foot(o=None) == -1 and foot(o=out + 1) == -1
    assert sized(o=src) == -1 and b"share no byte" in raw.dvd_last_error()
    assert sized(o=src + 74) == -1 and sized(s=out + 26) == -1                                  # the last byte of one on the first of the other
    docs = (lib.SizedImage * 2)()
    for d in docs:
        d.src, d.out, d.hs, d.ws, d.hp, d.wp = src, out, 5, 5, 3, 3
    ragged = lambda n=2, g=4, scale=0.987, r=16, f=flow, t=docs: raw.dvd_unwarp_u8_sized_ragged(f, g, t, n, C.c_float(scale), r, stats, None)   # noqa: E731
    assert ragged(f=None) == -1 and ragged(t=None) == -1 and ragged(n=-1) == -1
    assert ragged(r=17) == -60 and ragged(scale=float("nan")) == -60 and ragged(g=1) == -59
    docs[1].wp = 0
    assert ragged() == -59 and b"document 1" in raw.dvd_last_error()
    docs[1].wp, docs[1].out = 3, None
    assert ragged() == -1 and b"document 1" in raw.dvd_last_error()
    docs[1].out = src + 10
    assert ragged() == -1 and b"share no byte" in raw.dvd_last_error()
    docs[1].out = out + 3                                                                      # over document 0's page
    assert ragged() == -1 and b"document 1" in raw.dvd_last_error() and b"document 0" in raw.dvd_last_error()
    docs[1].out, docs[0].src = out + 512, out + 512 + 20                                       # over document 0's photograph
    assert ragged() == -1 and b"src or out of document" in raw.dvd_last_error()
    assert ragged(n=0) == 0                                                                    # nothing to do: no HIP call
    assert (lib.E_SIZED_SHAPE, lib.E_SIZED_PARAM, lib.SIZED_STATS) == (-59, -60, 3)


def test_ops_refuse_bad_arguments_and_host_tensors():
    from dvd_amd import lib, ops
    flow, src = torch.zeros(2, 8, 8), torch.zeros(6, 5, 3, dtype=torch.uint8)
    for bad in ((3,), (3, 4.0), "3x4", (0, 4), (3, 16385), (True, 4), None):
        for call in (lambda: ops.unwarp_u8_sized(flow, src, bad), lambda: ops.sized_footprint(flow, (6, 5), bad),
                     lambda: ops.unwarp_u8_sized_ragged(flow[None], [src], [bad])):
            with pytest.raises((ValueError, lib.DvdError), match="size"):
                call()
    for bad in (0, 17, 1.0, True, "4"):
        with pytest.raises(ValueError, match="max_radius must be an integer 1..16"):
            ops.unwarp_u8_sized(flow, src, (3, 4), max_radius=bad)
        with pytest.raises(ValueError, match="max_radius"):
            ops.sized_footprint(flow, (6, 5), (3, 4), max_radius=bad)
    for bad in (float("nan"), float("inf"), "1", True):
        with pytest.raises(ValueError, match="scale must be a finite number"):
            ops.unwarp_u8_sized(flow, src, (3, 4), scale=bad)
    for bad in ((6,), (6, 5.0), "6x5"):
        with pytest.raises(ValueError, match="sized_footprint: src_hw"):
            ops.sized_footprint(flow, bad, (3, 4))
    with pytest.raises(ValueError, match="on the device"):                                   # host tensors: no CPU path
        ops.unwarp_u8_sized(flow, src, (3, 4))
    with pytest.raises(ValueError, match="on the device"):
        ops.sized_footprint(flow, (6, 5), (3, 4))
    with pytest.raises(ValueError, match="on the device"):
        ops.unwarp_u8_sized_ragged(flow[None], [src], [(3, 4)])
    for bad in (src, "src", src.float()):                                                      # a host photograph too is a ValueError
        with pytest.raises(ValueError, match="src_hwc must be"):
            ops._sized_src(bad, "unwarp_u8_sized")
    assert ops.parse_page_size("x20") == ("scale", 20.0) and ops.parse_page_size("long:7") == ("long", 7) and ops.parse_page_size((0, 5)) == ("size", 0, 5)
    assert ops.page_size(97, 61, "x20") == (1940, 1220)
    assert ops.SIZED_MAX_RADIUS == Z.MAX_RADIUS and ops.SIZED_STATS == Z.STATS and ops.SIZED_MAX_SIDE == Z.MAX_SIDE


# ---- page_size ---------------------------------------------------------------------------------------------------------------------
def test_page_size():
    from dvd_amd.ops import page_size
    assert page_size(97, 61, (5, 7)) == (5, 7) and page_size(97, 61, [16384, 1]) == (16384, 1)
    assert page_size(97, 61, "40x25") == (40, 25) and page_size(97, 61, " 1X16384 ") == (1, 16384)
    # long:N - the long side becomes N, the other rounds to nearest (a half up), at least 1
    assert page_size(97, 61, "long:40") == (40, 25) and page_size(61, 97, "long:40") == (25, 40)          # 25.15
    assert page_size(3508, 2480, "long:1600") == (1600, 1131) and page_size(100, 100, "long:7") == (7, 7)   # 1131.13
    assert page_size(4, 2, "long:3") == (3, 2) and page_size(2, 4, "long:3") == (2, 3)                    # 1.5 -> 2
    assert page_size(1000, 3, "long:10") == (10, 1) and page_size(3, 1000, "long:10") == (1, 10)          # 0.03 -> 1
    assert page_size(5, 5, "long:16384") == (16384, 16384)
    # xF - both sides scaled and rounded, at least 1
    assert page_size(97, 61, "x0.5") == (49, 31) and page_size(3508, 2480, "x0.125") == (439, 310)        # 48.5 -> 49, 438.5 -> 439
    assert page_size(97, 61, "x2") == (194, 122) and page_size(97, 61, "x.25") == (24, 15) and page_size(3, 3, "x0.01") == (1, 1)
    assert page_size(97, 61, "X1.") == (97, 61)
    for bad in ("", "40", "40x", "x", "0x5", "5x0", "16385x1", "long:0", "long:", "long:-3", "long:4.5", "long:99999", "x0", "x-1", "x1e3",
                "x1000", "40x25x3", "wide:40", "40 x 25", None, 5, 2.0, (1,), (1, 2, 3), (1.0, 2), (True, 2), (0, 5), (5, 16385), b"4x4"):
        with pytest.raises(ValueError) as e:
            page_size(97, 61, bad)
        assert repr(bad) in str(e.value), bad
    for h, w in ((0, 5), (5, 0), (5.0, 5), (True, 5)):
        with pytest.raises(ValueError, match="photograph"):
            page_size(h, w, "x1")


# ---- apply_map ---------------------------------------------------------------------------------------------------------------------
def _fake_device(monkeypatch):
    monkeypatch.setattr(torch.Tensor, "cuda", lambda self, *a, **k: self)


def test_apply_map_size_flag(tmp_path, monkeypatch, capsys):
    from PIL import Image
    from dvd_amd import apply_map as A, ops
    flow, src = X.smooth_flow(8, seed=7), X.photograph(97, 61, seed=7)
    np.save(tmp_path / "m.npy", flow)
    Image.fromarray(src).save(tmp_path / "in.png")
    _fake_device(monkeypatch)
    seen = []

    def native(flow_, src_, *args, **kw):
        seen.append(("unwarp_u8", tuple(flow_.shape), tuple(src_.shape), args, kw))
        return src_

    def sized(flow_, src_, size, **kw):
        seen.append(("unwarp_u8_sized", tuple(flow_.shape), tuple(src_.shape), size, kw))
        page, stats = Z.unwarp(flow_.numpy(), src_.numpy(), size, max_radius=kw["max_radius"])
        return torch.from_numpy(page), stats
    monkeypatch.setattr(ops, "unwarp_u8", native)
    monkeypatch.setattr(ops, "unwarp_u8_sized", sized)
    args = [str(tmp_path / "m.npy"), str(tmp_path / "in.png"), str(tmp_path / "out.png")]
    A.main(args)                                                                               # no --size: today's call, untouched
    A.main(args + ["--mode", "bicubic"])
    assert seen == [("unwarp_u8", (1, 2, 8, 8), (97, 61, 3), (), {"mode": "bilinear"}), ("unwarp_u8", (1, 2, 8, 8), (97, 61, 3), (), {"mode": "bicubic"})]
    assert np.array_equal(np.asarray(Image.open(tmp_path / "out.png")), src) and capsys.readouterr().out == ""
    seen.clear()
    A.main(args + ["--size", "long:40", "--max-radius", "4"])
    assert seen == [("unwarp_u8_sized", (2, 8, 8), (97, 61, 3), (40, 25), {"max_radius": 4, "return_stats": True})]
    want, stats = Z.unwarp(flow, src, (40, 25), max_radius=4)
    assert np.array_equal(np.asarray(Image.open(tmp_path / "out.png")), want)
    line = capsys.readouterr().out
    assert line.count("\n") == 1 and f"capped {stats['capped']}, outside {stats['outside']}, invalid {stats['invalid']}" in line
    seen.clear()
    (tmp_path / "pts.txt").write_text("1 2\n")
    for extra, text in ((["--size", "x0.5", "--mode", "bicubic"], "--mode bicubic"), (["--size", "x0.5", "--points", str(tmp_path / "pts.txt")], "--points"),
                        (["--size", "huge"], "'huge'"), (["--size", "x0.5", "--max-radius", "17"], "--max-radius must be"), (["--max-radius", "4"], "needs --size")):
        with pytest.raises(SystemExit) as e:
            A.main(args[:2] + [str(tmp_path / "never.png")] + extra)
        assert e.value.code == 2 and text in capsys.readouterr().err, extra
    assert not seen                                                                            # refused before the device is asked
    np.save(tmp_path / "broken.npy", np.zeros((3, 4)))
    with pytest.raises(ValueError, match="broken.npy"):                                        # not a usage error: the file's own fault
        A.main([str(tmp_path / "broken.npy"), args[1], str(tmp_path / "never.png"), "--size", "x0.5"])
    with pytest.raises(SystemExit):                                                            # legal as a request, not for this photograph
        A.main(args[:2] + [str(tmp_path / "never.png"), "--size", "x500"])
    assert "97 x 61" in capsys.readouterr().err
    assert not (tmp_path / "never.png").exists()


# ---- render_pages ------------------------------------------------------------------------------------------------------------------
class ModelBackend:
    """render_pages' device, played by the NumPy model."""

    def __init__(self):
        self.calls = []

    def size(self, path):
        from PIL import Image
        with Image.open(path) as im:
            return im.size[1], im.size[0]

    def load(self, path):
        from PIL import Image
        return np.asarray(Image.open(path).convert("RGB"))

    def render(self, flows, photos, sizes, max_radius):
        self.calls.append([tuple(s) for s in sizes])
        got = [Z.unwarp(f, p, s, max_radius=max_radius) for f, p, s in zip(flows, photos, sizes)]
        return [g[0] for g in got], [g[1] for g in got]

    def write(self, page, path, fmt, quality):
        from PIL import Image
        Image.fromarray(page).save(path, quality=quality) if fmt == "jpeg" else Image.fromarray(page).save(path)

    def shape(self, photo):
        return int(photo.shape[0]), int(photo.shape[1])


def test_render_pages_matches_stems_and_skips(tmp_path, capsys):
    from PIL import Image
    from dvd_amd import render_pages as R
    maps, photos = tmp_path / "pred_flow", tmp_path / "img"
    maps.mkdir()
    photos.mkdir()
    docs = {"12_1 copy": ((30, 22), "12.JPG"), "7": ((24, 31), "7.png"), "lost": (None, None), "page_3": ((17, 40), "page_3.jpeg")}
    for k, (stem, (hw, image)) in enumerate(docs.items()):
        np.save(maps / f"flow_{stem}.npy", X.smooth_flow(8, seed=20 + k))
        if image:
            Image.fromarray(X.photograph(*hw, seed=20 + k)).save(photos / image, **({} if image.endswith("png") else {"quality": 95}))
    np.save(maps / "other.npy", np.zeros(3))                                                   # not a map of the run
    (photos / "7.txt").write_text("not an image")
    assert [s for s, _ in R.find_maps(str(maps))] == ["12_1 copy", "7", "lost", "page_3"]
    assert R.find_photograph(str(photos), "12_1 copy") == str(photos / "12.JPG") and R.find_photograph(str(photos), "lost") is None
    assert R.find_photograph(str(photos), "7") == str(photos / "7.png")
    lines, backend = [], ModelBackend()
    man = R.render_pages(str(maps), str(photos), str(tmp_path / "out"), "long:12", fmt="png", batch=2, max_radius=8, log=lines.append, backend=backend)
    assert json.loads((tmp_path / "out" / "manifest.json").read_text()) == man
    assert (man["size"], man["format"], man["quality"], man["max_radius"]) == ("long:12", "png", None, 8)
    assert [d["stem"] for d in man["documents"]] == ["12_1 copy", "7", "page_3"]
    assert sum("skipped: no photograph" in ln and "flow_lost.npy" in ln for ln in lines) == 1 and len(lines) == 4
    assert backend.calls == [[(12, 9), (9, 12)], [(5, 12)]]                                     # --batch 2: two launches
    for d in man["documents"]:
        hw, image = docs[d["stem"]]
        assert tuple(d) == R.MANIFEST_KEYS and (d["map"], d["image"], d["page"]) == (f"flow_{d['stem']}.npy", image, d["stem"] + ".png")
        src = backend.load(photos / image)
        want, stats = Z.unwarp(np.load(maps / d["map"]), src, tuple(d["page_size"]), max_radius=8)
        assert d["photo_size"] == list(hw) and {k: d[k] for k in Z.STATS} == stats
        assert np.array_equal(np.asarray(Image.open(tmp_path / "out" / d["page"])), want)
    assert sorted(os.listdir(tmp_path / "out")) == ["12_1 copy.png", "7.png", "manifest.json", "page_3.png"]
    man = R.render_pages(str(maps), str(photos), str(tmp_path / "jpg"), (10, 8), fmt="jpeg", quality=80, log=lines.append, backend=ModelBackend())
    assert man["quality"] == 80 and all(d["page"].endswith(".jpg") and d["page_size"] == [10, 8] for d in man["documents"])
    assert Image.open(tmp_path / "jpg" / "7.jpg").size == (8, 10)
    # a request is weighed against every document's own photograph before the first launch: x600 suits the 2 x 3 one alone
    class Blank(ModelBackend):
        def render(self, flows, photos, sizes, max_radius):
            self.calls.append([tuple(s) for s in sizes])
            return [np.zeros((*s, 3), np.uint8) for s in sizes], [dict.fromkeys(Z.STATS, 0) for _ in sizes]
    Image.fromarray(X.photograph(2, 3, seed=1)).save(photos / "lost.png")
    lines, backend = [], Blank()
    man = R.render_pages(str(maps), str(photos), str(tmp_path / "big"), "x600", log=lines.append, backend=backend)
    assert backend.calls == [[(1200, 1800)]] and [d["stem"] for d in man["documents"]] == ["lost"]
    assert sum("skipped" in ln and "it asks for" in ln for ln in lines) == 3 and sorted(os.listdir(tmp_path / "big")) == ["lost.png", "manifest.json"]
    os.remove(photos / "lost.png")
    for argv, text in (([str(maps), str(photos), str(tmp_path / "no"), "--size", "huge"], "'huge'"),
                       ([str(maps), str(photos), str(tmp_path / "no"), "--size", "x0.5", "--batch", "0"], "--batch"),
                       ([str(maps), str(photos), str(tmp_path / "no"), "--size", "x0.5", "--quality", "0"], "--quality"),
                       ([str(maps), str(photos), str(tmp_path / "no"), "--size", "x0.5", "--max-radius", "17"], "--max-radius"),
                       ([str(maps), str(photos), str(tmp_path / "no"), "--size", "x0.5", "--format", "gif"], "invalid choice"),
                       ([str(maps), str(photos), str(tmp_path / "no")], "--size"),
                       ([str(tmp_path / "none"), str(photos), str(tmp_path / "no"), "--size", "x0.5"], "MAP_DIR must be a directory"),
                       ([str(photos), str(photos), str(tmp_path / "no"), "--size", "x0.5"], "holds no flow_")):
        with pytest.raises(SystemExit) as e:
            R.main(argv)
        assert e.value.code == 2 and text in capsys.readouterr().err, argv
    assert not (tmp_path / "no").exists()                                                      # refused before anything is written
