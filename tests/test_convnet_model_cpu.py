"""CPU checks of the executor tests' own reference (tests/convnet_model.py) and of the executor's HOST side: the float32
model equals plain torch.nn modules on a net that uses every op kind, its float64 run agrees, abs_conv is what it says, and
the route the library stores per conv (dvd_convnet_op_info) is the dispatch rule written out independently here."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from convnet_model import abs_conv, add_conv, interpret
from dvd_amd import lib, prestage, synth


def _fill(name, shape):
    return torch.from_numpy(synth.uniform("cnmodel/" + name, shape, -0.5, 0.5, 3))


def _tiny():
    """Every op kind: dilated conv, two-source 1x1 conv, strided 7x7 / 3x3 (dilated) / 1x1 convs, both pools, both resizes
    (to a slot's size and to an explicit size), add with and without ReLU, InstanceNorm with and without ReLU, sigmoid."""
    P, sd = prestage.Program(3), {}
    s = {}
    s["c1"] = add_conv(P, sd, 0, 8, _fill, 3, 2, True)
    s["pc"] = P.pool(s["c1"], True)
    s["pf"] = P.pool(s["c1"], False)
    s["up"] = P.resize_like(s["pc"], s["c1"], False)
    s["cat"] = add_conv(P, sd, s["up"], 5, _fill, 1, 1, False, s["c1"])
    s["s7"] = add_conv(P, sd, 0, 6, _fill, 7, 1, False, -1, 2)
    s["n1"] = P.instnorm(s["s7"], True)
    s["s3"] = add_conv(P, sd, s["n1"], 6, _fill, 3, 2, True, -1, 2)
    s["s1"] = add_conv(P, sd, s["n1"], 6, _fill, 1, 1, False, -1, 2)
    s["n2"] = P.instnorm(s["s1"], False)
    s["ar"] = P.add(s["n2"], s["s3"], relu=True)
    s["ap"] = P.add(s["n2"], s["s3"])
    s["rt"] = P.resize_to(s["ap"], 9, 4, True)
    s["sg"] = P.sigmoid(s["rt"])
    return P, sd, s


class _Torch(nn.Module):
    """The same net from torch.nn modules."""

    def __init__(self, sd):
        super().__init__()
        mk = lambda k, cin, cout, ks, dil, stride: self._conv(sd, k, cin, cout, ks, dil, stride)  # noqa: E731
        self.c1, self.cat = mk(0, 3, 8, 3, 2, 1), mk(1, 16, 5, 1, 1, 1)
        self.s7, self.s3, self.s1 = mk(2, 3, 6, 7, 1, 2), mk(3, 6, 6, 3, 2, 2), mk(4, 6, 6, 1, 1, 2)
        self.pc, self.pf = nn.MaxPool2d(2, stride=2, ceil_mode=True), nn.MaxPool2d(2, stride=2, ceil_mode=False)
        self.inorm = nn.InstanceNorm2d(6)

    @staticmethod
    def _conv(sd, k, cin, cout, ks, dil, stride):
        m = nn.Conv2d(cin, cout, ks, stride=stride, padding=dil * (ks // 2), dilation=dil)
        m.load_state_dict({"weight": sd[f"c{k}.weight"], "bias": sd[f"c{k}.bias"]})
        return m

    def forward(self, x):
        r = {}
        r["c1"] = F.relu(self.c1(x))
        r["pc"], r["pf"] = self.pc(r["c1"]), self.pf(r["c1"])
        r["up"] = F.interpolate(r["pc"], size=r["c1"].shape[2:], mode="bilinear", align_corners=False)
        r["cat"] = self.cat(torch.cat((r["up"], r["c1"]), 1))
        r["s7"] = self.s7(x)
        r["n1"] = F.relu(self.inorm(r["s7"]))
        r["s3"], r["s1"] = F.relu(self.s3(r["n1"])), self.s1(r["n1"])
        r["n2"] = self.inorm(r["s1"])
        r["ar"], r["ap"] = F.relu(r["n2"] + r["s3"]), r["n2"] + r["s3"]
        r["rt"] = F.interpolate(r["ap"], size=(9, 4), mode="bilinear", align_corners=True)
        r["sg"] = torch.sigmoid(r["rt"])
        return r


@pytest.fixture(scope="module")
def tiny():
    P, sd, s = _tiny()
    x = torch.from_numpy(synth.normalish("cnmodel/x", (2, 3, 13, 11), 3))
    return P, sd, s, x, P.pack(sd)


def test_float32_model_equals_torch_nn_modules(tiny):
    P, sd, s, x, blob = tiny
    with torch.no_grad():
        got = interpret(P, blob, x)
        want = _Torch(sd).eval()(x)
    assert got[s["pf"]].shape[2:] == (6, 5) and got[s["pc"]].shape[2:] == (7, 6) and got[s["s7"]].shape[2:] == (7, 6)
    for name, slot in s.items():
        g, w = got[slot], want[name]
        assert g.dtype == torch.float32 and g.shape == w.shape, name
        assert torch.equal(g, w), name


def test_float64_model_and_batch(tiny):
    P, sd, s, x, blob = tiny
    with torch.no_grad():
        g32, g64 = interpret(P, blob, x), interpret(P, blob, x, torch.float64)
        one = interpret(P, blob, x[1:], torch.float64)
    for name, slot in s.items():
        assert g64[slot].dtype == torch.float64
        assert float((g32[slot].double() - g64[slot]).abs().max()) < 2e-5 * max(1.0, float(g64[slot].abs().max())), name
        assert torch.allclose(one[slot], g64[slot][1:], rtol=0, atol=1e-12), name       # images are independent
    # InstanceNorm as defined: per image and channel, biased variance, eps 1e-5, no affine
    v = g64[s["s1"]]
    mean = v.mean((2, 3), keepdim=True)
    want = (v - mean) / torch.sqrt(((v - mean) ** 2).mean((2, 3), keepdim=True) + 1e-5)
    assert torch.allclose(g64[s["n2"]], want, rtol=0, atol=1e-12)
    assert float(g64[s["n1"]].min()) == 0.0 and float(g64[s["n2"]].min()) < 0.0       # ReLU on the first, not the second


def test_abs_conv_is_the_sum_of_magnitudes(tiny):
    P, sd, s, x, blob = tiny
    with torch.no_grad():
        g64 = interpret(P, blob, x, torch.float64)
        for op in (0, 4, 5):                  # dilated, two sources, strided 7x7
            o = P.ops[op]
            mag = abs_conv(P, blob, op, g64)
            w, b = sd[f"c{[0, None, None, None, 1, 2][op]}.weight"].double(), sd[f"c{[0, None, None, None, 1, 2][op]}.bias"].double()
            inp = g64[o["a"]] if o["b"] < 0 else torch.cat((g64[o["a"]], g64[o["b"]]), 1)
            ks, st = w.shape[-1], 2 if o["flag"] == 2 else 1
            cols = F.unfold(inp.abs(), ks, dilation=o["dil"], padding=o["dil"] * (ks // 2), stride=st)
            want = (w.abs().reshape(w.shape[0], -1) @ cols + b.abs()[None, :, None]).reshape(mag.shape)
            assert mag.shape == g64[o["dst"]].shape
            assert torch.allclose(mag, want, rtol=1e-13, atol=0)
            raw = F.conv2d(inp, w, b, stride=st, padding=o["dil"] * (ks // 2), dilation=o["dil"])
            assert bool((raw.abs() <= mag * (1 + 1e-12)).all())


# ---------------------------------------------------------------------------------------------------------
# the stored route (host-only: dvd_convnet_create_batched needs no device)
# ---------------------------------------------------------------------------------------------------------
def _expected_route(o, ca, cb, h, w, batch):
    """The dispatch rule of the executor from a conv's shape, written out on its own."""
    ks, cout = o["ks"], o["cout"]
    kp = (ks * ks * (ca + cb) + 15) // 16 * 16
    if o["flag"] == 2:
        return prestage.PATH_STRIDED, 1
    S = 1
    tiles = ((h * w + 127) // 128) * ((cout + 127) // 128)
    if cout > 64 and kp >= 1024 and tiles < 128:
        units = kp // 16
        for c in range(2, units + 1):
            if tiles * c > 256:
                break
            if units % c == 0 and kp // c >= 128:
                S = c
    rows = batch * h * w
    if cout <= 64 and ca % 8 == 0 and cb % 8 == 0 and (ca + cb) % 16 == 0:
        return (prestage.PATH_NARROW1 if cout <= 32 else prestage.PATH_NARROW1X2 if rows < 16384 else prestage.PATH_NARROW2), 1
    if ca % 16 == 0 and cb % 16 == 0 and S == 1 and not (ks == 1 and cb == 0 and o["b"] < 0):
        return prestage.PATH_WIDE, 1
    if ks == 1 and o["b"] < 0 and ca == kp:
        return prestage.PATH_DIRECT, S
    return prestage.PATH_GATHER, S


def _routes(P, hw, batch):
    """[(op index, (path, ksplit), expected)] for every op of program P at input size hw."""
    h = C.c_void_p()
    lib.call("dvd_convnet_create_batched", P.c_ops(), len(P.ops), len(P.ch), P.ch[0], hw[0], hw[1], batch, C.byref(h))
    try:
        out, shp = [], [C.c_int(), C.c_int(), C.c_int()]
        for i, o in enumerate(P.ops):
            path, ks = C.c_int(), C.c_int()
            lib.call("dvd_convnet_op_info", h, i, C.byref(path), C.byref(ks))
            if o["op"] != prestage.CONV:
                out.append((i, (path.value, ks.value), (prestage.PATH_NONE, 1)))
                continue
            lib.call("dvd_convnet_slot_shape", h, o["a"], *[C.byref(v) for v in shp])
            cb = P.ch[o["b"]] if o["b"] >= 0 else 0
            out.append((i, (path.value, ks.value), _expected_route(o, shp[2].value, cb, shp[0].value, shp[1].value, batch)))
        assert lib.raw().dvd_convnet_op_info(h, len(P.ops), C.byref(path), C.byref(ks)) != 0
        assert lib.raw().dvd_convnet_op_info(h, -1, C.byref(path), C.byref(ks)) != 0
        return out
    finally:
        lib.raw().dvd_convnet_destroy(h)


@pytest.mark.parametrize("net,hw,batch", [("u2netp", (70, 50), 1), ("u2netp", (288, 288), 1), ("u2netp", (288, 288), 2),
                                          ("u2netp", (512, 512), 1), ("unet", (96, 96), 1), ("unet", (512, 512), 1),
                                          ("unet", (288, 288), 3), ("fnet", (288, 288), 1), ("fnet", (288, 288), 8),
                                          ("update", (36, 36), 1), ("update", (36, 36), 8)])
def test_stored_route_is_the_dispatch_rule_on_the_product_nets(net, hw, batch):
    build = {"u2netp": prestage.build_u2netp, "unet": prestage.build_unet, "fnet": prestage.build_geotr_fnet,
             "update": prestage.build_geotr_update}[net]
    P, _ = build()
    routes = _routes(P, hw, batch)
    bad = [(i, got, want) for i, got, want in routes if got != want]
    assert not bad, bad[:5]
    assert len({got[0] for _, got, _ in routes}) >= 3


def test_product_nets_cover_these_routes_and_factors():
    """What the product executes (so the op tests' cases are the product's): every route but a split direct 1x1, and the
    split-K factors 3, 4, 6, 9 and 18."""
    paths, factors = set(), set()
    for build, hw in ((prestage.build_u2netp, (512, 512)), (prestage.build_u2netp, (70, 50)), (prestage.build_unet, (288, 288)),
                      (prestage.build_geotr_fnet, (288, 288)), (prestage.build_geotr_update, (36, 36))):
        for _, (path, ks), _ in _routes(build()[0], hw, 1):
            paths.add(path)
            factors.add(ks)
            assert ks == 1 or path == prestage.PATH_GATHER
    assert paths == set(range(8)), paths
    assert {3, 4, 6, 9, 18} <= factors, factors
