"""GPU tests of the conv-net executor (dvd_amd/csrc/convnet.hip) op by op against the float64 model of the op list
(tests/convnet_model.py), on every route a convolution can take.

Each conv case is a one-op net (two-source cases: plus exact channel-selection 1x1 convs that make the sources), run
once with a batch of 3 and once per image, and is checked four ways:
  * exact probe: small-integer inputs, weights and bias - every partial sum is an integer below 2^24, so f32 arithmetic
    is exact in any order (split-K included) and the result must EQUAL the float64 model;
  * real-valued data: per element |got - ref64| <= 1.01 * (ks^2 cin + 2) * 2^-24 * abs_conv, the forward bound of an f32
    dot product of ks^2 cin terms in any summation order plus the bias add (ReLU is 1-Lipschitz);
  * batch invariance: an image gives the same bits alone and in the batch of 3;
  * workspace canary (gather, strided, split-K): a pattern behind the workspace the library asked for stays untouched.
Every case asserts the route (dvd_convnet_op_info) it was written for.
"""
import ctypes as C
from collections import namedtuple

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from convnet_model import abs_conv, add_conv, interpret
from dvd_amd import lib, prestage, synth
from dvd_amd.prestage import (PATH_DIRECT, PATH_GATHER, PATH_NARROW1, PATH_NARROW1X2, PATH_NARROW2, PATH_STRIDED,
                              PATH_WIDE)

pytestmark = pytest.mark.gpu

ROUTE_NAMES = {PATH_NARROW1: "narrow<1>x1", PATH_NARROW1X2: "narrow<1>x2", PATH_NARROW2: "narrow<2>", PATH_WIDE: "wide",
               PATH_DIRECT: "direct", PATH_GATHER: "gather", PATH_STRIDED: "strided"}
TAIL = 4096              # canary bytes behind the workspace
BATCH = 3


# ---------------------------------------------------------------------------------------------------------
# data
# ---------------------------------------------------------------------------------------------------------
def _ints(key, shape, lo, hi):
    """integers in [lo, hi] as f32"""
    u = synth.uniform01("cnops/" + key, int(np.prod(shape)), 7).astype(np.float64)
    return torch.from_numpy((np.floor(u * (hi - lo + 1)) + lo).astype(np.float32).reshape(shape))


def _fill_int(name, shape):
    return _ints(name, shape, -8, 8) if len(shape) == 1 else _ints(name, shape, -2, 2)


def _fill_real(name, shape):
    if len(shape) == 1:
        return torch.from_numpy(synth.uniform("cnops/" + name, shape, -0.5, 0.5, 7))
    return torch.from_numpy(synth.synth_tensor("cnops/" + name, shape, "w", 7))


def _select(P, sd, src, idx):
    """A slot holding channels `idx` of slot `src`: a 1x1 conv with one unit weight per output and no bias - one product
    by 1.0 plus zeros, exact in f32 on any route and for any data."""
    cout = len(idx)

    def fill(name, shape):
        t = torch.zeros(shape)
        if len(shape) == 4:
            t[torch.arange(cout), torch.tensor(idx), 0, 0] = 1.0
        return t
    return add_conv(P, sd, src, cout, fill, 1, 1, False)


# ---------------------------------------------------------------------------------------------------------
# running a program on the executor
# ---------------------------------------------------------------------------------------------------------
def _executor(P, outs, hw, batch, sd, canary=False):
    net = prestage.ConvNet(P, outs, hw, batch=batch)
    net.load_state_dict(sd)
    tail = None
    if canary:
        # a workspace of our own: exactly the bytes the library asks for, then a patterned tail it must never touch
        nbytes = lib.raw().dvd_convnet_workspace_bytes(net._h)
        buf = torch.full((nbytes + 256 + TAIL,), 0xA5, dtype=torch.uint8, device="cuda")
        lead = (-buf.data_ptr()) % 256
        net.workspace, net._ws, net._ws_bytes = buf, buf.data_ptr() + lead, nbytes
        tail = buf[lead + nbytes:lead + nbytes + TAIL]
    return net, tail


def _run(net, x):
    outs = net.run(x.cuda().contiguous())
    torch.cuda.synchronize()
    return [o.cpu() for o in outs]


def _tail_ok(tail):
    return tail is None or bool((tail == 0xA5).all())


# ---------------------------------------------------------------------------------------------------------
# conv cases
# ---------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "srcs cout ks dil hw route S stride relu route3 canary")


def _c(srcs, cout, ks, dil, hw, route, S=1, stride=1, relu=True, route3=None, canary=None):
    if not isinstance(srcs, tuple):
        srcs = (srcs,)
    if canary is None:
        canary = route in (PATH_GATHER, PATH_STRIDED) or S > 1
    return Case(srcs, cout, ks, dil, hw, route, S, stride, relu, route if route3 is None else route3, canary)


N1, N1X2, N2, WIDE, GATHER, DIRECT, STRIDED = (PATH_NARROW1, PATH_NARROW1X2, PATH_NARROW2, PATH_WIDE, PATH_GATHER, PATH_DIRECT,
                                               PATH_STRIDED)
CASES = [
    # narrow implicit kernel, one column group: cout 1 / 2 / 16 / 32; K-chunk counts nch = ks^2 cin / 16 of 1, 2, 3 (below
    # the prefetch depth), 9, 18, 27, 36 and 49 (every tail of the 4-unrolled loop); dilation 1 .. 8 on 3x2 (every tap but
    # the centre outside at dilation 8), 9x9 and 17x5; 6, 35 (x 3 images: waves straddle images) and 117 rows
    _c(16, 1, 1, 1, (3, 2), N1), _c(32, 2, 1, 1, (9, 9), N1, relu=False), _c(48, 16, 1, 1, (17, 5), N1),
    _c(16, 32, 3, 1, (9, 13), N1), _c(32, 16, 3, 2, (9, 9), N1, relu=False), _c(48, 2, 3, 4, (17, 5), N1),
    _c(64, 32, 3, 8, (9, 9), N1), _c(16, 16, 3, 8, (3, 2), N1, relu=False), _c(16, 1, 3, 2, (3, 2), N1),
    _c(64, 16, 3, 4, (17, 5), N1), _c(16, 16, 3, 1, (5, 7), N1), _c(32, 32, 3, 4, (3, 2), N1, relu=False),
    _c(16, 16, 7, 1, (9, 9), N1), _c(16, 32, 7, 2, (17, 5), N1, relu=False), _c(16, 2, 7, 8, (3, 2), N1),
    _c((8, 8), 16, 3, 1, (9, 9), N1), _c((24, 8), 32, 3, 2, (17, 5), N1, relu=False), _c((8, 24), 2, 3, 4, (9, 9), N1),
    _c((16, 48), 16, 3, 1, (5, 7), N1), _c((8, 8), 1, 1, 1, (3, 2), N1, relu=False), _c((24, 8), 16, 7, 1, (9, 9), N1),
    _c(16, 2, 3, 1, (3, 2), N1), _c(16, 16, 3, 8, (17, 5), N1, relu=False), _c(32, 1, 3, 1, (17, 5), N1),
    _c(48, 32, 3, 2, (9, 9), N1), _c(64, 2, 3, 4, (9, 9), N1, relu=False), _c((8, 24), 32, 3, 8, (17, 5), N1),
    # narrow, two column groups
    _c(16, 33, 3, 1, (9, 13), N1X2), _c(16, 48, 3, 2, (9, 13), N1X2, relu=False), _c(16, 64, 3, 1, (9, 13), N1X2),
    _c((8, 24), 48, 3, 2, (9, 13), N1X2), _c(32, 64, 1, 1, (9, 13), N1X2, relu=False), _c(16, 33, 7, 1, (9, 13), N1X2),
    # <1> versus <2>: 16383 rows, 16384 rows, and a ragged last workgroup (the batch of 3 is past the threshold throughout)
    _c(16, 33, 3, 1, (127, 129), N1X2, route3=N2), _c(16, 64, 3, 1, (127, 129), N1X2, route3=N2, relu=False),
    _c(16, 33, 3, 1, (128, 128), N2, relu=False), _c(16, 64, 3, 1, (128, 128), N2),
    _c(16, 33, 3, 1, (130, 127), N2), _c(16, 64, 3, 1, (130, 127), N2, relu=False),
    # wide implicit GEMM: cout 65 and 130 take the scalar epilogue; one and two sources; 1x1 over two sources; 7x7
    _c(16, 65, 3, 1, (5, 7), WIDE), _c(96, 72, 3, 2, (12, 11), WIDE, relu=False), _c((16, 16), 128, 3, 1, (12, 11), WIDE),
    _c((16, 32), 130, 3, 2, (5, 7), WIDE, relu=False), _c((16, 16), 72, 1, 1, (5, 7), WIDE), _c((16, 32), 65, 1, 1, (12, 11), WIDE),
    _c(16, 72, 7, 1, (12, 11), WIDE, relu=False), _c(16, 130, 7, 2, (5, 7), WIDE), _c(96, 128, 3, 1, (5, 7), WIDE),
    _c(128, 72, 3, 1, (128, 128), WIDE),                  # kp 1152 >= 1024 but 128 tiles: no split-K
    # gather + GEMM: K padded 27 -> 32 and 147 -> 160; unaligned sources
    _c(3, 1, 3, 1, (9, 9), GATHER), _c(3, 4, 7, 1, (17, 5), GATHER, relu=False), _c((1, 1), 2, 3, 1, (5, 7), GATHER),
    _c((5, 1), 3, 3, 2, (9, 9), GATHER, relu=False), _c((3, 4), 5, 3, 1, (9, 13), GATHER), _c((3, 4), 6, 1, 1, (3, 2), GATHER),
    _c(8, 72, 3, 1, (12, 11), GATHER, relu=False), _c(3, 64, 3, 4, (9, 9), GATHER),
    # direct 1x1 read
    _c(16, 72, 1, 1, (5, 7), DIRECT), _c(64, 72, 1, 1, (12, 11), DIRECT, relu=False), _c(256, 72, 1, 1, (9, 9), DIRECT),
    # split-K with the product's factors on small maps; the direct 1x1 read with split-K
    _c(128, 128, 3, 1, (9, 9), GATHER, S=9), _c(512, 512, 3, 1, (18, 18), GATHER, S=18, relu=False),
    _c((64, 64), 128, 3, 1, (9, 9), GATHER, S=9, relu=False), _c((120, 8), 128, 3, 1, (9, 9), GATHER, S=9),
    _c(1024, 72, 1, 1, (5, 7), DIRECT, S=8),
    # stride 2: 7x7, 3x3, 1x1; a 2x2 input gives one output pixel; one dilated case
    _c(3, 24, 7, 1, (50, 46), STRIDED, stride=2), _c(24, 32, 3, 1, (7, 7), STRIDED, stride=2, relu=False),
    _c(24, 32, 1, 1, (8, 5), STRIDED, stride=2), _c(64, 72, 3, 1, (2, 2), STRIDED, stride=2, relu=False),
    _c(3, 5, 7, 1, (2, 2), STRIDED, stride=2), _c(64, 16, 3, 2, (8, 5), STRIDED, stride=2),
    _c(3, 8, 1, 1, (7, 7), STRIDED, stride=2, relu=False), _c(64, 130, 1, 1, (2, 2), STRIDED, stride=2),
]


def _case_id(c):
    src = "+".join(str(s) for s in c.srcs)
    return (f"{ROUTE_NAMES[c.route].replace('<', '').replace('>', '')}-c{src}-o{c.cout}-k{c.ks}d{c.dil}s{c.stride}"
            f"-{c.hw[0]}x{c.hw[1]}" + (f"-S{c.S}" if c.S > 1 else ""))


def _build(c, fill):
    """(program, state dict, op index of the conv under test, its slot, input channels)"""
    P, sd = prestage.Program(max(c.srcs)), {}
    c0 = P.ch[0]
    if len(c.srcs) == 1:
        a, b = 0, -1
    else:
        ca, cb = c.srcs
        # two sources with different content: a = the input (or a stride of its channels), b = its channels reversed
        a = 0 if ca == c0 else _select(P, sd, 0, [(2 * j + 1) % c0 for j in range(ca)])
        b = _select(P, sd, 0, [c0 - 1 - j for j in range(cb)])
    dst = add_conv(P, sd, a, c.cout, fill, c.ks, c.dil, c.relu, b, c.stride)
    return P, sd, len(P.ops) - 1, dst, c0


def _bound(c):
    return 1.01 * (c.ks * c.ks * sum(c.srcs) + 2) * 2.0 ** -24


@pytest.mark.parametrize("c", CASES, ids=_case_id)
def test_conv(c):
    # ---- exact probe -------------------------------------------------------------------------------------
    P, sd, op, dst, c0 = _build(c, _fill_int)
    x = _ints(f"x/{_case_id(c)}", (BATCH, c0, *c.hw), -4, 4)
    net3, tail3 = _executor(P, [dst], c.hw, BATCH, sd, c.canary)
    assert net3.op_info(op) == (c.route3, c.S), (net3.op_info(op), ROUTE_NAMES[c.route3], c.S)
    got = _run(net3, x)[0]
    assert _tail_ok(tail3), "the executor wrote behind the workspace it asked for"
    blob = P.pack(sd)
    with torch.no_grad():
        want = interpret(P, blob, x, torch.float64)[dst]
    assert float(want.abs().max()) < 2 ** 24 and got.shape == want.shape
    assert torch.equal(got, want.float()), f"exact probe: {int((got != want.float()).sum())} of {got.numel()} elements differ"
    # ---- real-valued data, batch of 3 and each image alone ----------------------------------------------
    P, sd, op, dst, c0 = _build(c, _fill_real)
    key, shape = f"cnops/xr/{_case_id(c)}", (BATCH, c0, *c.hw)
    x = torch.from_numpy(synth.uniform(key, shape, -1, 1, 7) if c.ks == 1 else synth.normalish(key, shape, 7))
    net3, tail3 = _executor(P, [dst], c.hw, BATCH, sd, c.canary)
    net1, tail1 = _executor(P, [dst], c.hw, 1, sd, c.canary)
    assert net3.op_info(op) == (c.route3, c.S) and net1.op_info(op) == (c.route, c.S), (net1.op_info(op), net3.op_info(op))
    got = _run(net3, x)[0]
    alone = [_run(net1, x[i:i + 1])[0] for i in range(BATCH)]
    assert _tail_ok(tail3) and _tail_ok(tail1), "the executor wrote behind the workspace it asked for"
    blob = P.pack(sd)
    with torch.no_grad():
        slots = interpret(P, blob, x, torch.float64)
        mag = abs_conv(P, blob, op, slots)
    want = slots[dst]
    err, bound = (got.double() - want).abs(), _bound(c) * mag
    ratio = float((err / bound).max())
    print(f"conv {_case_id(c)}: route {ROUTE_NAMES[c.route]} S {c.S}: max err/bound {ratio:.3e} (max err {float(err.max()):.2e})")
    assert bool((err <= bound).all()), ratio
    for i in range(BATCH):
        assert torch.equal(alone[i][0], got[i]), f"image {i} differs between a batch of 1 and a batch of {BATCH}"


# ---------------------------------------------------------------------------------------------------------
# the other ops, on batched nets
# ---------------------------------------------------------------------------------------------------------
def _one_op(c, hw, emit, x):
    """Run the program `emit(P) -> slot` over x [N, c, *hw] -> its output on the host."""
    P = prestage.Program(c)
    dst = emit(P)
    net = prestage.ConvNet(P, [dst], hw, batch=x.shape[0])
    net.weights = torch.zeros(4, device="cuda")       # no conv: an empty blob (the library still wants a pointer)
    return _run(net, x)[0]


@pytest.mark.parametrize("hw,ceil", [((7, 5), True), ((1, 4), True), ((2, 2), True), ((7, 5), False), ((8, 6), False)])
@pytest.mark.parametrize("c", [3, 64])
def test_pool(hw, ceil, c):
    x = torch.from_numpy(synth.normalish(f"cnops/pool/{hw}/{c}", (BATCH, c, *hw), 7))
    got = _one_op(c, hw, lambda P: P.pool(0, ceil), x)
    assert torch.equal(got, F.max_pool2d(x, 2, stride=2, ceil_mode=ceil))


@pytest.mark.parametrize("relu", [False, True])
def test_add(relu):
    c, hw = 24, (9, 13)
    x = torch.from_numpy(synth.normalish("cnops/add", (BATCH, c, *hw), 7))
    P, sd = prestage.Program(c), {}
    rev = _select(P, sd, 0, [c - 1 - j for j in range(c)])
    dst = P.add(0, rev, relu=relu)
    net, _ = _executor(P, [rev, dst], hw, BATCH, sd)
    got_rev, got = _run(net, x)
    assert torch.equal(got_rev, x.flip(1))
    want = x + x.flip(1)
    assert torch.equal(got, torch.relu(want) if relu else want)
    assert relu or float(got.min()) < 0


@pytest.mark.parametrize("src,dst", [((2, 3), (9, 9)), ((18, 18), (35, 25)), ((9, 9), (9, 9)), ((7, 5), (1, 1)), ((1, 1), (4, 6))])
@pytest.mark.parametrize("align", [False, True])
def test_resize(src, dst, align):
    for c in (1, 16, 64):
        x = torch.from_numpy(synth.uniform(f"cnops/resize/{src}/{c}", (BATCH, c, *src), -1, 1, 7))
        got = _one_op(c, src, lambda P: P.resize_to(0, dst[0], dst[1], align), x)
        want = F.interpolate(x, size=dst, mode="bilinear", align_corners=align)
        err = float((got - want).abs().max())
        print(f"resize {src} -> {dst} align {align} c {c}: max abs {err:.2e}")
        assert got.shape == want.shape and err <= 2e-6, err
    # to another slot's size: the same kernel through resize_like
    if dst == (9, 9) and src == (9, 9):
        x = torch.from_numpy(synth.uniform("cnops/resize/like", (BATCH, 16, 9, 9), -1, 1, 7))
        got = _one_op(16, (9, 9), lambda P: P.resize_like(P.pool(0, True), 0, align), x)
        want = F.interpolate(F.max_pool2d(x, 2, stride=2, ceil_mode=True), size=(9, 9), mode="bilinear", align_corners=align)
        assert float((got - want).abs().max()) <= 2e-6


def test_sigmoid():
    c, hw = 16, (25, 23)
    x = torch.from_numpy(synth.uniform("cnops/sigmoid", (BATCH, c, *hw), -30, 30, 7))
    x[0, 0, 0, :8] = torch.tensor([0.0, -0.0, 30.0, -30.0, 1e-30, -1e-30, 88.0, -88.0])
    x[1, 3, 2, :4] = torch.tensor([100.0, -100.0, 1e30, -1e30])
    got = _one_op(c, hw, lambda P: P.sigmoid(0), x).double()
    want = torch.sigmoid(x.double())
    inside = x.abs() <= 30
    rel = float(((got - want).abs() / want)[inside].max())
    print(f"sigmoid: max relative error {rel * 2 ** 23:.2f} x 2^-23 for |x| <= 30")
    assert rel <= 2.0 ** -22, rel
    assert bool(torch.isfinite(got).all())
    big = got[1, 3, 2, :4]
    assert abs(float(big[0]) - 1) <= 1e-37 and abs(float(big[1])) <= 1e-37 and abs(float(big[2]) - 1) <= 1e-37 \
        and abs(float(big[3])) <= 1e-37, big
    assert float(got[0, 0, 0, 0]) == 0.5 and float(got[0, 0, 0, 1]) == 0.5


@pytest.mark.parametrize("hw", [(1, 1), (1, 5), (4, 4), (1, 17), (25, 23)])
@pytest.mark.parametrize("relu", [False, True])
def test_instnorm(hw, relu):
    worst = 0.0
    for c in (1, 24, 64, 65, 192):
        x = torch.from_numpy(synth.normalish(f"cnops/in/{hw}/{c}", (BATCH, c, *hw), 7)) * 1.5 + 0.25
        # a constant channel: 0.5 sums exactly (multiples of 0.5 up to 288) and (hw * 0.5) / hw is 0.5, so x - mean is 0
        x[1, c - 1] = 0.5
        got = _one_op(c, hw, lambda P: P.instnorm(0, relu), x).double()
        xd = x.double()
        mean = xd.mean((2, 3), keepdim=True)
        want = (xd - mean) / torch.sqrt(((xd - mean) ** 2).mean((2, 3), keepdim=True) + 1e-5)
        want = torch.relu(want) if relu else want
        assert bool((got[1, c - 1] == 0).all()), "a constant channel must give exactly 0"
        if hw == (1, 1):
            assert bool((got == 0).all())
            continue
        err = float((got - want).abs().max() / want.abs().max())
        worst = max(worst, err)
        assert err <= 2e-6, (c, err)
    print(f"instnorm {hw} relu {relu}: max abs / max |want| {worst:.2e}")


def test_instnorm_offset_needs_two_passes():
    """64 + k / 256 with integer |k| <= 512 at hw = 256: every f32 partial sum and the mean are exact, the variance is ~1.3 on
    a mean of 64 - E[x^2] - E[x]^2 in f32 would lose it (4096 +- 2^-11 against 1.3); the centred second pass does not."""
    c, hw = 24, (16, 16)
    k = _ints("in/offset", (BATCH, c, *hw), -512, 512)
    x = 64.0 + k / 256.0
    got = _one_op(c, hw, lambda P: P.instnorm(0, False), x).double()
    xd = x.double()
    mean = xd.mean((2, 3), keepdim=True)
    want = (xd - mean) / torch.sqrt(((xd - mean) ** 2).mean((2, 3), keepdim=True) + 1e-5)
    err = float((got - want).abs().max() / want.abs().max())
    print(f"instnorm with offset 64: max abs / max |want| {err:.2e}")
    assert err <= 2e-6, err


# ---------------------------------------------------------------------------------------------------------
# refusals (host-only)
# ---------------------------------------------------------------------------------------------------------
def _create(P, hw, n_slots=None):
    h = C.c_void_p()
    rc = lib.raw().dvd_convnet_create(P.c_ops(), len(P.ops), n_slots or len(P.ch), P.ch[0], hw[0], hw[1], C.byref(h))
    msg = lib.raw().dvd_last_error().decode()
    if rc == 0:
        lib.raw().dvd_convnet_destroy(h)
    return rc, msg


def _plain(k):
    return ("plain", f"c{k}.weight", f"c{k}.bias")


def _bad_ks5(P):
    P.conv(0, 4, _plain(0), 5)


def _bad_dil0(P):
    P.conv(0, 4, _plain(0), 3, 0)


def _bad_stride2_two_sources(P):
    P.conv(0, 4, _plain(1), 3, 1, 2, P.conv(0, 16, _plain(0), 3), stride=2)


def _bad_add(P):
    P.add(0, P.pool(0, True))


def _bad_floor_pool(P):
    P.pool(0, False)


def _bad_twice(P):
    d = P.sigmoid(0)
    P.sigmoid(0)
    P.ops[1]["dst"] = d


def _bad_undefined(P):
    P.sigmoid(0)
    P.sigmoid(0)
    P.ops[0]["a"] = 2            # slot 2 is written by the NEXT op


def _bad_w_off(P):
    P.conv(P.conv(0, 4, _plain(0), 3), 4, _plain(1), 3)
    P.ops[1]["w_off"] += 4


@pytest.mark.parametrize("emit,hw,words", [
    (_bad_ks5, (9, 9), "conv parameters"), (_bad_dil0, (9, 9), "conv parameters"),
    (_bad_stride2_two_sources, (9, 9), "stride"), (_bad_add, (9, 9), "differ in shape"), (_bad_floor_pool, (1, 1), "1-pixel"),
    (_bad_twice, (9, 9), "destination"), (_bad_undefined, (9, 9), "not defined"), (_bad_w_off, (9, 9), "w_off")],
    ids=lambda v: v.__name__[5:] if callable(v) else None)
def test_create_refuses(emit, hw, words):
    P = prestage.Program(16)
    emit(P)
    rc, msg = _create(P, hw)
    assert rc != 0 and msg.startswith("convnet_create: op") and words in msg, (rc, msg)
    # the same list without the fault is accepted (the refusal is about the fault, not about the list)
    Q = prestage.Program(16)
    Q.conv(Q.pool(Q.sigmoid(0), True), 4, _plain(0), 3)
    assert _create(Q, (9, 9))[0] == 0
