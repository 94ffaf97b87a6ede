"""Every token-side launch of the engine (tests/token_callsites.py), with the engine's own arguments and sizes, against a
plain float64 restatement of the operation.

Each record is launched through lib.call with the table's raw arguments on 0xFF-filled allocations (NaN as f16 and as f32)
that end in a 256-byte guard, and the WHOLE of every buffer is compared afterwards, byte for byte: what the launch must write
against the reference, every other byte against its value before the launch (gap columns of a strided output, neighbouring column slices
of z, inputs, guards).  Exact pass: inputs that make the result exactly representable, compared bit for bit.  Random pass:
the engine's magnitudes against float64 under a bound DERIVED from the arithmetic (below), never from the kernel's output.

Error model (u = 2^-24, the unit roundoff of f32; one ulp of an f32 value v is at most 2^-23 |v|):
  * a chain of n f32 roundings over terms t_i deviates by at most n u sum|t_i| (standard forward bound, first order);
  * an f16 store is correctly rounded: 2^-11 |y| in the normal range, 2^-25 below 2^-14;
  * rsqrtf, expf, sinf, cosf: the HIP math API documents 1 ulp for each on AMD GPUs; the allowance here is 2 ulps;
  * where an argument is itself a rounded f32 expression, its error times the function's Lipschitz constant is added.
"""
import dataclasses
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from dvd_amd import lib

import token_callsites as TS
from dither_ref import dither_ref

pytestmark = pytest.mark.gpu

U = 2.0 ** -24            # unit roundoff of f32
ULP = 2.0 ** -23          # one f32 ulp, relative
H_REL, H_SUB = 2.0 ** -11, 2.0 ** -25          # half an f16 ulp: relative (normal range) and absolute (subnormal range)
RSQ_ULPS = EXP_ULPS = TRIG_ULPS = 2            # documented 1 ulp each, 2x margin
DT = {2: torch.float16, 4: torch.float32}
GUARD = 256


class Bufs:
    """One device allocation per buffer of the record, 0xFF-filled, with a guard behind the last byte the launch may touch."""

    def __init__(self, c):
        size = {}
        for p, n in c.extents().items():
            buf, off = c.args[p]
            size[buf] = max(size.get(buf, 0), off + n * TS.POINTERS[c.kernel][p])
        self.raw = {b: torch.full((-(-n // 256) * 256 + GUARD,), 255, dtype=torch.uint8, device="cuda") for b, n in size.items()}
        self.c = c

    def flat(self, p, raw=None):
        """Typed flat view from pointer parameter `p` to the end of its extent."""
        buf, off = self.c.args[p]
        esz = TS.POINTERS[self.c.kernel][p]
        return (raw or self.raw)[buf][off:off + self.c.extents()[p] * esz].view(DT[esz])

    def addr(self, ptr):
        return self.raw[ptr[0]].data_ptr() + ptr[1]

    def snapshot(self):
        return {b: t.clone() for b, t in self.raw.items()}


def _sv(flat, shape, strides):
    return torch.as_strided(flat, shape, strides, flat.storage_offset())


def written(c, bufs, raw=None):
    """{pointer parameter: strided view of exactly the elements the launch must write}."""
    a, k = c.args, c.kernel
    f = lambda p: bufs.flat(p, raw)                        # noqa: E731
    T = (a["g"] // 2) ** 2 if "g" in a else 0
    if k == "layernorm_rows":
        return {"out16": _sv(f("out16"), (a["batch"], a["rows"], a["c"]), (a["stride_out"], a["ldout"], 1))}
    if k == "small_linear":
        return {"y": _sv(f("y"), (a["m"], a["n"]), (a["ldy"], 1))}
    if k == "patch_rows":
        return {"out": _sv(f("out"), (a["n"] * T, 4 * a["c"]), (a["ldo"], 1))}
    if k == "build_r_rows":
        return {"out16": _sv(f("out16"), (a["n"] * T, a["ldo"]), (a["ldo"], 1))}
    if k == "colmean":
        return {"partial": f("partial"), "pooled": f("pooled")}
    if k == "final_tokens":
        return {p: f(p) for p in ("x0", "tok8") if a[p] is not None}
    if k == "embed_obs_ln":
        return {"tok32": f("tok32"), "ln16": f("ln16")}
    out = {"posenc_add": "z", "dwconv3x3": "out16"}.get(k, "out")
    return {out: f(out)}


def launch(c, bufs):
    lib.call("dvd_" + c.kernel, *TS.c_args(c, bufs.addr), lib.stream_ptr())
    torch.cuda.synchronize()


def run(c, bufs, expect=None):
    """Launch `c`; compare every buffer in full.  expect: {pointer: exact expected tensor} (exact pass), or None: the written
    elements are returned for a numeric comparison and only have to be finite here.  Returns the written views."""
    want = bufs.snapshot()
    launch(c, bufs)
    got, wv = written(c, bufs), written(c, bufs, want)
    for p, v in got.items():
        wv[p].copy_(v if expect is None else expect[p].reshape(v.shape).to(v.dtype))
        if expect is None:
            assert bool(torch.isfinite(v).all()), f"{c.site} {p}: non-finite output"
    for b, r in bufs.raw.items():                      # bytes, not values: -0 is not +0, a NaN is not the 0xFF fill
        if not torch.equal(r, want[b]):
            bad = (r != want[b]).nonzero()
            raise AssertionError(f"{c.site} buffer {b}: {bad.numel()} bytes differ from the expected buffer (written "
                                 f"elements, inputs, or bytes that must stay untouched), first at byte {int(bad[0])}")
    return got


def close(c, what, got, ref, bound):
    err = (got.double() - ref).abs()
    worst = float((err - bound).max())
    print(f"{c.site} {what}: max err {float(err.max()):.3e}, max err / bound {float((err / (bound + 1e-300)).max()):.3f}")
    assert worst <= 0, f"{c.site} {what}: error exceeds the derived bound by {worst:.3e} (max err {float(err.max()):.3e})"


def f16_bound(y, dy):
    """Bound of f16(y_kernel) against y: the f32 error dy plus half an f16 ulp of the value that is rounded."""
    return dy + H_REL * (y.abs() + dy) + H_SUB


def ints(t, lo, hi, gen):
    t.copy_(torch.randint(lo, hi + 1, t.shape, generator=gen, device="cuda").to(t.dtype))


def rnd(t, scale, gen, shift=0.0):
    t.copy_((torch.randn(t.shape, generator=gen, device="cuda") * scale + shift).to(t.dtype))


def tern(t, density, gen):
    v = torch.randint(-1, 2, t.shape, generator=gen, device="cuda").float()
    t.copy_((v * (torch.rand(t.shape, generator=gen, device="cuda") < density)).to(t.dtype))


# ------------------------------------------------------------------------------------------------------------------
# LayerNorm: float64 value and error bound of the f32 evaluation  y0 = (x - mean) * rsqrtf(var + eps)
# ------------------------------------------------------------------------------------------------------------------
def ln_ref(x, dx, eps):
    """x [R, C] float64, dx: bound of the error already in the kernel's copy of x (0, or [R, C]).
    A row sum is C/64 sequential adds per lane and a 6-level tree over the 64 lanes: ns = C/64 + 6 roundings.
      mean  = sum * (1/C)            : ns adds, the rounded constant and the product -> (ns + 2) u mean|x|, plus mean(dx)
      d     = x - mean               : dd = dx + dmean + u |d|
      var   = sum(d^2) * (1/C)       : |d^2 error| <= 2 |d| dd + dd^2; square, ns adds, constant, product -> (ns + 4) u var
      rstd  = rsqrtf(var + eps)      : add u; d rstd / rstd = dvar / (2 (var + eps)); RSQ_ULPS ulps of the function value
      y0    = d * rstd               : dd rstd + |y0| (drstd/rstd + u)"""
    C = x.shape[-1]
    ns = C // 64 + 6
    mean = x.mean(-1, keepdim=True)
    d = x - mean
    var = (d * d).mean(-1, keepdim=True)
    rstd = (var + eps).rsqrt()
    y0 = d * rstd
    dxm = dx.mean(-1, keepdim=True) if torch.is_tensor(dx) else dx
    dmean = dxm + (ns + 2) * U * x.abs().mean(-1, keepdim=True)
    dd = dx + dmean + U * d.abs()
    dvar = (2 * d.abs() * dd + dd * dd).mean(-1, keepdim=True) + (ns + 4) * U * var
    drel = 0.5 * dvar / (var + eps) + U + RSQ_ULPS * ULP
    return y0, dd * rstd + y0.abs() * (drel + U)


def case_layernorm_rows(c, gen):
    a = c.args
    bufs = Bufs(c)
    C, rows = a["c"], a["rows"]
    # rows of every kind the mean subtraction and eps have to cope with: N(0, 1) times a per-row scale drawn log-uniformly
    # from 0.01 to 2 (variance from 1e-4, where eps = 1e-6 is 1 % of it, to 4) plus a per-row offset of order 0.5
    zin = bufs.flat("in")
    rnd(zin, 1.0, gen)
    for b in range(a["batch"]):
        v = _sv(zin[b * a["stride_in"]:], (rows, C), (a["ldin"], 1))
        scale = torch.exp(torch.rand((rows, 1), generator=gen, device="cuda") * math.log(200.0) + math.log(0.01))
        v.mul_(scale).add_(torch.randn((rows, 1), generator=gen, device="cuda") * 0.5)
    for p, s, m in (("gamma", 0.2, 1.0), ("beta", 0.2, 0.0), ("shift", 0.3, 0.0), ("scale", 0.3, 0.0)):
        if a[p] is not None:
            rnd(bufs.flat(p), s, gen, m)
    got = run(c, bufs)["out16"]
    nmod = (rows - 1) // a["mod_rows"] + 1
    for b in range(a["batch"]):
        x = _sv(zin[b * a["stride_in"]:], (rows, C), (a["ldin"], 1)).double()
        y, dy = ln_ref(x, 0.0, a["eps"])
        if a["gamma"] is not None:                       # y * g + b: product and sum
            g, bt = bufs.flat("gamma").double(), bufs.flat("beta").double()
            dy = dy * g.abs() + 2 * U * ((y * g).abs() + bt.abs())
            y = y * g + bt
        if a["shift"] is not None:                       # y * (1 + scale) + shift: sum, product and sum
            ridx = torch.arange(rows, device="cuda") // a["mod_rows"]
            sc = _sv(bufs.flat("scale"), (nmod, C), (a["ldmod"], 1)).double()[ridx]
            sh = _sv(bufs.flat("shift"), (nmod, C), (a["ldmod"], 1)).double()[ridx]
            dy = dy * (1 + sc).abs() + 3 * U * ((y * (1 + sc)).abs() + sh.abs())
            y = y * (1 + sc) + sh
        close(c, f"slice {b}", got[b], y, f16_bound(y, dy))


def case_embed_obs_ln(c, gen):
    a = c.args
    n, g = a["n"], a["g"]
    side = g // 2
    T = side * side
    bufs = Bufs(c)
    rnd(bufs.flat("x"), 1.0, gen)
    rnd(bufs.flat("w"), 0.3, gen)
    rnd(bufs.flat("bias"), 0.1, gen)
    rnd(bufs.flat("pos"), 0.5, gen)
    got = run(c, bufs)
    x = bufs.flat("x").double().reshape(n, 2, side, 2, side, 2)
    patches = x.permute(0, 2, 4, 1, 3, 5).reshape(n * T, 8)                      # conv weight order c, p, q
    w, b = bufs.flat("w").double().reshape(384, 8), bufs.flat("bias").double()
    pos = bufs.flat("pos").double().reshape(T, 384).repeat(n, 1)
    tok = patches @ w.T + b + pos
    # bias + 8 products + pos: 8 products and 9 adds on one accumulator
    dtok = 17 * U * (patches.abs() @ w.abs().T + b.abs() + pos.abs())
    close(c, "tok32", got["tok32"].reshape(n * T, 384), tok, dtok)
    # the LayerNorm reads the f32 tokens the kernel stored (checked above): reference = float64 LN of those values
    y, dy = ln_ref(got["tok32"].reshape(n * T, 384).double(), 0.0, 1e-6)
    close(c, "ln16", got["ln16"].reshape(n * T, 384), y, f16_bound(y, dy))


def case_final_tokens(c, gen):
    a = c.args
    n, g = a["n"], a["g"]
    side = g // 2
    T = side * side
    C = 1536
    bufs = Bufs(c)
    rnd(bufs.flat("z"), 1.5, gen)
    rnd(bufs.flat("gamma"), 0.2, gen, 1.0)
    rnd(bufs.flat("beta"), 0.1, gen)
    rnd(bufs.flat("shift"), 0.3, gen)
    rnd(bufs.flat("scale"), 0.3, gen)
    rnd(bufs.flat("w8"), 0.03, gen)
    rnd(bufs.flat("b8"), 0.1, gen)
    rnd(bufs.flat("init_flow"), 0.3, gen)
    got = run(c, bufs)
    gm, bt = bufs.flat("gamma").double(), bufs.flat("beta").double()
    w, b8 = bufs.flat("w8").double().reshape(8, C), bufs.flat("b8").double()
    nmod = (n * T - 1) // a["mod_rows"] + 1
    shm = _sv(bufs.flat("shift"), (nmod, C), (a["ldmod"], 1)).double()
    scm = _sv(bufs.flat("scale"), (nmod, C), (a["ldmod"], 1)).double()
    o, do = [], []
    for r0 in range(0, n * T, 8192):
        z = bufs.flat("z").reshape(n * T, C)[r0:r0 + 8192].double()
        ridx = torch.arange(r0, r0 + z.shape[0], device="cuda") // a["mod_rows"]
        y0, dy0 = ln_ref(z, 0.0, 1e-5)
        v1 = y0 * gm + bt                                   # product and sum
        dv1 = dy0 * gm.abs() + 2 * U * ((y0 * gm).abs() + bt.abs())
        y1, dy1 = ln_ref(v1, dv1, 1e-6)
        sc, sh = scm[ridx], shm[ridx]
        y = y1 * (1 + sc) + sh                              # sum, product and sum
        dy = dy1 * (1 + sc).abs() + 3 * U * ((y1 * (1 + sc)).abs() + sh.abs())
        # Linear 1536 -> 8: per lane 24 products on one accumulator, the 6-level tree, the bias
        o.append(y @ w.T + b8)
        do.append(dy @ w.abs().T + (24 + 6 + 1 + 1) * U * (y.abs() @ w.abs().T + b8.abs()))
    o, do = torch.cat(o), torch.cat(do)
    if "tok8" in got:
        close(c, "tok8", got["tok8"].reshape(n * T, 8), o, do)
    # unpatchify: token channel (p, q, c) of token (ty, tx) -> x0[n, c, 2 ty + p, 2 tx + q]; then + init_flow (one more add)
    unp = lambda t: t.reshape(n, side, side, 2, 2, 2).permute(0, 5, 1, 3, 2, 4).reshape(n, 2, g, g)     # noqa: E731
    x0 = unp(o) + bufs.flat("init_flow").double().reshape(n, 2, g, g)
    close(c, "x0", got["x0"].reshape(n, 2, g, g), x0, unp(do) + U * x0.abs())


# ------------------------------------------------------------------------------------------------------------------
# small_linear
# ------------------------------------------------------------------------------------------------------------------
def small_linear_ref(c, x, w, b):
    """float64 y = act_out(W act_in(x) + b) and the bound of the f32 kernel.  x [m, width] float64."""
    a = c.args
    K, kmod = a["k"], a["kmod"]
    kk = torch.arange(K, device="cuda") % kmod
    if a["act_in"] == 2:
        # timestep sinusoid: f = exp(-ln(1e4) k / half), angle = t f.  In f32: the constant, its product with k and the
        # quotient by half put 3 u |e| on the exponent e (|e| <= 9.22), i.e. 3 u |e| relative on f; expf adds EXP_ULPS ulps,
        # the product t f one rounding.  |cos'|, |sin'| <= 1, function values <= 1: TRIG_ULPS ulps of 1.
        half = kmod // 2
        kf = torch.where(kk < half, kk, kk - half).double()
        e = -math.log(1e4) * kf / half
        ang = x[:, :1] * e.exp()
        xv = torch.where(kk < half, ang.cos(), ang.sin())
        dxv = ang.abs() * (3 * U * e.abs() + EXP_ULPS * ULP + U) + TRIG_ULPS * ULP
    else:
        xv = x[:, kk]
        dxv = torch.zeros_like(xv)
        if a["act_in"] == 1:
            # SiLU x / (1 + expf(-x)): expf EXP_ULPS ulps (a relative error of 1 + e no larger), the sum and the quotient
            xv = xv * torch.sigmoid(xv)
            dxv = xv.abs() * (EXP_ULPS * ULP + 2 * U)
    v = xv @ w.T + b
    # per lane ceil(K/64) products on one accumulator, the 6-level tree, the bias
    nch = -(-K // 64) + 6 + 1 + 1
    dv = nch * U * (xv.abs() @ w.abs().T + b.abs()) + dxv @ w.abs().T
    if a["act_out"] == 1:        # SiLU: |silu'| <= 1.1 (its maximum is 1.0998 at x = 2.4)
        y = v * torch.sigmoid(v)
        return y, 1.1 * dv + y.abs() * (EXP_ULPS * ULP + 2 * U)
    if a["act_out"] == 2:        # ReLU: 1-Lipschitz
        return torch.relu(v), dv
    if a["act_out"] == 3:        # sigmoid 1 / (1 + expf(-v)): |sigmoid'| <= 1/4
        y = torch.sigmoid(v)
        return y, 0.25 * dv + y * (EXP_ULPS * ULP + 2 * U)
    return v, dv


def case_small_linear(c0, gen):
    # exact pass: no input activation, output activation none or ReLU; sparse ternary x and W, integer bias
    c = dataclasses.replace(c0, args={**c0.args, "act_in": 0, "act_out": c0.args["act_out"] if c0.args["act_out"] in (0, 2) else 0})
    a = c.args
    bufs = Bufs(c)
    xw = min(a["k"], a["kmod"])
    x = _sv(bufs.flat("x"), (a["m"], xw), (a["ldx"], 1))
    tern(x, 0.25, gen)
    tern(bufs.flat("w"), 0.125, gen)
    ints(bufs.flat("b"), -3, 3, gen)
    w = bufs.flat("w").double().reshape(a["n"], a["k"])
    y, _ = small_linear_ref(c, x.double(), w, bufs.flat("b").double())
    assert bool((y != 0).any())
    run(c, bufs, {"y": y})
    del bufs
    # random pass at the engine's magnitudes (inputs N(0, 1), weights N(0, 1/K)); the timestep embedder at several t
    c, a = c0, c0.args
    for t in ((0.0, 1.0, 333.3333, 600.0) if a["act_in"] == 2 else (None,)):
        bufs = Bufs(c)
        xw = 1 if a["act_in"] == 2 else min(a["k"], a["kmod"])
        x = _sv(bufs.flat("x"), (a["m"], xw), (a["ldx"], 1))
        if t is None:
            rnd(x, 1.0, gen)
        else:
            x.fill_(t)
        rnd(bufs.flat("w"), 1.0 / math.sqrt(a["k"]), gen)
        rnd(bufs.flat("b"), 0.1, gen)
        got = run(c, bufs)["y"]
        y, dy = small_linear_ref(c, x.double(), bufs.flat("w").double().reshape(a["n"], a["k"]), bufs.flat("b").double())
        close(c, "y" if t is None else f"y(t={t})", got, y, dy)


# ------------------------------------------------------------------------------------------------------------------
# adaptive positional encoding
# ------------------------------------------------------------------------------------------------------------------
def case_colmean(c, gen):
    a = c.args
    n, T, C, ch = a["n"], a["t"], a["c"], a["chunks"]
    per = -(-T // ch)                                  # tokens per chunk: the last ones may be short or empty
    for exact in (True, False):
        bufs = Bufs(c)
        z = bufs.flat("z").reshape(n, T, C)
        if exact:
            ints(z, -8, 8, gen)                         # |sum| <= 8 T < 2^24: every partial sum is exact in f32
        else:
            rnd(z, 1.0, gen, 0.25)
        zd = z.double()
        if exact:
            part = torch.zeros(n, ch, C, dtype=torch.float64, device="cuda")
            for k in range(ch):
                if k * per < T:
                    part[:, k] = zd[:, k * per:min(T, (k + 1) * per)].sum(1)
            # one correctly rounded f32 division of an integer below 2^24 by T < 2^15: rounding the float64 quotient to
            # f32 gives the same value (double rounding is innocuous for a quotient when 53 >= 2 * 24 + 2)
            run(c, bufs, {"partial": part, "pooled": (zd.sum(1) / T).float()})
        else:
            got = run(c, bufs)
            # a chunk's partial sum: at most `per` adds (an empty chunk is an exact 0)
            part, mag = (torch.zeros(n, ch, C, dtype=torch.float64, device="cuda") for _ in range(2))
            for k in range(ch):
                if k * per < T:
                    part[:, k] = zd[:, k * per:min(T, (k + 1) * per)].sum(1)
                    mag[:, k] = zd[:, k * per:min(T, (k + 1) * per)].abs().sum(1)
            close(c, "partial", got["partial"].reshape(n, ch, C), part, per * U * mag)
            # per adds in a chunk, `chunks` adds over the partial sums, the division
            close(c, "pooled", got["pooled"].reshape(n, C), zd.mean(1), (per + ch + 1) * U * zd.abs().mean(1))


def case_posenc_add(c, gen):
    a = c.args
    n, side, C = a["n"], a["side"], a["c"]
    for exact in (True, False):
        bufs = Bufs(c)
        for p, lo, s in (("z", 8, 1.0), ("hs", 3, 0.5), ("ws", 3, 0.5), ("htab", 3, 0.5), ("wtab", 3, 0.5)):
            if exact:
                ints(bufs.flat(p), -lo, lo, gen)
            else:
                rnd(bufs.flat(p), s, gen, 0.5 if p in ("hs", "ws") else 0.0)      # hs, ws are sigmoid outputs
        z = bufs.flat("z").double().reshape(n, side, side, C)
        hs, ws = (bufs.flat(p).double().reshape(n, 1, 1, C) for p in ("hs", "ws"))
        ht = bufs.flat("htab").double().reshape(1, side, 1, C)
        wt = bufs.flat("wtab").double().reshape(1, 1, side, C)
        ref = z + hs * ht + ws * wt
        if exact:
            run(c, bufs, {"z": ref})
        else:
            bound = 4 * U * (z.abs() + (hs * ht).abs() + (ws * wt).abs())       # two products, two sums
            close(c, "z", run(c, bufs)["z"].reshape(n, side, side, C), ref, bound)
        del bufs, z, ref


# ------------------------------------------------------------------------------------------------------------------
# depthwise 3x3 + bias + ReLU
# ------------------------------------------------------------------------------------------------------------------
def _dw_ref(x, w9, b):
    """x [n, side, side, c], w9 [9, c] tap-major (dy, dx ascending), b [c]: relu(b + sum of in-range taps), and sum |terms|."""
    n, side, _, ch = x.shape
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))
    acc = b.expand(n, side, side, ch).clone()
    mag = b.abs().expand(n, side, side, ch).clone()
    for t in range(9):
        s = xp[:, t // 3:t // 3 + side, t % 3:t % 3 + side] * w9[t]
        acc += s
        mag += s.abs()
    return torch.relu(acc), mag


def case_dwconv3x3(c, gen):
    a = c.args
    n, side, C = a["n"], a["side"], a["c"]
    assert c.args["in16"][0] == c.args["out16"][0]            # both halves of mlp16
    # exact pass: small integers - every tap product and partial sum is an integer below 2^11, exact in f32 and in f16
    bufs = Bufs(c)
    ints(bufs.flat("in16"), -3, 3, gen)
    ints(bufs.flat("w9c"), -2, 2, gen)
    ints(bufs.flat("b"), -4, 4, gen)
    ref, _ = _dw_ref(bufs.flat("in16").float().reshape(n, side, side, C), bufs.flat("w9c").reshape(9, C), bufs.flat("b"))
    run(c, bufs, {"out16": ref})
    del bufs, ref
    # random pass: post-ReLU f16 activations, taps N(0, 0.3); whole images of a seeded subset of channels in float64
    bufs = Bufs(c)
    x16 = bufs.flat("in16")
    rnd(x16, 1.0, gen)
    x16.clamp_(min=0)
    rnd(bufs.flat("w9c"), 0.3, gen)
    rnd(bufs.flat("b"), 0.2, gen)
    got = run(c, bufs)["out16"].reshape(n, side, side, C)
    rs = np.random.default_rng(a["side"])
    idx = sorted(set(rs.integers(0, C, 48).tolist()) | {0, 7, 8, 511, 512, C - 1})
    idx = torch.as_tensor(idx, device="cuda")
    ref, mag = _dw_ref(x16.reshape(n, side, side, C)[..., idx].double(), bufs.flat("w9c").reshape(9, C)[:, idx].double(),
                       bufs.flat("b")[idx].double())
    # the bias and 9 FMAs on one accumulator (the f16 -> f32 conversion of the input is exact); ReLU is 1-Lipschitz
    close(c, "out16", got[..., idx], ref, f16_bound(ref, 9 * U * mag))


# ------------------------------------------------------------------------------------------------------------------
# rows of the r-embedder GEMM
# ------------------------------------------------------------------------------------------------------------------
def _r_rows_layout(flow, init_feat, ldo):
    """cat([init_flow, init_feat], dim=1) [n, 258, g, g] as 2x2 patch rows in (p, q, channel) order, K padded with zeros."""
    n, _, g, _ = flow.shape
    side = g // 2
    x = torch.cat([flow, init_feat], dim=1)
    rows = x.reshape(n, 258, side, 2, side, 2).permute(0, 2, 4, 3, 5, 1).reshape(n * side * side, 4 * 258)
    return F.pad(rows, (0, ldo - 4 * 258))


def case_build_r_rows(c, gen):
    a = c.args
    n, g, hyp, mode = a["n"], a["g"], a["n_hyp"], a["mode"]
    docs = n // hyp
    bufs = Bufs(c)
    feat = bufs.flat("feat").reshape(docs, g, g, 256)
    flow = bufs.flat("flow").reshape(n, 2, g, g)
    if mode != 2:
        # pure data movement on f16-representable values: bit-equal
        feat.copy_(torch.randint(-64, 65, feat.shape, generator=gen, device="cuda") / 8.0)
        flow.copy_(torch.randint(-64, 65, flow.shape, generator=gen, device="cuda") / 128.0)
        if mode == 3:
            fi = bufs.flat("init_feat").reshape(n, 256, g, g)
            fi.copy_(torch.randint(-64, 65, fi.shape, generator=gen, device="cuda") / 8.0)
        init = {0: lambda: torch.zeros(n, 256, g, g, device="cuda"),
                1: lambda: feat.permute(0, 3, 1, 2).repeat_interleave(hyp, 0),
                3: lambda: bufs.flat("init_feat").reshape(n, 256, g, g)}[mode]()
        run(c, bufs, {"out16": _r_rows_layout(flow, init, a["ldo"])})
        return
    # mode 2: init_feat = grid_sample(feat_doc, (init_flow + base) * 2 - 1), bilinear, zeros padding, align_corners=True,
    # base = linspace(0, 1, g) in x and y.  Sampling positions (in pixels): a quarter exactly on integer positions from 3
    # outside the image to 3 outside on the other side (borders included), a quarter anywhere in that range, the rest
    # within +-0.4 of the image size around their own pixel.
    rnd(feat, 1.0, gen)
    px = torch.arange(g, device="cuda", dtype=torch.float32)
    base = torch.stack([px.expand(g, g), px[:, None].expand(g, g)])[None]                  # pixel coordinates x, y
    kind = torch.rand((n, 1, g, g), generator=gen, device="cuda")
    tgt_int = torch.randint(-3, g + 3, (n, 2, g, g), generator=gen, device="cuda").float()
    tgt_any = torch.rand((n, 2, g, g), generator=gen, device="cuda") * (g + 5) - 3
    fl = (torch.rand((n, 2, g, g), generator=gen, device="cuda") * 0.8 - 0.4)
    fl = torch.where(kind < 0.25, (tgt_int - base) / (g - 1), torch.where(kind < 0.5, (tgt_any - base) / (g - 1), fl))
    flow.copy_(fl)
    got = run(c, bufs)["out16"]
    fd = flow.double()
    pos = (((fd + base.double() / (g - 1)) * 2 - 1) + 1) / 2 * (g - 1)                      # [n, 2, g, g]: ix, iy
    # f32 evaluation of the position: x / (g - 1) is two roundings (the reciprocal, the product), the sum with the flow
    # one, 2 s - 1 one, + 1 one, * (g - 1) one: each at most u times a value below (1 + |flow|) in grid units (* 2 for the
    # doubled ones), i.e. (g - 1) u 6 (1 + |flow|) pixels, plus u |position| for the last product
    dpos = (g - 1) * U * 6 * (1 + fd.abs()) + U * pos.abs()
    init = torch.empty(n, 256, g, g, dtype=torch.float64, device="cuda")
    dinit = torch.empty_like(init)
    for i in range(n):
        f = feat[i // hyp].double()                                              # [g, g, 256]
        # the sampled value is piecewise bilinear and continuous in the position (zeros outside): its slope in x is at
        # most the largest difference of horizontal neighbours, the zero padding included; same in y
        fp = F.pad(f, (0, 0, 1, 1, 1, 1))
        lx = (fp[:, 1:] - fp[:, :-1]).abs().amax((0, 1))
        ly = (fp[1:] - fp[:-1]).abs().amax((0, 1))
        ix, iy = pos[i, 0], pos[i, 1]
        x0, y0 = ix.floor(), iy.floor()
        val = torch.zeros(g, g, 256, dtype=torch.float64, device="cuda")
        mag = torch.zeros_like(val)
        for dyy in (0, 1):
            for dxx in (0, 1):
                xx, yy = x0 + dxx, y0 + dyy
                wgt = (1 - (ix - xx).abs()) * (1 - (iy - yy).abs())
                ok = (xx >= 0) & (xx < g) & (yy >= 0) & (yy < g)
                tap = f[yy.clamp(0, g - 1).long(), xx.clamp(0, g - 1).long()] * (wgt * ok)[..., None]
                val += tap
                mag += tap.abs()
        # weights: two differences and a product each, then four FMAs: 8 roundings over the four terms
        err = lx * dpos[i, 0][..., None] + ly * dpos[i, 1][..., None] + 8 * U * mag
        init[i], dinit[i] = val.permute(2, 0, 1), err.permute(2, 0, 1)
    ref = _r_rows_layout(fd, init, a["ldo"])
    dref = _r_rows_layout(torch.zeros_like(fd), dinit, a["ldo"])
    assert bool((got[:, 4 * 258:] == 0).all()), f"{c.site}: K padding not zero"
    close(c, "out16", got[:, :4 * 258], ref[:, :4 * 258], f16_bound(ref, dref)[:, :4 * 258])
    # the special positions are there: more than a pixel outside on each side, and on (within f32 rounding of) integers
    assert bool((pos < -1).any()) and bool((pos > g).any()) and bool(((pos - pos.round()).abs() < 1e-3).all(1).any())


# ------------------------------------------------------------------------------------------------------------------
# data movement
# ------------------------------------------------------------------------------------------------------------------
def case_patch_rows(c, gen):
    a = c.args
    n, C, g = a["n"], a["c"], a["g"]
    side = g // 2
    bufs = Bufs(c)
    rnd(bufs.flat("in"), 1.0, gen)
    x = _sv(bufs.flat("in"), (n, C, g, g), (a["sn"], a["sc"], a["sy"], a["sx"]))      # element [n, channel, y, x]
    ref = x.reshape(n, C, side, 2, side, 2).permute(0, 2, 4, 3, 5, 1).reshape(n * side * side, 4 * C)
    run(c, bufs, {"out": ref})


def case_im2col3x3(c, gen):
    a = c.args
    C, h, w = a["c"], a["h"], a["w"]
    bufs = Bufs(c)
    rnd(bufs.flat("in"), 1.0, gen)
    x = F.pad(_sv(bufs.flat("in"), (C, h, w), (a["sc"], a["sy"], a["sx"])), (1, 1, 1, 1))
    taps = torch.stack([x[:, ky:ky + h, kx:kx + w] for ky in range(3) for kx in range(3)])          # [9, C, h, w]
    ref = F.pad(taps.permute(2, 3, 0, 1).reshape(h * w, 9 * C), (0, a["ldo"] - 9 * C))
    run(c, bufs, {"out": ref})


def case_nhwc_to_nchw(c, gen):
    a = c.args
    bufs = Bufs(c)
    rnd(bufs.flat("in"), 1.0, gen)
    run(c, bufs, {"out": bufs.flat("in").reshape(a["h"] * a["w"], a["c"]).t().contiguous()})


def case_maxpool2_nhwc(c, gen):
    a = c.args
    bufs = Bufs(c)
    rnd(bufs.flat("in"), 1.0, gen)
    x = bufs.flat("in").reshape(a["h"] // 2, 2, a["w"] // 2, 2, a["c"])
    run(c, bufs, {"out": x.amax((1, 3))})


def case_resize_bilinear_nhwc(c, gen):
    a = c.args
    C, hin, win, hout, wout = a["c"], a["hin"], a["win"], a["hout"], a["wout"]
    bufs = Bufs(c)
    rnd(bufs.flat("in"), 1.0, gen)
    x = bufs.flat("in").double().reshape(hin, win, C)
    got = run(c, bufs)["out"].reshape(hout, wout, C)

    def axis(nin, nout):
        f = torch.arange(nout, device="cuda", dtype=torch.float64) * (nin - 1) / (nout - 1)          # align_corners=True
        i0 = f.floor().clamp(max=nin - 1).long()
        return i0, (i0 + 1).clamp(max=nin - 1), f - i0

    y0, y1, wy = axis(hin, hout)
    x0, x1, wx = axis(win, wout)
    wy, wx = wy[:, None, None], wx[None, :, None]

    def interp(t):
        return (1 - wy) * ((1 - wx) * t[y0][:, x0] + wx * t[y0][:, x1]) + wy * ((1 - wx) * t[y1][:, x0] + wx * t[y1][:, x1])

    # source position = scale * index in f32: the rounded scale and the product, 2 u (nin - 1) pixels; the result is
    # continuous and piecewise bilinear in it: slope <= the largest neighbour difference.  Weights (a difference each, two
    # complements) and the 3 products + 3 sums of the blend: 8 roundings over the four weighted taps.
    ly = (x[1:] - x[:-1]).abs().amax((0, 1))
    lx = (x[:, 1:] - x[:, :-1]).abs().amax((0, 1))
    bound = ly * 2 * U * (hin - 1) + lx * 2 * U * (win - 1) + 8 * U * interp(x.abs())
    close(c, "out", got, interp(x), bound)


def _conv_ref(x, wgt, bias, C, h, w):
    """x [h, w, C], wgt [cout, kp] with column (ky * 3 + kx) * C + channel, pad 1: relu(conv + bias) as 9 shifted matrix
    products, [h * w, cout]."""
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))
    acc = bias.expand(h * w, -1).clone()
    for t in range(9):
        acc += xp[t // 3:t // 3 + h, t % 3:t % 3 + w].reshape(h * w, C) @ wgt[:, t * C:(t + 1) * C].T
    return acc


def case_conv3x3_nhwc(c, gen):
    a = c.args
    C, co, h, w, kp = a["c"], a["cout"], a["h"], a["w"], a["kp"]
    assert a["relu"] == 1
    for exact in (True, False):
        bufs = Bufs(c)
        if exact:                    # sparse ternary operands, integer bias: every partial sum is a small integer
            tern(bufs.flat("in"), 0.125, gen)
            tern(bufs.flat("wgt"), 0.125, gen)
            ints(bufs.flat("bias"), -2, 2, gen)
        else:
            rnd(bufs.flat("in"), 1.0, gen)
            rnd(bufs.flat("wgt"), 1.0 / math.sqrt(9 * C), gen)
            rnd(bufs.flat("bias"), 0.1, gen)
        x = bufs.flat("in").double().reshape(h, w, C)
        wg, b = bufs.flat("wgt").double().reshape(co, kp), bufs.flat("bias").double()
        ref = torch.relu(_conv_ref(x, wg, b, C, h, w))
        if exact:
            run(c, bufs, {"out": ref})
        else:
            # K = 9 C products summed in an order the GEMM chooses, then the bias: for ANY order at most (K + 1) roundings
            # on each partial sum; ReLU is 1-Lipschitz
            mag = _conv_ref(x.abs(), wg.abs(), b.abs(), C, h, w)
            close(c, "out", run(c, bufs)["out"].reshape(h * w, co), ref, (9 * C + 1) * U * mag)
        del bufs, x, ref


def case_dither_f16(c, gen):
    a = c.args
    for step in (a["step"], a["step"] + 5):
        cc = dataclasses.replace(c, args={**a, "step": step})
        bufs = Bufs(cc)
        w = torch.randn(a["nelem"], generator=gen, device="cuda") * 0.03          # a weight as (hi, lo) = (f16(W), f16(W - hi))
        hi = w.half()
        bufs.flat("hi").copy_(hi)
        bufs.flat("lo").copy_((w - hi.float()).half())
        ref = dither_ref(bufs.flat("hi").cpu().numpy(), bufs.flat("lo").cpu().numpy(), a["elem0"], step)
        assert (ref != hi.cpu().numpy()).any()
        run(cc, bufs, {"out": torch.from_numpy(ref).cuda()})
        del bufs


CASE_FN = {k: globals()["case_" + k] for k in TS.PARAMS}


# ------------------------------------------------------------------------------------------------------------------
# the cases: each distinct record once per size
# ------------------------------------------------------------------------------------------------------------------
def _key(c):
    ptr = TS.POINTERS[c.kernel]
    ws = set(TS.workspace_bytes(16, 1, 1)) | {"x_t", "init_flow", "init_feat", "x0_out", "mask_y512", "line_msk", "feat_out"}
    k = [c.site]
    for p, v in c.args.items():
        if p not in ptr:
            k.append(v)
        else:                                          # the six decoder layers repeat one record with other weights
            k.append(None if v is None else (v[0] if v[0] in ws else "weight", v[1]))
    return tuple(k)


def _cases():
    out, ids = [], []
    only64 = ("small_linear", "colmean", "posenc_add")
    for G, docs, hyp in ((288, 1, 2), (72, 1, 2), (72, 4, 2), (16, 5, 2), (64, 32, 2)):
        recs = TS.calls(G, docs, hyp, feat_mode=1)
        recs += [c for m in (0, 2, 3) for c in TS.calls(G, docs, hyp, feat_mode=m) if c.site == "r_rows"]
        seen, nel = set(), set()
        last = {s: [c for c in recs if c.site == s][-1] for s in ("feat_resize", "feat_nchw", "dither") if
                any(c.site == s for c in recs)}
        for c in recs:
            if G == 64 and c.kernel not in only64:
                continue
            if c.site.startswith("pyr_") and G != 288:          # fixed 512 x 512 sizes: once
                continue
            if c.site in ("feat_resize", "feat_nchw") and c.note["doc"] not in (0, last[c.site].note["doc"]):
                continue
            if c.site == "dither":                              # each weight size once, and the last (largest elem0)
                if (G, docs) != (288, 1) and c is not last["dither"]:
                    continue
                if c.args["nelem"] in nel and c is not last["dither"]:
                    continue
                nel.add(c.args["nelem"])
            k = _key(c)
            if k in seen:
                continue
            seen.add(k)
            tag = "".join(f"-{n}{v}" for n, v in c.note.items() if n in ("layer", "stream", "doc", "weight"))
            if c.site == "r_rows":
                tag += f"-mode{c.args['mode']}"
            if c.site == "pyr_pool" or c.site == "pyr_conv":
                tag = f"-layer{c.note['layer']}"
            out.append(c)
            ids.append(f"G{G}-s{docs * hyp}-{c.site}{tag}")
        # per-sample modulation (ldmod = c, mod_rows = T): in the ABI, not used by the engine
        if G in (72, 16):
            ln = next(c for c in recs if c.site == "ln_attn")
            N, T = docs * hyp, (G // 2) ** 2
            out.append(dataclasses.replace(ln, args={**ln.args, "shift": ("modrows", 0), "scale": ("modrows", N * 384 * 4),
                                                     "ldmod": 384, "mod_rows": T}))
            ids.append(f"G{G}-s{N}-ln_attn-per_sample_mod")
    assert len(set(ids)) == len(ids), [i for i in ids if ids.count(i) > 1]
    return out, ids


CASES, CASE_IDS = _cases()


def test_every_site_has_a_large_and_a_small_case():
    for site, _, _ in TS.SITES:
        mine = [i for i in CASE_IDS if f"-{site}" in i]
        assert any(i.startswith("G288-") for i in mine), site
        if not site.startswith("pyr_") and site != "dither":            # the 512 x 512 pyramid has one size; dithering
            assert any(i.startswith(("G72-", "G16-")) for i in mine), site     # runs on large grids only (G = 72 included)
    assert any(i.startswith("G72-") and "-dither" in i for i in CASE_IDS)


@pytest.mark.parametrize("i", range(len(CASES)), ids=CASE_IDS)
def test_engine_token_call_site_vs_float64(i):
    """One token-side launch exactly as the engine issues it.  Bounds and the figures measured on an MI355X are printed per
    output (`max err / bound`); see the module docstring for the error model."""
    c = CASES[i]
    gen = torch.Generator(device="cuda")
    gen.manual_seed(4000 + i)
    try:
        CASE_FN[c.kernel](c, gen)
    finally:
        torch.cuda.empty_cache()
