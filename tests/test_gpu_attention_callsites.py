"""The six product attention kernels (the library picks one from head_dim, tq and tk) on exact probes, against a per-element
bound derived from their arithmetic, at the engine's four call forms, and across layouts - product library only, no lab
build, no environment switch.  tests/attention_model.py holds the probes, the bound and their derivations;
tests/test_attention_model_cpu.py shows on an emulation that each check can fail.

Every launch writes into a sentinel-filled allocation with guard rows before row 0 and after row tq - 1 of every batch and
pad columns beside the heads' columns (the engine forms: the neighbouring slabs of att16); everything outside [b, :tq, :C]
must come back unchanged, compared as int16.  Q, K and V^T are views with ld > C into NaN-filled allocations.

Selector and census are required bit for bit on every kernel (the census at a ragged key count to one f16 ulp, as derived in
attention_model.census_probe); no kernel / probe pair needed the one-ulp allowance."""
import ctypes as C

import pytest
import torch

from dvd_amd import lib

import attention_callsites as CS
import attention_model as AM

pytestmark = pytest.mark.gpu

DEV = "cuda"                       # where every operand is allocated
SENT = 0x3555                      # f16 0.33325: finite, and no probe's answer
G0, G1, PAD = 2, 3, 8              # guard rows before / after every batch of O; pad columns of every operand

R64X, H64X = "flash_attn_r64x_kernel<0>", "flash_attn_h64x_kernel<0, true>"
GLDS = {64: "flash_attn_glds_kernel<64, 0>", 256: "flash_attn_glds_kernel<256, 0>"}
REG = {64: "flash_attn_kernel<64>", 256: "flash_attn_kernel<256>"}
GEN = {64: H64X, 256: R64X}


def nan16(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float16, device=DEV)


def launch(prob, interleave=False, kernel=None, pad=PAD):
    """One dvd_flash_attn of prob's (q, k, v) with every operand a padded view; returns the [B, tq, C] output (CPU) after the
    canary check.  interleave: Q and K as the column halves of one [B, T, 2C + pad] buffer (the engine's fused projection).
    pad = 0: every operand contiguous (ld = C, V^T ld = tk); O keeps its guard rows, which lie outside the tensor."""
    q, k, v, heads, hd = (prob[n] for n in ("q", "k", "v", "heads", "hd"))
    B, tq, Cc = q.shape
    Bkv, tk, _ = k.shape
    if kernel is not None:
        assert lib.flash_attn_kernel_name(hd, tq, tk) == kernel, (hd, tq, tk, lib.flash_attn_kernel_name(hd, tq, tk))
    if interleave:
        assert Bkv == B
        qk = nan16(B, max(tq, tk), 2 * Cc + pad)
        qd, kd = qk[:, :tq, :Cc], qk[:, :tk, Cc:2 * Cc]
    else:
        qd, kd = nan16(B, tq, Cc + pad)[:, :, :Cc], nan16(Bkv, tk, Cc + 2 * pad)[:, :, :Cc]
    qd.copy_(q)
    kd.copy_(k)
    vt = nan16(Bkv, Cc, tk + pad)[:, :, :tk]
    vt.copy_(v.transpose(1, 2))
    oall = torch.full((B, G0 + tq + G1, Cc + pad), SENT, dtype=torch.int16, device=DEV)
    od = oall.view(torch.float16)[:, G0:G0 + tq, :Cc]
    d = lib.AttnDesc()
    d.head_dim, d.heads, d.batch, d.tq, d.tk, d.kv_batch_div = hd, heads, B, tq, tk, prob["kv_div"]
    d.Q, d.ldq, d.strideQ = qd.data_ptr(), qd.stride(1), qd.stride(0)
    d.K, d.ldk, d.strideK = kd.data_ptr(), kd.stride(1), kd.stride(0)
    d.Vt, d.ldvt, d.strideVt = vt.data_ptr(), vt.stride(1), vt.stride(0)
    d.O, d.ldo, d.strideO = od.data_ptr(), od.stride(1), od.stride(0)
    d.scale = prob["scale"]
    lib.call("dvd_flash_attn", C.byref(d), lib.stream_ptr())
    torch.cuda.synchronize()
    host = oall.cpu()
    out = host.view(torch.float16)[:, G0:G0 + tq, :Cc].clone()
    host[:, G0:G0 + tq, :Cc] = SENT
    stray = (host != SENT).nonzero()
    assert stray.numel() == 0, f"stores outside [b, :tq, :C]: {stray.shape[0]}, first (b, row - {G0}, col) = {stray[0].tolist()}"
    return out


def bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


def first_diff(out, want):
    bad = (out.view(torch.int16) != want.view(torch.int16)).nonzero()
    return f"{bad.shape[0]} elements differ, first (b, row, col) = {bad[0].tolist()}" if bad.numel() else "equal"


def run_probes(kernel, B, Bkv, tq, tk, heads, hd, seed):
    sel = AM.selector_probe(B, Bkv, tq, tk, heads, hd, seed)
    out = launch(sel, kernel=kernel)
    assert bits_equal(out, sel["want"]), (kernel, "selector", first_diff(out, sel["want"]))
    cen = AM.census_probe(B, Bkv, tq, tk, heads, hd, seed + 1)
    out = launch(cen, kernel=kernel)
    ok, ulps = AM.census_ok(out, cen)
    assert ok, (kernel, "census", f"largest error {ulps} f16 ulps", "exact" if cen["exact"] else "to one ulp (ragged tk)")


# ---- 1. selector and census on every product kernel ----------------------------------------------------------------
GEN_SHAPES = [(5377, tk) for tk in (64, 128, 192, 256, 320, 384, 448, 896)] + [(tq, 192) for tq in (5376, 5393, 5500)]
GLDS_SHAPES = [(tq, tk) for tq in (1, 31, 128, 129, 300) for tk in (64, 192, 512)]
REG_SHAPES = [(tq, tk) for tk in (8, 56, 72, 136, 1000) for tq in (1, 200)] + [(5400, 72)]
BATCHES = [(2, 2), (3, 1)]


@pytest.mark.parametrize("B,Bkv", BATCHES)
@pytest.mark.parametrize("tq,tk", GEN_SHAPES)
@pytest.mark.parametrize("hd", [64, 256])
def test_probes_generated_kernels(hd, tq, tk, B, Bkv):
    """r64x / h64x: every exit of the generated loop (2 .. 14 tiles of 32 keys, and 28: a second trip), the exact threshold
    tq = 5376, one live row in the last workgroup (5377), one row past a 16-row query block (5393), ragged (5500)."""
    run_probes(GEN[hd], B, Bkv, tq, tk, 2, hd, seed=tq + tk)


@pytest.mark.parametrize("B,Bkv", BATCHES)
@pytest.mark.parametrize("tq,tk", GLDS_SHAPES)
@pytest.mark.parametrize("hd", [64, 256])
def test_probes_glds_kernels(hd, tq, tk, B, Bkv):
    run_probes(GLDS[hd], B, Bkv, tq, tk, 2, hd, seed=tq + tk)


@pytest.mark.parametrize("B,Bkv", BATCHES)
@pytest.mark.parametrize("tq,tk", REG_SHAPES)
@pytest.mark.parametrize("hd", [64, 256])
def test_probes_register_staged_kernels(hd, tq, tk, B, Bkv):
    """Ragged key counts: fewer keys than a tile (8, 56), a masked tail after one, two and fifteen whole tiles; tq = 5400 stays
    on this kernel although it is past the generated kernels' threshold."""
    run_probes(REG[hd], B, Bkv, tq, tk, 2, hd, seed=tq + tk)


@pytest.mark.parametrize("hd", [64, 256])
@pytest.mark.parametrize("family,tq,tk", [("gen", 5377, 192), ("glds", 300, 192), ("reg", 200, 136)])
def test_probes_six_heads(hd, family, tq, tk):
    run_probes({"gen": GEN, "glds": GLDS, "reg": REG}[family][hd], 2, 1, tq, tk, 6, hd, seed=6)


# ---- 2. the per-element bound ---------------------------------------------------------------------------------------
def check_bound(out, case, kernel, what, rows=None, pairs=None):
    """|out - ref| <= bound for every element of the (batch, head) `pairs` (default: all) and query `rows` (default: all), and the
    same around the float64 output of the kernel's own operands (Q c rounded to f16 on the head_dim 64 LDS-DMA kernels)."""
    heads, hd, kv_div = case["heads"], case["hd"], case["kv_div"]
    worst = worst_k = 0.0
    for b, h in (pairs or [(b, h) for b in range(case["q"].shape[0]) for h in range(heads)]):
        hs = slice(h * hd, (h + 1) * hd)
        kb = b // kv_div
        r, e, rk, ek = AM.bound(case["q"][b:b + 1, :, hs], case["k"][kb:kb + 1, :, hs], case["v"][kb:kb + 1, :, hs], 1, hd,
                                case["scale"], 1, kernel, rows=rows, ideal=True)
        o = out[b:b + 1, :, hs] if rows is None else out[b:b + 1, rows][:, :, hs]
        assert torch.isfinite(o).all(), (kernel, what, b, h)
        worst = max(worst, float(((o.double() - r).abs() / e).max()))
        worst_k = max(worst_k, float(((o.double() - rk).abs() / ek).max()))
    line = f"{kernel} {what}: largest err/bound {worst:.3f}, around the kernel's own operands {worst_k:.3f}"
    print("\nattention bound: " + line)
    assert worst <= 1.0 and worst_k <= 1.0, line
    return worst


@pytest.mark.parametrize("amp", [1.0, 1.5, 3.0])
@pytest.mark.parametrize("hd", [64, 256])
@pytest.mark.parametrize("family,tq,tk", [("gen", 5377, 448), ("glds", 300, 512), ("reg", 200, 1000)])
def test_bound_per_kernel(hd, family, tq, tk, amp):
    """Random inputs as in the CPU test (amplitudes 1, 1.5 and 3, six planted dominant keys, V columns scaled 2^-8 .. 2^4), two
    heads; at (5377, 448) one batch, which keeps the float64 work of a case under 10 GFLOP, else two batches on one K / V.
    At amplitude 3 the scores spread over about 13 log2 units, so a later tile passes the row's m by more than THR in
    nearly every tile: the deferred rescale - in r64x / h64x the rare block that scales O^T, l and the packed P(t) by
    f16(alpha) - runs at moderate alpha, which the selector (alpha 0 or 1) cannot show."""
    kernel = {"gen": GEN, "glds": GLDS, "reg": REG}[family][hd]
    B, Bkv = (1, 1) if family == "gen" else (2, 1)
    case = AM.random_case(B, Bkv, tq, tk, 2, hd, amp, seed=int(10 * amp) + hd)
    check_bound(launch(case, kernel=kernel), case, kernel, f"({tq}, {tk}) amp {amp}")


# ---- 3. the engine's call forms -------------------------------------------------------------------------------------
GUARD = 4096                       # sentinel elements before and after att16


class EngineBuffers:
    """One device allocation per workspace buffer the attention sites of calls(G, 1, 2) touch; att16 whole, sentinel-filled."""

    def __init__(self, calls, G):
        size = {}
        for c in calls:
            for f in ("Q", "K", "Vt"):
                buf, off = getattr(c, f)
                size[buf] = max(size.get(buf, 0), off + CS.extent(c, f))
        self.buf = {n: nan16(s) for n, s in size.items()}
        self.natt = CS.att16_elements(G, 1, 2)
        self.att = torch.full((GUARD + self.natt + GUARD,), SENT, dtype=torch.int16, device=DEV)

    def address(self, p):
        buf, off = p
        return self.att.data_ptr() + 2 * (GUARD + off) if buf == "att16" else self.buf[buf].data_ptr() + 2 * off

    def fill(self, c, q, k, v):
        view = lambda p, shape, strides: torch.as_strided(self.buf[p[0]], shape, strides, p[1])       # noqa: E731
        view(c.Q, (c.batch, c.tq, c.C), (c.sQ, c.ldq, 1)).copy_(q)
        view(c.K, (c.kv_batch, c.tk, c.C), (c.sK, c.ldk, 1)).copy_(k)
        view(c.Vt, (c.kv_batch, c.C, c.tk), (c.sVt, c.ldvt, 1)).copy_(v.transpose(1, 2))

    def run(self, c):
        """launch c; the output [batch, tq, C] (CPU); everything else of att16 and its guards must still hold the sentinel"""
        self.att.fill_(SENT)
        lib.call("dvd_flash_attn", C.byref(CS.descriptor(c, self.address)), lib.stream_ptr())
        torch.cuda.synchronize()
        host = self.att.cpu()
        lo = GUARD + c.O[1]
        n = CS.extent(c, "O")
        assert c.ldo == c.C and c.sO == c.tq * c.C and n == c.batch * c.tq * c.C      # the engine's outputs are dense slabs
        out = host[lo:lo + n].view(torch.float16).reshape(c.batch, c.tq, c.C).clone()
        host[lo:lo + n] = SENT
        stray = (host != SENT).nonzero()
        assert stray.numel() == 0, (c.site, f"{stray.shape[0]} stores outside the slab, first at att16 element "
                                            f"{int(stray[0]) - GUARD}")
        return out


def gathered(v, pi, kv_div, heads, hd):
    want = torch.empty(pi.shape[0], pi.shape[2], heads * hd, dtype=torch.float16)
    for b in range(pi.shape[0]):
        for h in range(heads):
            want[b, :, h * hd:(h + 1) * hd] = v[b // kv_div, pi[b, h], h * hd:(h + 1) * hd]
    return want


def bound_rows(T, n):
    """n query rows: the first workgroup's, the last workgroup's, and a stride between them"""
    if T <= n:
        return torch.arange(T)
    e = n // 4
    return torch.cat([torch.arange(e), torch.linspace(e, T - e - 1, n - 2 * e).long(), torch.arange(T - e, T)]).unique()


ENGINE_KERNELS = {160: GEN, 16: GLDS, 72: REG}


@pytest.mark.parametrize("site", ["ca_doc", "ca_r", "sa", "dec"])
@pytest.mark.parametrize("G", [160, 16, 72])
def test_engine_call_forms(G, site):
    """The descriptors of attention_callsites.calls(G, 1, 2) over real allocations: selector and census on the whole output of
    every launch of the site, the bound on <= 256 query rows of two heads of the first and the last batch (the decoder at
    G = 160: 128 rows) at amplitude 1.5 and - the rescale at moderate alpha, see test_bound_per_kernel - at 3, the rest of
    att16 guarded.  The three document streams share Q and differ in K / V^T."""
    calls = [c for c in CS.calls(G, 1, 2) if c.site == site and c.note.get("layer", 0) == 0]
    c0 = calls[0]
    kernel = ENGINE_KERNELS[G][c0.head_dim]
    assert lib.flash_attn_kernel_name(c0.head_dim, c0.tq, c0.tk) == kernel
    eb = EngineBuffers(calls, G)
    shape = (c0.batch, c0.kv_batch, c0.tq, c0.tk, c0.heads, c0.head_dim)
    perm = [lambda v: v, lambda v: v.flip(1), lambda v: v.roll(17, 1)]       # a stream's V = the probe's, keys re-ordered

    sel = AM.selector_probe(*shape, seed=G)
    for s, c in enumerate(calls):
        eb.fill(c, sel["q"], sel["k"], perm[s](sel["v"]))
    for s, c in enumerate(calls):
        out = eb.run(c)
        want = gathered(perm[s](sel["v"]), sel["pi"], c.kv_div, c.heads, c.head_dim)
        assert bits_equal(out, want), (site, s, "selector", first_diff(out, want))

    cen = AM.census_probe(*shape, seed=G + 1)
    for c in calls:
        eb.fill(c, cen["q"], cen["k"], cen["v"])
    for s, c in enumerate(calls):
        ok, ulps = AM.census_ok(eb.run(c), cen)
        assert ok, (site, s, "census", ulps)

    rows = bound_rows(c0.tq, 128 if (G == 160 and c0.head_dim == 256) else 256)
    pairs = sorted({(b, h) for b in (0, c0.batch - 1) for h in (1, c0.heads - 2)})
    for amp in (1.5, 3.0):
        q = None
        for s, c in enumerate(calls):
            case = AM.random_case(*shape, amp, seed=G + 2 + s + int(10 * amp), q=q)
            q = case["q"]
            eb.fill(c, case["q"], case["k"], case["v"])
            check_bound(eb.run(c), case, kernel, f"engine {site}[{s}] G={G} amp {amp}", rows=rows,
                        pairs=pairs if s == 0 or G != 160 else pairs[:1])


# ---- 4. layout invariance -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hd", [64, 256])
@pytest.mark.parametrize("family,tq,tk", [("gen", 5376, 256), ("glds", 300, 256), ("reg", 200, 136)])
def test_layout_invariance(hd, family, tq, tk):
    """One (q, k, v) problem gives the same bits alone (heads 1, batch 1, every operand contiguous: ld = C), as head 3 of 6,
    as batch 4 of 5, with Q and K interleaved in one buffer, and as one of three batches that share a K / V (kv_div 3) - these
    four in padded views.  No reference."""
    kernel = {"gen": GEN, "glds": GLDS, "reg": REG}[family][hd]
    one = AM.random_case(1, 1, tq, tk, 1, hd, 1.5, seed=hd + tq)
    alone = launch(one, kernel=kernel, pad=0)
    assert torch.isfinite(alone).all()

    def embed(B, Bkv, heads, b, h, seed):
        big = AM.random_case(B, Bkv, tq, tk, heads, hd, 1.5, seed=seed)
        hs = slice(h * hd, (h + 1) * hd)
        big["q"][b, :, hs] = one["q"][0]
        big["k"][b // big["kv_div"], :, hs], big["v"][b // big["kv_div"], :, hs] = one["k"][0], one["v"][0]
        return big, (b, slice(None), hs)

    for what, (big, at), inter in (("head 3 of 6", embed(1, 1, 6, 0, 3, 1), False),
                                   ("batch 4 of 5", embed(5, 5, 1, 4, 0, 2), False),
                                   ("interleaved Q / K", embed(2, 2, 2, 1, 1, 3), True),
                                   ("kv_div 3, batch 1 of 3", embed(3, 1, 1, 1, 0, 4), False)):
        out = launch(big, interleave=inter, kernel=kernel)[at]
        assert bits_equal(out, alone[0]), (kernel, what, first_diff(out[None], alone))
