"""The GEMM of every engine call site at the engine's own shapes against float64, and the batch == single guarantee where
the batch changes the GEMM kernel (t384 FULL vs ragged) or moves stores past 2^31 elements.

At G = 288 every t384 call site has 324 to 2592 tiles on at most 256 persistent workgroups: each workgroup runs several
tiles, and with M % 384 == 0 (FULL) the XT form fetches the next tile's first half-slabs during the current tile's loop.
The unit tests of tests/test_gpu_gemm.py stay below 256 tiles; this file checks the tile hand-off."""
import math

import numpy as np
import pytest
import torch

from dvd_amd import lib, synth

import gemm_callsites as CS

pytestmark = pytest.mark.gpu

ESZ = {torch.float16: 2, torch.float32: 4}


def _ftype(c, f):
    if f in ("A", "B", "A_lo", "B_lo"):
        return torch.float32 if c.dtype == 1 else torch.float16
    return torch.float16 if f == "C16" else torch.float32


def _extent(c, f):
    """Elements from the pointer to one past the last one the GEMM touches."""
    if f in ("A", "A_lo"):
        return (c.batch - 1) * c.sA + (c.M - 1) * c.lda + c.K
    if f in ("B", "B_lo"):
        return (c.batch - 1) * c.sB + (c.N - 1) * c.ldb + c.K
    if f == "C32":
        return (c.batch - 1) * c.sC32 + (c.M - 1) * c.ldc + c.N
    if f == "C16":
        return (c.batch - 1) * c.sC16 + (c.M - 1) * c.ldc16 + c.N
    if f == "res":
        return (c.batch - 1) * c.sRes + (c.M - 1) * c.ldres + c.N
    if f == "bias":
        return c.M if c.bias_row else c.N
    if f == "pos":
        return (c.pos_rows - 1) * c.ldpos + c.N
    if f == "gate":
        return ((c.M - 1) // c.gate_rows) * c.ldgate + c.N
    raise KeyError(f)


def _fields(c):
    return [f for f in CS.PTR_FIELDS if getattr(c, f) is not None]


class Bufs:
    """One device allocation per buffer of the call, 0xFF-filled (NaN as f16 and as f32)."""

    def __init__(self, c):
        size = {}
        for f in _fields(c):
            buf, off = getattr(c, f)
            size[buf] = max(size.get(buf, 0), off + _extent(c, f) * ESZ[_ftype(c, f)])
        self.raw = {b: torch.full((-(-n // 256) * 256,), 255, dtype=torch.uint8, device="cuda") for b, n in size.items()}
        self.c = c

    def flat(self, f, raw=None):
        buf, off = getattr(self.c, f)
        r = (raw or self.raw)[buf]
        return r[off:off + _extent(self.c, f) * ESZ[_ftype(self.c, f)]].view(_ftype(self.c, f))

    def addr(self, p):
        buf, off = p
        return self.raw[buf].data_ptr() + off


def _mat(flat, off, rows, cols, ld):
    """rows x cols at element `off` of `flat` (as_strided's offset counts from the start of the storage, not of the view)"""
    return torch.as_strided(flat, (rows, cols), (ld, 1), flat.storage_offset() + off)


def _gelu(x):
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))


def _reference(c, flat, rows, dev):
    """float64 epilogue(A . B^T) of rows `rows` of every batch: {output field: [batch, len(rows), N]}.  flat(f) -> the
    field's typed flat view (any device); the products run on `dev`."""
    rows_t = torch.as_tensor(rows, dtype=torch.long)
    outs = {f: [] for f in ("C32", "C16") if getattr(c, f) is not None}
    g = lambda f: flat(f).to(dev)                            # noqa: E731
    A, B = g("A"), g("B")
    Alo = g("A_lo") if c.A_lo is not None else None
    Blo = g("B_lo") if c.B_lo is not None else None
    rdev = rows_t.to(dev)
    for b in range(c.batch):
        a = _mat(A, b * c.sA, c.M, c.K, c.lda)[rdev].double()
        if Alo is not None:
            a = a + _mat(Alo, b * c.sA, c.M, c.K, c.lda)[rdev].double()
        w = _mat(B, b * c.sB, c.N, c.K, c.ldb).double()
        if Blo is not None:
            w = w + _mat(Blo, b * c.sB, c.N, c.K, c.ldb).double()
        y = a @ w.T
        if c.bias is not None:
            bias = g("bias").double()
            y = y + (bias[rdev][:, None] if c.bias_row else bias[None, :c.N])
        if c.act == 1:
            y = _gelu(y)
        elif c.act == 2:
            y = torch.relu(y)
        if c.pos is not None:
            y = y + _mat(g("pos"), 0, c.pos_rows, c.N, c.ldpos)[rdev % c.pos_rows].double()
        if c.gate is not None:
            y = y * _mat(g("gate"), 0, (c.M - 1) // c.gate_rows + 1, c.N, c.ldgate)[rdev // c.gate_rows].double()
        if c.res is not None:
            y = y + _mat(g("res"), b * c.sRes, c.M, c.N, c.ldres)[rdev].double()
        for f in outs:
            outs[f].append(y)
    return {f: torch.stack(v) for f, v in outs.items()}


def _out_view(c, flat, f, b):
    ld, s = (c.ldc, c.sC32) if f == "C32" else (c.ldc16, c.sC16)
    return _mat(flat, b * s, c.M, c.N, ld)


def _fill(bufs, c, gen, exact):
    """Inputs: exact -> sparse ternary operands / bias / gate, small integers for pos and residual; else the engine's
    magnitudes (f16 activations ~ N(0, 1), weights ~ N(0, 1/K) as (hi, lo) pairs, f32 epilogue operands)."""
    def rnd(n, scale):
        return torch.randn(n, generator=gen, device="cuda") * scale

    def tern(n, density):
        v = torch.randint(-1, 2, (n,), generator=gen, device="cuda").float()
        return v * (torch.rand(n, generator=gen, device="cuda") < density)

    wfield = "A" if "vt" in c.site else "B"                   # the V^T projections take the weight as A
    for f in _fields(c):
        if f in ("C32", "C16"):
            continue                                            # NaN; a residual output is filled as the residual
        fl = bufs.flat(f)
        n = fl.numel()
        if exact:
            v = {"pos": lambda: torch.randint(-2, 3, (n,), generator=gen, device="cuda").float(),
                 "res": lambda: torch.randint(-8, 9, (n,), generator=gen, device="cuda").float(),
                 "bias": lambda: tern(n, 0.5), "gate": lambda: tern(n, 0.7)}.get(f, lambda: tern(n, 0.125))()
        elif f in ("A", "B"):
            v = rnd(n, 1.0 / math.sqrt(c.K)) if f == wfield else rnd(n, 1.0)
        elif f in ("A_lo", "B_lo"):
            v = rnd(n, 2.0 ** -11 / math.sqrt(c.K))             # the rounding residual of an f32 weight
        else:
            v = rnd(n, {"bias": 0.1, "pos": 0.1, "gate": 0.5, "res": 1.0}[f])
        fl.copy_(v.to(fl.dtype))


CASES = []                        # (G, docs, hyp, call): each distinct descriptor once
for _g, _d, _h in ((288, 1, 2), (72, 1, 2), (72, 4, 2)):
    _seen = set()
    for _c in CS.calls(_g, _d, _h):
        _key = (_c.site, _c.M, _c.N, _c.K, _c.batch, _c.note.get("stream"))
        if _key not in _seen:             # the six decoder layers repeat one descriptor
            _seen.add(_key)
            CASES.append((_g, _d, _h, _c))
CASE_IDS = [f"G{g}-s{d * h}-{c.site}" + (f"-{c.note['stream']}" if "stream" in c.note else "") for g, d, h, c in CASES]


def _fake_name(c, G, docs, hyp):
    bufs = {}

    def addr(p):
        if p[0] not in bufs:
            bufs[p[0]] = (1 << 40) + len(bufs) * (1 << 36)
        return bufs[p[0]] + p[1]
    return lib.gemm_kernel_name(CS.descriptor(c, addr))


def _sample_rows(M, seed):
    rows = set()
    for t in (384, 256):
        for r0 in range(0, M, t):
            rows.update((r0, min(r0 + t, M) - 1))
    rows.update(range(max(0, M - 17), M))                                  # the ragged tail
    rows.update(np.random.default_rng(seed).integers(0, M, 64).tolist())
    return sorted(rows)


@pytest.mark.parametrize("i", range(len(CASES)), ids=CASE_IDS)
def test_engine_gemm_call_site_vs_float64(i):
    """One engine GEMM launch, exactly as the engine describes it (column slices of the [NT, 1536] token buffer with batch
    strides, in-place residual, gate and pos rows, (hi, lo) pairs or one dithered weight), at G = 288 x 2 samples and G = 72 x
    2 and 8 samples.  Exact pass: sparse ternary operands keep every sum an exactly representable integer, so the WHOLE
    output buffer must equal the float64 result (a dropped, repeated or misplaced tile or K slab anywhere fails it).  Random
    pass: the engine's magnitudes, sampled rows against a CPU float64 reference."""
    import dataclasses
    G, docs, hyp, c0 = CASES[i]
    name = _fake_name(c0, G, docs, hyp)
    # the t384 call sites (at G = 72 dec_vt's N = T = 1296 is no multiple of 256: the 128 x 128 family)
    if c0.site in ("sa_qk", "fc1", "dec_qk", "dec_vt", "dec_conv1", "dec_fc", "dec_conv2") and (G, c0.site) != (72, "dec_vt"):
        fl = 2 if c0.site in ("dec_fc", "dec_conv2") else 0
        full = (c0.M % 384 == 0)
        assert name == f"gemm_nt_t384_kernel<0, {fl}, {'true' if full else 'false'}, true>", name
        if G == 288:
            assert full and -(-c0.M // 384) * (c0.N // 256) > 256            # the persistent multi-tile regime
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1000 + i)
    for exact in (True, False):
        # exact pass: GELU left out (fc1's flavour does not depend on it: C16 output without residual)
        c = dataclasses.replace(c0, act=0) if exact and c0.act == 1 else c0
        bufs = Bufs(c)
        _fill(bufs, c, gen, exact)
        d = CS.descriptor(c, bufs.addr)
        assert lib.gemm_kernel_name(d) == name, (lib.gemm_kernel_name(d), name)
        outs = [f for f in ("C32", "C16") if getattr(c, f) is not None]
        if exact:
            want = {b: t.clone() for b, t in bufs.raw.items()}
            ref = _reference(c, bufs.flat, list(range(c.M)), "cuda")
            for f in outs:
                wf = bufs.flat(f, want)
                for b in range(c.batch):
                    _out_view(c, wf, f, b).copy_(ref[f][b].to(wf.dtype))
            del ref
            lib.call("dvd_gemm_nt", d, lib.stream_ptr())
            torch.cuda.synchronize()
            for f in outs:
                got, exp = bufs.flat(f), bufs.flat(f, want)
                bad = ~((got == exp) | (torch.isnan(got) & torch.isnan(exp)))
                assert not bool(bad.any()), (f"{c.site} {f}: {int(bad.sum())} elements differ from the exact integer result, "
                                             f"first at element {int(bad.nonzero()[0])}")
        else:
            before = {f: bufs.flat(f).cpu() for f in _fields(c) if f not in ("C32", "C16")}
            rows = _sample_rows(c.M, i)
            ref = _reference(c, lambda f: before[f], rows, "cpu")
            lib.call("dvd_gemm_nt", d, lib.stream_ptr())
            torch.cuda.synchronize()
            tol = 1e-4 * math.sqrt(c.K)
            ridx = torch.as_tensor(rows, device="cuda")
            for f in outs:
                for b in range(c.batch):
                    got = _out_view(c, bufs.flat(f), f, b)[ridx].double().cpu()
                    exp = ref[f][b]
                    bound = tol + (2.0 ** -11 * exp.abs() if f == "C16" else 0.0)
                    err = (got - exp).abs() - bound
                    assert bool(torch.isfinite(got).all()), f"{c.site} {f} batch {b}: non-finite output"
                    assert float(err.max()) <= 0, f"{c.site} {f} batch {b}: err {float((got - exp).abs().max())}"
        del bufs
    torch.cuda.empty_cache()


@pytest.mark.parametrize("fl", range(5))
def test_t384_full_and_ragged_same_bits(fl):
    """gemm_nt_t384_kernel<0, FL, true, true> (M % 384 == 0: XT look-ahead, no row masks) and <0, FL, false, true> give the
    same bits on the rows they share - the engine runs one or the other for the same document depending on the batch (G = 72:
    one document 2 592 rows, ragged; four 10 368 = 27 x 384 rows, FULL)."""
    gen = torch.Generator(device="cuda")
    gen.manual_seed(77 + fl)
    # (C32, C16, res, act): flavour 0 f16 only, 1 f32 only, 2 f32 + residual, 3 f32 + f16 (+ GELU), 4 f32 + f16 + residual
    c32, c16, use_res, act = {0: (False, True, False, 2), 1: (True, False, False, 0), 2: (True, False, True, 2),
                              3: (True, True, False, 1), 4: (True, True, True, 0)}[fl]
    for N in (1536, 2048, 3072):
        k = -(-513 * 256 // N) + 1                      # more than 512 tiles: every workgroup runs two or three
        for K in (1536, 2048):
            Mf = 384 * k
            Mmax = Mf + 383
            a = torch.randn(Mmax, K, generator=gen, device="cuda").half()
            b = (torch.randn(N, K, generator=gen, device="cuda") / math.sqrt(K)).half()
            bias = torch.randn(N, generator=gen, device="cuda") * 0.1
            res = torch.randn(Mmax, N, generator=gen, device="cuda")
            base = None
            for M in (Mf, Mf + 1, Mf + 130, Mf + 383):
                o32 = torch.full((Mmax, N), float("nan"), device="cuda") if c32 else None
                o16 = torch.full((Mmax, N), float("nan"), device="cuda", dtype=torch.float16) if c16 else None
                if use_res:
                    o32 = res.clone() if c32 else None
                d = lib.GemmDesc()
                d.dtype, d.M, d.N, d.K, d.batch, d.lo_scale = 0, M, N, K, 1, 1.0
                d.A, d.lda, d.B, d.ldb = a.data_ptr(), K, b.data_ptr(), K
                if c32:
                    d.C32, d.ldc = o32.data_ptr(), N
                if c16:
                    d.C16, d.ldc16 = o16.data_ptr(), N
                if use_res:
                    d.res, d.ldres = (o32 if c32 else res).data_ptr(), N
                d.bias, d.act = bias.data_ptr(), act
                full = "true" if M % 384 == 0 else "false"
                assert lib.gemm_kernel_name(d) == f"gemm_nt_t384_kernel<0, {fl}, {full}, true>"
                lib.call("dvd_gemm_nt", d, lib.stream_ptr())
                got = [t[:Mf].clone() for t in (o32, o16) if t is not None]
                tails = [t[M:] for t in (o32, o16) if t is not None and not use_res]
                torch.cuda.synchronize()
                for t in tails:
                    assert bool(torch.isnan(t).all()), f"FL{fl} N={N} K={K} M={M}: rows past M written"
                if base is None:
                    base = got
                    assert all(bool(torch.isfinite(t).all()) for t in got)
                else:
                    for x, y in zip(base, got):
                        assert torch.equal(x, y), f"FL{fl} N={N} K={K}: M={M} (ragged) differs from M={Mf} (FULL)"


def _engine_docs(G, idx):
    keys = ("y512", "mask_cat", "mask_y512", "line_msk")
    ds = [synth.synth_document(d, G, 1234) for d in idx]
    return {k: torch.from_numpy(np.stack([d[k] for d in ds])) for k in keys}, keys


@pytest.mark.parametrize("G,docs,check", [(72, 4, (0, 3)), (288, 32, (0, 16, 31))], ids=["g72-4docs", "g288-32docs"])
def test_engine_batch_equals_single_where_the_batch_changes_the_gemm(G, docs, check):
    """G = 72: four documents run the FULL t384 instance, one document the ragged one.  G = 288 x 32 documents: the f16 FFN
    buffers (NT * 2048) and the DiT MLP buffer (4 NT * 1536) hold more than 2^31 elements, so every document past the first
    few is stored behind 64-bit offsets.  One evaluation with feat_mode 1 and one with feat_mode 2: the checked documents
    must have the bits they have alone."""
    from dvd_amd import schedule
    from dvd_amd.engine import Engine
    H = 2
    sd = synth.synth_state_dict(G, 7, blocks=[11])
    cond, keys = _engine_docs(G, range(docs))
    xT = torch.from_numpy(np.concatenate([synth.synth_noise(d, H, G, 1234) for d in range(docs)]))
    t1, t2 = schedule.embedded_time(900.0), schedule.embedded_time(400.0)
    eng = Engine(G, docs, H)
    eng.load_state_dict(sd)
    eng.prepare(*[cond[k].cuda() for k in keys])
    x = xT.cuda()
    zeros = torch.zeros(docs * H, 2, G, G, device="cuda")
    x0_a = eng.denoise(x, t1, 1, zeros, dither_step=0)[[h for d in check for h in (H * d, H * d + 1)]].cpu()
    flow = (torch.rand(docs * H, 2, G, G, generator=torch.Generator().manual_seed(5)) * 0.2 - 0.1).cuda()
    x0_b = eng.denoise(x, t2, 2, flow, dither_step=1)[[h for d in check for h in (H * d, H * d + 1)]].cpu()
    blob = eng.blob
    del eng, x, zeros
    torch.cuda.empty_cache()
    one = Engine(G, 1, H)
    one.bind_blob(blob)
    for j, d in enumerate(check):
        one.prepare(*[cond[k][d:d + 1].cuda() for k in keys])
        xs = xT[H * d:H * d + H].cuda()
        a = one.denoise(xs, t1, 1, torch.zeros(H, 2, G, G, device="cuda"), dither_step=0).cpu()
        b = one.denoise(xs, t2, 2, flow[H * d:H * d + H].contiguous(), dither_step=1).cpu()
        assert torch.equal(a, x0_a[H * j:H * j + H]), f"document {d}, feat_mode 1"
        assert torch.equal(b, x0_b[H * j:H * j + H]), f"document {d}, feat_mode 2"
    del one
    torch.cuda.empty_cache()
