"""The attention test model against itself (CPU only): the call-site table against engine.hip, the product kernel of every
site on seven grids, the two exact probes and the per-element bound on an f32 / f16 emulation of the tile loop, and - the
sensitivity check - five deliberately wrong variants OF THE EMULATION, each of which at least one of the three checks must
flag.  tests/test_gpu_attention_callsites.py runs the same probes and the same bound on the kernels."""
import os
import re

import pytest
import torch

from dvd_amd import lib

import attention_callsites as CS
import attention_model as AM

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GRIDS = (16, 32, 64, 72, 152, 160, 288)


def test_table_covers_every_engine_attn_call():
    src = open(os.path.join(ROOT, "dvd_amd", "csrc", "engine.hip")).read()
    n = len(re.findall(r"TRY\(attn\(", src))
    assert n == len(CS.SITES), (
        f"engine.hip has {n} `TRY(attn(` lines, tests/attention_callsites.py describes {len(CS.SITES)}: add the new call to SITES "
        "and calls() there, its kernel to EXPECTED in this file and its form to tests/test_gpu_attention_callsites.py")
    got = [c.site for c in CS.calls(32, 1, 2)]
    assert got == [s for s, launches in CS.SITES for _ in range(launches)]


# the dispatch rule, written out: tk % 64 != 0 -> the register-staged kernel; else tq >= 5376 -> the generated kernel;
# else the LDS-DMA kernel.  T = (G / 2)^2 for every site (tq = tk = T).
EXPECTED = {
    16: ("flash_attn_glds_kernel<64, 0>", "flash_attn_glds_kernel<256, 0>"),           # T = 64
    32: ("flash_attn_glds_kernel<64, 0>", "flash_attn_glds_kernel<256, 0>"),           # 256
    64: ("flash_attn_glds_kernel<64, 0>", "flash_attn_glds_kernel<256, 0>"),           # 1024
    72: ("flash_attn_kernel<64>", "flash_attn_kernel<256>"),                           # 1296 = 20 * 64 + 16
    152: ("flash_attn_kernel<64>", "flash_attn_kernel<256>"),                          # 5776 = 90 * 64 + 16, although >= 5376
    160: ("flash_attn_h64x_kernel<0, true>", "flash_attn_r64x_kernel<0>"),             # 6400
    288: ("flash_attn_h64x_kernel<0, true>", "flash_attn_r64x_kernel<0>"),             # 20736
}


@pytest.mark.parametrize("G", GRIDS)
def test_product_kernel_of_every_site(G):
    T = (G // 2) ** 2
    for docs, hyp in ((1, 2), (3, 4)):                     # the batch never enters
        for c in CS.calls(G, docs, hyp):
            assert (c.tq, c.tk) == (T, T)
            name = lib.flash_attn_kernel_name(c.head_dim, c.tq, c.tk)
            assert name == EXPECTED[G][c.head_dim == 256], (G, c.site, name)
            assert name == AM.kernel_rule(c.head_dim, c.tq, c.tk) and name in AM.FAMILY


def test_kernel_rule_at_the_thresholds():
    for hd in (64, 256):
        for tq, tk in ((5375, 448), (5376, 448), (5377, 64), (1, 64), (5376, 72), (200, 8), (300, 512), (5500, 896)):
            assert lib.flash_attn_kernel_name(hd, tq, tk) == AM.kernel_rule(hd, tq, tk), (hd, tq, tk)


def test_call_forms():
    """What the GPU test relies on: kv_div = hyp on the three document streams, batch 4N and interleaved Q / K on the
    self-attention, head_dim 256 and interleaved Q / K on the decoder, the output slabs back to back inside att16."""
    G, docs, hyp = 32, 2, 3
    T, N = 256, 6
    cs = CS.calls(G, docs, hyp)
    doc = [c for c in cs if c.site == "ca_doc"]
    assert [c.kv_div for c in doc] == [hyp] * 3 and [c.O[1] for c in doc] == [s * N * T * 384 for s in range(3)]
    r, = [c for c in cs if c.site == "ca_r"]
    assert r.kv_div == 1 and r.O == ("att16", 3 * N * T * 384) and r.O[1] + CS.extent(r, "O") == CS.att16_elements(G, docs, hyp)
    sa, = [c for c in cs if c.site == "sa"]
    assert sa.batch == 4 * N and sa.Q[0] == sa.K[0] and sa.K[1] == 384 and sa.ldq == sa.ldk == 768 and sa.sQ == 2 * T * 384
    dec = [c for c in cs if c.site == "dec"]
    assert len(dec) == 6 and all(c.head_dim == 256 and c.K == ("qk16", 1536) and c.ldq == 3072 and c.ldo == 1536 for c in dec)
    for c in cs:
        assert c.O[1] + CS.extent(c, "O") <= CS.att16_elements(G, docs, hyp)


# ---- probes on the emulation ----------------------------------------------------------------------------------------
TKS = (64, 192, 448, 896, 1000)


def models_for(hd, tk):
    """Every model of this head_dim whose kernel takes this key count (ragged tk: the 64-key loops with f32 and f16 row sums)."""
    return [n for n in AM.MODELS if AM.HEAD_DIM[n] == hd and (tk % 64 == 0 or "flash_attn_kernel" in n or "plain" in n)]


def test_models_for():
    assert models_for(64, 1000) == ["flash_attn_kernel<64>", "plain<64>, l from f16"]
    assert set(models_for(256, 64)) == {"flash_attn_kernel<256>", "flash_attn_glds_kernel<256, 0>", "flash_attn_r64x_kernel<0>",
                                        "plain<256>, l from f16"}
    assert sorted(AM.HEAD_DIM[n] for n in AM.FAMILY) == [64, 64, 64, 256, 256, 256]


@pytest.mark.parametrize("hd", [64, 256])
@pytest.mark.parametrize("tk", TKS)
def test_probes_are_exact_on_the_emulation(hd, tk):
    sel = AM.selector_probe(2, 1, 150, tk, 2, hd, seed=tk + hd)
    cen = AM.census_probe(2, 1, 70, tk, 2, hd, seed=tk + hd)
    assert sel["gap"] >= 45.0
    if tk <= 150:
        assert all(len(torch.unique(sel["pi"][b, h])) == tk for b in range(2) for h in range(2))       # onto the keys
    for model in models_for(hd, tk):
        out = AM.emulate_all(sel, model)
        assert torch.equal(out.view(torch.int16), sel["want"].view(torch.int16)), (model, "selector")
        ok, ulps = AM.census_ok(AM.emulate_all(cen, model), cen)
        assert ok, (model, "census", ulps)


def test_selector_probe_beyond_4096_keys():
    """13 bits from 4097 keys on (the engine's smallest generated-kernel grid has 6400): the gap is still >= 45."""
    for hd in (64, 256):
        sel = AM.selector_probe(1, 1, 8, 6400, 1, hd, seed=3)
        assert sel["gap"] >= 45.0
        for model in models_for(hd, 6400):
            assert torch.equal(AM.emulate_all(sel, model), sel["want"]), model


# ---- the bound on the emulation -------------------------------------------------------------------------------------
def ref_matches(case):
    """ref() on a row subset equals the same rows of the whole, and the bound's own reference"""
    rows = torch.tensor([0, 7, 159])
    args = [case[n] for n in ("q", "k", "v", "heads", "hd", "scale", "kv_div")]
    whole, part = AM.ref(*args), AM.ref(*args, rows=rows)
    r, _ = AM.bound(*args, f"flash_attn_kernel<{case['hd']}>", rows=rows)
    return torch.equal(whole[:, rows], part) and float((r - part).abs().max()) < 1e-12


@pytest.mark.parametrize("amp", [1.0, 1.5, 3.0])
@pytest.mark.parametrize("model", list(AM.MODELS))
def test_bound_holds_and_is_not_slack(model, amp):
    """max err / bound over the elements lies in [0.1, 1]: the bound holds, and it is not loosened until it hides things."""
    hd = AM.HEAD_DIM[model]
    tk = 448 if model in ("flash_attn_r64x_kernel<0>", "flash_attn_h64x_kernel<0, true>") else 896
    case = AM.random_case(2, 1, 160, tk, 2, hd, amp, seed=int(10 * amp) + hd)
    assert ref_matches(case)
    out = AM.emulate_all(case, model)
    assert torch.isfinite(out).all()
    r, e, rk, ek = AM.bound(*[case[n] for n in ("q", "k", "v", "heads", "hd", "scale", "kv_div")], model, ideal=True)
    x, xk = float(((out.double() - r).abs() / e).max()), float(((out.double() - rk).abs() / ek).max())
    print(f"{model} amp {amp}: max err/bound {x:.3f} (around the kernel's own operands: {xk:.3f}), "
          f"median bound {float(e.median()):.2e}")
    assert 0.1 <= x <= 1.0 and 0.1 <= xk <= 1.0, (model, amp, x, xk)
    assert AM.MODELS[model]["prescale"] or (torch.equal(r, rk) and torch.equal(e, ek))


# ---- sensitivity: the emulation made wrong --------------------------------------------------------------------------
@pytest.mark.parametrize("model", list(AM.MODELS))
def test_every_mutation_is_flagged(model):
    """The unmutated emulation passes selector, census and bound; each of the five wrong variants fails at least one."""
    hd = AM.HEAD_DIM[model]
    tk = 448
    sel = AM.selector_probe(2, 1, 150, tk, 2, hd, seed=11)
    cen = AM.census_probe(2, 1, 70, tk, 2, hd, seed=12)
    case = AM.random_case(2, 1, 160, tk, 2, hd, 1.5, seed=13)
    r, e = AM.bound(*[case[n] for n in ("q", "k", "v", "heads", "hd", "scale", "kv_div")], model)

    def checks(mut):
        s = torch.equal(AM.emulate_all(sel, model, mutate=mut), sel["want"])
        c = AM.census_ok(AM.emulate_all(cen, model, mutate=mut), cen)[0]
        x = float(((AM.emulate_all(case, model, mutate=mut).double() - r).abs() / e).max())
        return s, c, x

    s, c, x = checks(None)
    assert s and c and x <= 1.0, (model, s, c, x)
    for mut in AM.MUTATIONS:
        s, c, x = checks(mut)
        print(f"{model} {mut}: selector {'pass' if s else 'FAIL'}, census {'pass' if c else 'FAIL'}, err/bound {x:.3g}")
        assert (not s) or (not c) or x > 1.0, (model, mut, "no check notices this mutation")
