"""The token-side launch table (tests/token_callsites.py) against engine.hip and against what the C entry points require
(CPU only: the records carry fabricated addresses of the engine's alignment)."""
import os
import re
from collections import Counter

import pytest

import token_callsites as TS

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SIZES = ((288, 1, 2), (288, 32, 2), (72, 4, 2), (64, 32, 2), (16, 5, 2))


def _engine_src():
    return open(os.path.join(ROOT, "dvd_amd", "csrc", "engine.hip")).read()


def launch_lines(src):
    """(kernel, engine function) of every `TRY(dvd_<kernel>(` line, in source order."""
    marks = [("prepare", src.index('extern "C" int dvd_engine_prepare_docs')),
             ("feat_nchw", src.index('extern "C" int dvd_engine_feat_nchw')),
             ("step", src.index("static int enqueue_step")),
             ("denoise", src.index('extern "C" int dvd_engine_denoise_step'))]
    out = []
    for m in re.finditer(r"TRY\(dvd_(\w+)\(", src):
        assert m.start() > marks[0][1], "a token-side launch in front of dvd_engine_prepare_docs"
        fn = [name for name, at in marks if at < m.start()][-1]
        out.append((m.group(1), fn))
    return out


def test_sites_follow_engine_source():
    """One SITES entry per `TRY(dvd_...(` line, same kernel, same engine function, same order: an engine edit that adds,
    drops or moves a token-side launch fails here until the table follows."""
    got = launch_lines(_engine_src())
    want = [(k, fn) for _, k, fn in TS.SITES]
    assert got == want, [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w] or (len(got), len(want))
    assert len(TS.SITES) == 25 and len({s for s, _, _ in TS.SITES}) == 25


def test_launch_line_scan_sees_a_dropped_and_a_moved_launch():
    """The scan itself: deleting one launch line or swapping two makes the comparison fail."""
    src = _engine_src()
    want = [(k, fn) for _, k, fn in TS.SITES]
    line = next(ln for ln in src.splitlines() if "TRY(dvd_colmean(" in ln)
    assert launch_lines(src.replace(line, "")) != want
    a = next(ln for ln in src.splitlines() if "TRY(dvd_embed_obs_ln(" in ln)
    b = next(ln for ln in src.splitlines() if "TRY(dvd_posenc_add(" in ln)
    swapped = src.replace(a, "@@").replace(b, a).replace("@@", b)
    assert launch_lines(swapped) != want


def test_calls_are_in_engine_order_with_the_engine_counts():
    # execution order: the first layer's im2col runs before the other layers' implicit convs, the dithering launches
    # before enqueue_step; everything else is source order
    order = ["pyr_im2col", "pyr_conv", "pyr_pool", "feat_resize", "patch_rows", "feat_nchw", "dither", "t_embed0",
             "t_embed2", "ada", "fin_ada", "embed_obs", "r_rows", "ln_attn", "ln_mlp", "colmean", "pe_h0", "pe_h2", "pe_w0",
             "pe_w2", "posenc", "dec_ln1", "dec_ln2", "dec_dw", "final"]
    assert sorted(order) == sorted(s for s, _, _ in TS.SITES)
    for G, docs, hyp in SIZES:
        cs = TS.calls(G, docs, hyp)
        first = list(dict.fromkeys(c.site for c in cs))
        expect = [s for s in order if not (s == "feat_resize" and G == 64) and not (s == "dither" and (G // 2) ** 2 <= 1024)]
        assert first == expect, (G, first)
        n = Counter(c.kernel for c in cs)
        groups = -(-docs // TS.prepare_group_size(G, docs))
        assert n["im2col3x3"] == docs and n["conv3x3_nhwc"] == 6 * docs and n["maxpool2_nhwc"] == 3 * docs
        assert n["resize_bilinear_nhwc"] == (0 if G == 64 else docs) and n["patch_rows"] == 3 * groups
        assert n["nhwc_to_nchw"] == docs and n["small_linear"] == 8 and n["layernorm_rows"] == 2 + 12
        assert n["embed_obs_ln"] == n["build_r_rows"] == n["colmean"] == n["posenc_add"] == n["final_tokens"] == 1
        assert n["dwconv3x3"] == 6 and n["dither_f16"] == (34 if (G // 2) ** 2 > 1024 else 0)
        # per decoder layer: ln1, ln2, dw
        dec = [c.site for c in cs if c.site.startswith("dec_")]
        assert dec == ["dec_ln1", "dec_ln2", "dec_dw"] * 6


def fake_address(buffers):
    """Workspace buffers 256-byte aligned; weights and the caller's tensors 16 bytes past that (what set_tensor requires)."""
    ws = set(TS.workspace_bytes(16, 1, 1))

    def addr(p):
        buf, off = p
        if buf not in buffers:
            buffers[buf] = (1 << 40) + len(buffers) * (1 << 36) + (0 if buf in ws else 16)
        return buffers[buf] + off
    return addr


def check_preconditions(c, addr):
    """What the entry point DVD_REQUIREs, plus the alignment its kernel's vector accesses rely on."""
    a = c.args
    al = {p: (None if v is None else addr(v)) for p, v in c.pointers().items()}
    ok = lambda p, n: al[p] is None or al[p] % n == 0                     # noqa: E731
    k = c.kernel
    if k == "layernorm_rows":
        assert al["in"] and al["out16"] and a["c"] in (384, 1536)
        assert (a["gamma"] is None) == (a["beta"] is None) and (a["shift"] is None) == (a["scale"] is None)
        assert a["shift"] is None or a["mod_rows"] > 0
        assert a["rows"] > 0 and 0 < a["batch"] < 65536
        assert a["ldin"] % 4 == 0 and a["stride_in"] % 2 == 0 and a["ldout"] % 4 == 0 and a["stride_out"] % 2 == 0
        assert a["ldmod"] % 4 == 0 and ok("in", 16) and ok("out16", 8)
        assert all(ok(p, 16) for p in ("gamma", "beta", "shift", "scale"))
        # the kernel's own vector width: 8-byte loads at C = 384 (column slices), 16-byte loads at C = 1536
        v = 2 if a["c"] == 384 else 4
        assert (a["stride_in"] * 4) % (4 * v) == 0 and (a["ldin"] * 4) % (4 * v) == 0
        assert (a["stride_out"] * 2) % (2 * v) == 0 and (a["ldout"] * 2) % (2 * v) == 0
    elif k == "small_linear":
        assert al["x"] and al["w"] and al["y"] and min(a["m"], a["k"], a["n"], a["kmod"]) > 0
        assert 0 <= a["act_in"] <= 2 and 0 <= a["act_out"] <= 3 and -(-a["m"] // 8) < 65536
        assert a["ldy"] >= a["n"] and (a["act_in"] == 2 or a["ldx"] >= min(a["k"], a["kmod"]))
        assert a["act_in"] != 2 or a["kmod"] % 2 == 0
    elif k == "colmean":
        assert 0 < a["n"] < 65536 and a["t"] > 0 and a["c"] > 0 and 0 < a["chunks"] < 65536
    elif k == "posenc_add":
        assert a["n"] > 0 and a["side"] > 0 and a["c"] % 4 == 0 and all(ok(p, 16) for p in al)
    elif k == "dwconv3x3":
        assert a["n"] > 0 and a["side"] > 0 and a["c"] % 8 == 0 and all(ok(p, 16) for p in al)
        assert a["c"] % 512 == 0                                       # the strip kernel's rule on large maps
    elif k == "embed_obs_ln":
        assert a["n"] > 0 and a["g"] >= 2 and a["g"] % 2 == 0 and all(al.values())
    elif k == "build_r_rows":
        assert al["feat"] and al["flow"] and al["out16"] and a["ldo"] >= 1032 and a["n"] > 0 and a["g"] % 2 == 0
        assert a["n_hyp"] > 0 and 0 <= a["mode"] <= 3 and (a["mode"] != 3 or al["init_feat"])
        assert ok("feat", 16) and a["n"] % a["n_hyp"] == 0
    elif k == "final_tokens":
        assert all(al[p] for p in ("z", "gamma", "beta", "shift", "scale", "w8", "b8", "x0"))
        assert a["n"] > 0 and a["g"] % 2 == 0 and a["mod_rows"] > 0 and ok("z", 16)
    elif k == "patch_rows":
        assert al["in"] and al["out"] and a["n"] > 0 and a["c"] > 0 and a["g"] % 2 == 0 and a["ldo"] >= 4 * a["c"]
        assert a["n"] * (a["g"] // 2) ** 2 < 1 << 31
    elif k == "im2col3x3":
        assert al["in"] and al["out"] and a["c"] > 0 and a["h"] > 0 and a["w"] > 0 and a["ldo"] >= 9 * a["c"]
    elif k == "conv3x3_nhwc":
        assert all(al.values()) and a["c"] % 16 == 0 and a["cout"] > 0 and a["kp"] >= 9 * a["c"] and a["kp"] % 4 == 0
        assert ok("in", 16) and ok("wgt", 16)
    elif k == "maxpool2_nhwc":
        assert a["c"] % 4 == 0 and a["h"] % 2 == 0 and a["w"] % 2 == 0 and all(ok(p, 16) for p in al)
    elif k == "resize_bilinear_nhwc":
        assert a["c"] % 4 == 0 and min(a["hin"], a["win"], a["hout"], a["wout"]) > 0 and all(ok(p, 16) for p in al)
    elif k == "nhwc_to_nchw":
        assert al["in"] and al["out"]
    elif k == "dither_f16":
        assert a["nelem"] > 0 and a["nelem"] % 8 == 0 and all(ok(p, 16) for p in al) and 0 <= a["elem0"] < 1 << 32
    else:
        raise KeyError(k)


@pytest.mark.parametrize("G,docs,hyp", SIZES)
def test_every_record_meets_the_entry_points_preconditions(G, docs, hyp):
    ws = TS.workspace_bytes(G, docs, hyp)
    assert 4 * (G // 2) ** 2 * docs * hyp < 1 << 31                    # dvd_engine_denoise_step's own limit
    for mode in (0, 1, 2, 3):
        bufs = {}
        addr = fake_address(bufs)
        for c in TS.calls(G, docs, hyp, feat_mode=mode):
            check_preconditions(c, addr)
            # ... and every workspace pointer stays inside the buffer plan() sized for it (the prepare-time patch rows use
            # the scratch from p_col to the end of p_tok32 as one region: engine_prepare_docs checks that itself)
            for p, n in c.extents().items():
                buf, off = c.args[p]
                if buf in ws and not (c.kernel == "patch_rows" and p == "out"):
                    assert off + n * TS.POINTERS[c.kernel][p] <= ws[buf], (c.site, p, buf)
            if c.kernel == "patch_rows":
                T = (G // 2) ** 2
                avail = ws["p_col"] + ws["p_actA"] + ws["p_actB"] + ws["p_rows"] + ws["p_tok32"]
                assert c.args["n"] * T * (1536 + TS.HID) * 4 <= avail


def test_preconditions_check_bites():
    """check_preconditions is not vacuous: the batched LayerNorm with an odd slice stride, or a depthwise conv on 2040
    channels, is refused."""
    import dataclasses
    cs = {c.site: c for c in TS.calls(72, 1, 2)}
    for site, change in (("ln_attn", {"stride_in": 383}), ("ln_attn", {"ldout": 386}), ("dec_dw", {"c": 2040}),
                         ("dither", {"nelem": 1004}), ("colmean", {"chunks": 65536})):
        bad = dataclasses.replace(cs[site], args={**cs[site].args, **change})
        with pytest.raises(AssertionError):
            check_preconditions(bad, fake_address({}))
