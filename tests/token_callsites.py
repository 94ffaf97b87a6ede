"""Every launch of dvd_amd/csrc/engine.hip that is neither a GEMM nor attention, with the arguments the engine computes.

`calls(G, docs, hyp, feat_mode)` returns one `Call` per launch of one dvd_engine_prepare_docs, one dvd_engine_feat_nchw and one
dvd_engine_denoise_step (the dithering launches in front of enqueue_step, decoder layers and prepare groups included), in
engine order.  `Call.args` is the C argument list without the stream, by parameter name and in ABI order.  A pointer is a
`(buffer, byte offset)` pair or None (a null pointer); the buffer is a workspace buffer of plan() (256-byte aligned), a weight
tensor (16-byte aligned, dvd_engine_set_tensor), or one of the caller's tensors (x_t, init_flow, init_feat, x0_out, mask_y512,
line_msk, feat_out); the offset is the engine's own pointer arithmetic.  The CPU test (test_token_dispatch.py) checks the table
against engine.hip and the entry points' preconditions; the GPU test (test_gpu_token_callsites.py) gives every buffer a real
allocation and launches the record.

Keep this table in step with engine.hip: test_token_dispatch.py matches the `TRY(dvd_...(` lines against SITES.
"""
from __future__ import annotations

from dataclasses import dataclass, field

from gemm_callsites import DEC, FFN, HID, RK, prepare_group_size

COLCHUNKS = 64
PYR_CIN = (4, 64, 64, 128, 128, 256, 256)
PYR_COUT = (64, 64, 128, 128, 256, 256, 256)
PYR_LAYERS = ((0, 512, False), (1, 512, True), (2, 256, False), (3, 256, True), (4, 128, False), (5, 128, False),
              (6, 128, True))                       # (layer, height = width, followed by a 2x2 max-pool)


def pyr_kpad(i):
    return (9 * PYR_CIN[i] + 63) // 64 * 64


# one entry per `TRY(dvd_<kernel>(` line of engine.hip, in source order: (site id, kernel, engine function)
SITES = [
    ("pyr_conv", "conv3x3_nhwc", "prepare"), ("pyr_im2col", "im2col3x3", "prepare"), ("pyr_pool", "maxpool2_nhwc", "prepare"),
    ("feat_resize", "resize_bilinear_nhwc", "prepare"), ("patch_rows", "patch_rows", "prepare"),
    ("feat_nchw", "nhwc_to_nchw", "feat_nchw"),
    ("t_embed0", "small_linear", "step"), ("t_embed2", "small_linear", "step"), ("ada", "small_linear", "step"),
    ("fin_ada", "small_linear", "step"), ("embed_obs", "embed_obs_ln", "step"), ("r_rows", "build_r_rows", "step"),
    ("ln_attn", "layernorm_rows", "step"), ("ln_mlp", "layernorm_rows", "step"), ("colmean", "colmean", "step"),
    ("pe_h0", "small_linear", "step"), ("pe_h2", "small_linear", "step"), ("pe_w0", "small_linear", "step"),
    ("pe_w2", "small_linear", "step"), ("posenc", "posenc_add", "step"), ("dec_ln1", "layernorm_rows", "step"),
    ("dec_ln2", "layernorm_rows", "step"), ("dec_dw", "dwconv3x3", "step"), ("final", "final_tokens", "step"),
    ("dither", "dither_f16", "denoise"),
]
KERNEL_OF = {s: k for s, k, _ in SITES}

# parameter names of the C entry points (include/dvd_hip.h), stream left out
PARAMS = {
    "conv3x3_nhwc": ("in", "c", "wgt", "kp", "bias", "out", "cout", "h", "w", "relu"),
    "im2col3x3": ("in", "sc", "sy", "sx", "out", "ldo", "c", "h", "w"),
    "maxpool2_nhwc": ("in", "out", "c", "h", "w"),
    "resize_bilinear_nhwc": ("in", "out", "c", "hin", "win", "hout", "wout"),
    "patch_rows": ("in", "sn", "sc", "sy", "sx", "out", "ldo", "n", "c", "g"),
    "nhwc_to_nchw": ("in", "out", "c", "h", "w"),
    "small_linear": ("x", "ldx", "w", "b", "y", "ldy", "m", "k", "n", "kmod", "act_in", "act_out"),
    "embed_obs_ln": ("x", "w", "bias", "pos", "tok32", "ln16", "n", "g"),
    "build_r_rows": ("feat", "init_feat", "flow", "out16", "ldo", "n", "g", "n_hyp", "mode"),
    "layernorm_rows": ("in", "ldin", "stride_in", "out16", "ldout", "stride_out", "batch", "rows", "c", "gamma", "beta",
                       "shift", "scale", "ldmod", "mod_rows", "eps"),
    "colmean": ("z", "partial", "pooled", "n", "t", "c", "chunks"),
    "posenc_add": ("z", "hs", "ws", "htab", "wtab", "n", "side", "c"),
    "dwconv3x3": ("in16", "out16", "w9c", "b", "n", "side", "c"),
    "final_tokens": ("z", "gamma", "beta", "shift", "scale", "ldmod", "mod_rows", "w8", "b8", "init_flow", "x0", "tok8",
                     "n", "g"),
    "dither_f16": ("hi", "lo", "out", "nelem", "elem0", "step"),
}
# which parameters are pointers, and the element size behind each
POINTERS = {
    "conv3x3_nhwc": {"in": 4, "wgt": 4, "bias": 4, "out": 4},
    "im2col3x3": {"in": 4, "out": 4},
    "maxpool2_nhwc": {"in": 4, "out": 4},
    "resize_bilinear_nhwc": {"in": 4, "out": 4},
    "patch_rows": {"in": 4, "out": 4},
    "nhwc_to_nchw": {"in": 4, "out": 4},
    "small_linear": {"x": 4, "w": 4, "b": 4, "y": 4},
    "embed_obs_ln": {"x": 4, "w": 4, "bias": 4, "pos": 4, "tok32": 4, "ln16": 2},
    "build_r_rows": {"feat": 4, "init_feat": 4, "flow": 4, "out16": 2},
    "layernorm_rows": {"in": 4, "out16": 2, "gamma": 4, "beta": 4, "shift": 4, "scale": 4},
    "colmean": {"z": 4, "partial": 4, "pooled": 4},
    "posenc_add": {"z": 4, "hs": 4, "ws": 4, "htab": 4, "wtab": 4},
    "dwconv3x3": {"in16": 2, "out16": 2, "w9c": 4, "b": 4},
    "final_tokens": {"z": 4, "gamma": 4, "beta": 4, "shift": 4, "scale": 4, "w8": 4, "b8": 4, "init_flow": 4, "x0": 4,
                     "tok8": 4},
    "dither_f16": {"hi": 2, "lo": 2, "out": 2},
}


@dataclass
class Call:
    site: str
    kernel: str
    args: dict
    note: dict = field(default_factory=dict)

    def pointers(self):
        return {p: self.args[p] for p in POINTERS[self.kernel]}

    def extents(self):
        """Per non-null pointer parameter: elements from the pointer to one past the last one the launch may touch."""
        a, k = self.args, self.kernel
        if k == "conv3x3_nhwc":
            e = {"in": a["h"] * a["w"] * a["c"], "wgt": a["cout"] * a["kp"], "bias": a["cout"],
                 "out": a["h"] * a["w"] * a["cout"]}
        elif k == "im2col3x3":
            e = {"in": (a["c"] - 1) * a["sc"] + (a["h"] - 1) * a["sy"] + (a["w"] - 1) * a["sx"] + 1,
                 "out": a["h"] * a["w"] * a["ldo"]}
        elif k == "maxpool2_nhwc":
            e = {"in": a["h"] * a["w"] * a["c"], "out": (a["h"] // 2) * (a["w"] // 2) * a["c"]}
        elif k == "resize_bilinear_nhwc":
            e = {"in": a["hin"] * a["win"] * a["c"], "out": a["hout"] * a["wout"] * a["c"]}
        elif k == "patch_rows":
            T = (a["g"] // 2) ** 2
            e = {"in": (a["n"] - 1) * a["sn"] + (a["c"] - 1) * a["sc"] + (a["g"] - 1) * (a["sy"] + a["sx"]) + 1,
                 "out": (a["n"] * T - 1) * a["ldo"] + 4 * a["c"]}
        elif k == "nhwc_to_nchw":
            e = {"in": a["h"] * a["w"] * a["c"], "out": a["h"] * a["w"] * a["c"]}
        elif k == "small_linear":
            e = {"x": (a["m"] - 1) * a["ldx"] + (1 if a["act_in"] == 2 else min(a["k"], a["kmod"])),
                 "w": a["n"] * a["k"], "b": a["n"], "y": (a["m"] - 1) * a["ldy"] + a["n"]}
        elif k == "embed_obs_ln":
            T = (a["g"] // 2) ** 2
            e = {"x": a["n"] * 2 * a["g"] ** 2, "w": HID * 8, "bias": HID, "pos": T * HID, "tok32": a["n"] * T * HID,
                 "ln16": a["n"] * T * HID}
        elif k == "build_r_rows":
            T = (a["g"] // 2) ** 2
            e = {"feat": ((a["n"] - 1) // a["n_hyp"] + 1) * a["g"] ** 2 * 256, "init_feat": a["n"] * 256 * a["g"] ** 2,
                 "flow": a["n"] * 2 * a["g"] ** 2, "out16": a["n"] * T * a["ldo"]}
        elif k == "layernorm_rows":
            mod = ((a["rows"] - 1) // a["mod_rows"]) * a["ldmod"] + a["c"]
            e = {"in": (a["batch"] - 1) * a["stride_in"] + (a["rows"] - 1) * a["ldin"] + a["c"],
                 "out16": (a["batch"] - 1) * a["stride_out"] + (a["rows"] - 1) * a["ldout"] + a["c"],
                 "gamma": a["c"], "beta": a["c"], "shift": mod, "scale": mod}
        elif k == "colmean":
            e = {"z": a["n"] * a["t"] * a["c"], "partial": a["n"] * a["chunks"] * a["c"], "pooled": a["n"] * a["c"]}
        elif k == "posenc_add":
            e = {"z": a["n"] * a["side"] ** 2 * a["c"], "hs": a["n"] * a["c"], "ws": a["n"] * a["c"],
                 "htab": a["side"] * a["c"], "wtab": a["side"] * a["c"]}
        elif k == "dwconv3x3":
            tok = a["n"] * a["side"] ** 2 * a["c"]
            e = {"in16": tok, "out16": tok, "w9c": 9 * a["c"], "b": a["c"]}
        elif k == "final_tokens":
            T = (a["g"] // 2) ** 2
            mod = ((a["n"] * T - 1) // a["mod_rows"]) * a["ldmod"] + DEC
            e = {"z": a["n"] * T * DEC, "gamma": DEC, "beta": DEC, "shift": mod, "scale": mod, "w8": 8 * DEC, "b8": 8,
                 "init_flow": a["n"] * 2 * a["g"] ** 2, "x0": a["n"] * 2 * a["g"] ** 2, "tok8": a["n"] * T * 8}
        elif k == "dither_f16":
            e = {"hi": a["nelem"], "lo": a["nelem"], "out": a["nelem"]}
        else:
            raise KeyError(k)
        return {p: n for p, n in e.items() if a[p] is not None}


def _rup(x, a=256):
    return (x + a - 1) // a * a


def wide_weights():
    """tensor_specs(): the f16 weights with a dithered copy, in spec order, with their element counts."""
    v = [("ca_wv16", HID * HID), ("sa_wqk16", 2 * HID * HID), ("sa_wv16", HID * HID), ("fc1_w16", 4 * HID * HID)]
    for j in range(6):
        p = f"d{j}_"
        v += [(p + "wqk16", 2 * DEC * DEC), (p + "wv16", DEC * DEC), (p + "wfc16", DEC * DEC), (p + "c1w16", FFN * DEC),
              (p + "c2w16", DEC * FFN)]
    return v


def dither_offsets():
    """plan(): element offset of every wide weight's copy inside w16dith, and the buffer's element count."""
    off, total = {}, 0
    for name, nelem in wide_weights():
        off[name] = total
        total += (nelem + 127) // 128 * 128
    return off, total


def workspace_bytes(G, docs, hyp):
    """plan(): byte size of every workspace buffer (rounded up to 256 as `add` does)."""
    T = (G // 2) ** 2
    N = docs * hyp
    NT = N * T
    b = {"feat": docs * G * G * 256 * 4, "tbuf": 256, "th": HID * 4, "cvec": HID * 4, "mod": 6 * HID * 4,
         "finmod": 2 * DEC * 4, "pooled": N * DEC * 4, "petmp": N * DEC * 4, "hs": N * DEC * 4, "wsc": N * DEC * 4,
         "part": N * COLCHUNKS * DEC * 4, "w16dith": dither_offsets()[1] * 2,
         "xtok32": NT * HID * 4, "xq16": NT * HID * 2, "arows16": NT * RK * 2, "z": NT * DEC * 4, "h16": NT * DEC * 2,
         "mlp16": NT * 4 * DEC * 2,
         "p_cat4": 4 * 512 * 512 * 4, "p_col": 512 * 512 * 576 * 4, "p_actA": 512 * 512 * 64 * 4,
         "p_actB": 512 * 512 * 64 * 4, "p_rows": T * 1536 * 4, "p_tok32": T * HID * 4}
    return {k: _rup(v) for k, v in b.items()}


def calls(G, docs, hyp, feat_mode=1, dither_step=0):
    """The engine's token-side launches with its default options (dither on large grids)."""
    side = G // 2
    T = side * side
    N = docs * hyp
    NT = T * N
    dither = T > 1024                                  # dvd_engine_create: small_tiles = T <= 1024, dither = !small_tiles
    W = lambda w: (w, 0)                               # noqa: E731  (Engine::F)
    out = []

    def add(site, note=None, **kw):
        k = KERNEL_OF[site]
        assert tuple(kw) == PARAMS[k], (site, tuple(kw), PARAMS[k])
        out.append(Call(site=site, kernel=k, args=dict(kw), note=note or {}))

    # ---- dvd_engine_prepare_docs ----
    for d in range(docs):
        cur, sc, sy, sx = ("p_cat4", 0), 512 * 512, 512, 1          # the first layer reads the planar cat([y512, mask_cat])
        act = (("p_actA", 0), ("p_actB", 0))
        wi = 0
        for idx, hw, pool in PYR_LAYERS:
            cin, cout, kp = PYR_CIN[idx], PYR_COUT[idx], pyr_kpad(idx)
            outp = act[wi]
            wi ^= 1
            if sc == 1 and cin % 16 == 0 and kp == 9 * cin:
                add("pyr_conv", {"doc": d, "layer": idx}, **{"in": cur}, c=cin, wgt=W(f"pyr{idx}_w"), kp=kp,
                    bias=W(f"pyr{idx}_b"), out=outp, cout=cout, h=hw, w=hw, relu=1)
            else:
                add("pyr_im2col", {"doc": d, "layer": idx}, **{"in": cur}, sc=sc, sy=sy, sx=sx, out=("p_col", 0), ldo=kp,
                    c=cin, h=hw, w=hw)                              # ... followed by the pyr_conv0 GEMM (gemm_callsites.py)
            if pool:
                add("pyr_pool", {"doc": d, "layer": idx}, **{"in": outp}, out=act[wi], c=cout, h=hw, w=hw)
                outp = act[wi]
                wi ^= 1
                hw //= 2
            cur, sc, sy, sx = outp, 1, hw * cout, cout
        if G != 64:                                                  # G == 64: a device copy
            add("feat_resize", {"doc": d}, **{"in": cur}, out=("feat", d * G * G * 256 * 4), c=256, hin=64, win=64, hout=G,
                wout=G)
    gmax = prepare_group_size(G, docs)
    for d0 in range(0, docs, gmax):
        gd = min(gmax, docs - d0)
        for name, src, sn, sc, sy, sx, c in (("c", ("feat", d0 * G * G * 256 * 4), G * G * 256, 1, G * 256, 256, 256),
                                             ("m", ("mask_y512", d0 * 384 * G * G * 4), 384 * G * G, G * G, G, 1, 384),
                                             ("l", ("line_msk", d0 * 64 * G * G * 4), 64 * G * G, G * G, G, 1, 64)):
            add("patch_rows", {"stream": name, "group": d0}, **{"in": src}, sn=sn, sc=sc, sy=sy, sx=sx, out=("p_col", 0),
                ldo=4 * c, n=gd, c=c, g=G)

    # ---- dvd_engine_feat_nchw ----
    for d in range(docs):
        add("feat_nchw", {"doc": d}, **{"in": ("feat", d * G * G * 256 * 4)}, out=("feat_out", d * 256 * G * G * 4), c=256,
            h=G, w=G)

    # ---- dvd_engine_denoise_step: the dithered weight copies, then enqueue_step ----
    if dither:
        off, _ = dither_offsets()
        for name, nelem in wide_weights():
            add("dither", {"weight": name}, hi=W(name), lo=W(name + "_lo"), out=("w16dith", off[name] * 2), nelem=nelem,
                elem0=off[name], step=dither_step)
    add("t_embed0", x=("tbuf", 0), ldx=1, w=W("t_w0"), b=W("t_b0"), y=("th", 0), ldy=HID, m=1, k=256, n=HID, kmod=256,
        act_in=2, act_out=1)
    add("t_embed2", x=("th", 0), ldx=HID, w=W("t_w2"), b=W("t_b2"), y=("cvec", 0), ldy=HID, m=1, k=HID, n=HID, kmod=HID,
        act_in=0, act_out=0)
    add("ada", x=("cvec", 0), ldx=HID, w=W("ada_w"), b=W("ada_b"), y=("mod", 0), ldy=6 * HID, m=1, k=HID, n=6 * HID,
        kmod=HID, act_in=1, act_out=0)
    add("fin_ada", x=("cvec", 0), ldx=HID, w=W("fin_ada_w"), b=W("fin_ada_b"), y=("finmod", 0), ldy=2 * DEC, m=1, k=DEC,
        n=2 * DEC, kmod=HID, act_in=1, act_out=0)
    sh_a, sc_a, sh_m, sc_m = ("mod", 0), ("mod", HID * 4), ("mod", 3 * HID * 4), ("mod", 4 * HID * 4)
    add("embed_obs", x=("x_t", 0), w=W("obs_w"), bias=W("obs_b"), pos=W("pos"), tok32=("xtok32", 0), ln16=("xq16", 0), n=N,
        g=G)
    add("r_rows", feat=("feat", 0), init_feat=("init_feat", 0) if feat_mode == 3 else None, flow=("init_flow", 0),
        out16=("arows16", 0), ldo=RK, n=N, g=G, n_hyp=hyp, mode=feat_mode)
    for site, sh, sc in (("ln_attn", sh_a, sc_a), ("ln_mlp", sh_m, sc_m)):
        add(site, **{"in": ("z", 0)}, ldin=DEC, stride_in=HID, out16=("h16", 0), ldout=HID, stride_out=NT * HID, batch=4,
            rows=NT, c=HID, gamma=None, beta=None, shift=sh, scale=sc, ldmod=0, mod_rows=NT, eps=1e-6)
    add("colmean", z=("z", 0), partial=("part", 0), pooled=("pooled", 0), n=N, t=T, c=DEC, chunks=COLCHUNKS)
    for site, x, w, y, act in (("pe_h0", "pooled", "pe_h0", "petmp", 2), ("pe_h2", "petmp", "pe_h2", "hs", 3),
                               ("pe_w0", "pooled", "pe_w0", "petmp", 2), ("pe_w2", "petmp", "pe_w2", "wsc", 3)):
        add(site, x=(x, 0), ldx=DEC, w=W(w + "_w"), b=W(w + "_b"), y=(y, 0), ldy=DEC, m=N, k=DEC, n=DEC, kmod=DEC,
            act_in=0, act_out=act)
    add("posenc", z=("z", 0), hs=("hs", 0), ws=("wsc", 0), htab=W("pe_htab"), wtab=W("pe_wtab"), n=N, side=side, c=DEC)
    for j in range(6):
        p = f"d{j}_"
        for site, g, b in (("dec_ln1", "n1w", "n1b"), ("dec_ln2", "n2w", "n2b")):
            add(site, {"layer": j}, **{"in": ("z", 0)}, ldin=DEC, stride_in=0, out16=("h16", 0), ldout=DEC, stride_out=0,
                batch=1, rows=NT, c=DEC, gamma=W(p + g), beta=W(p + b), shift=None, scale=None, ldmod=0, mod_rows=1,
                eps=1e-5)
        add("dec_dw", {"layer": j}, in16=("mlp16", 0), out16=("mlp16", NT * FFN * 2), w9c=W(p + "dww"), b=W(p + "dwb"), n=N,
            side=side, c=FFN)
    add("final", z=("z", 0), gamma=W("dec_nw"), beta=W("dec_nb"), shift=("finmod", 0), scale=("finmod", DEC * 4), ldmod=0,
        mod_rows=NT, w8=W("fin_w"), b8=W("fin_b"), init_flow=("init_flow", 0), x0=("x0_out", 0), tok8=None, n=N, g=G)
    return out


def c_args(call, address):
    """The ctypes argument tuple of `call` without the stream; address((buffer, byte offset)) -> int."""
    import ctypes as C
    out = []
    for p in PARAMS[call.kernel]:
        v = call.args[p]
        if p in POINTERS[call.kernel]:
            out.append(None if v is None else C.c_void_p(address(v)))
        elif isinstance(v, float):
            out.append(C.c_float(v))
        else:
            out.append(v)
    return out
