"""Every gemm() call of dvd_amd/csrc/engine.hip as a dvd_gemm_desc, written out as the engine builds it.

`calls(G, docs, hyp)` returns one `Call` per launch of one dvd_engine_prepare_docs + one enqueue_step (decoder layers and
prepare groups included), in engine order.  Pointers are `(buffer, byte offset)` pairs: the buffer is a workspace buffer
of plan() (256-byte aligned, engine.hip `add`), a weight tensor (16-byte aligned, dvd_engine_set_tensor) or the dithered
copy of a wide weight (inside w16dith, 256-byte aligned); the offset is the engine's own pointer arithmetic.  The CPU test
(test_gemm_dispatch.py) gives each buffer a fabricated aligned address and asks dvd_gemm_kernel_name; the GPU test
(test_gpu_gemm_callsites.py) gives each one a real allocation and runs the descriptor.

Keep this table in step with engine.hip: test_gemm_dispatch.py counts the `TRY(gemm(` lines against SITES.
"""
from __future__ import annotations

from dataclasses import dataclass, field

HID, DEC, FFN, RK = 384, 1536, 2048, 1088          # engine.hip constants
PYR_CIN0, PYR_COUT0 = 4, 64                          # the pyramid's first layer: the only one on the im2col + GEMM route
PYR_KP0 = ((9 * PYR_CIN0 + 63) // 64) * 64

# one entry per `TRY(gemm(` line of engine.hip, in source order: (site id, engine function)
SITES = [
    ("pyr_conv0", "prepare"), ("patch_embed", "prepare"), ("ca_k32", "prepare"), ("ca_vt32", "prepare"),
    ("r_embed", "step"), ("ca_q", "step"), ("ca_k", "step"), ("ca_vt", "step"), ("ca_out", "step"),
    ("sa_qk", "step"), ("sa_vt", "step"), ("sa_proj", "step"), ("fc1", "step"), ("fc2", "step"),
    ("dec_qk", "step"), ("dec_vt", "step"), ("dec_fc", "step"), ("dec_conv1", "step"), ("dec_conv2", "step"),
]
WIDE = {"ca_wv16", "sa_wqk16", "sa_wv16", "fc1_w16", "wqk16", "wv16", "wfc16", "c1w16", "c2w16"}


@dataclass
class Call:
    site: str
    dtype: int
    M: int
    N: int
    K: int
    batch: int
    A: tuple
    lda: int
    sA: int
    B: tuple
    ldb: int
    sB: int
    C32: tuple = None
    ldc: int = 0
    sC32: int = 0
    C16: tuple = None
    ldc16: int = 0
    sC16: int = 0
    bias: tuple = None
    bias_row: int = 0
    act: int = 0
    pos: tuple = None
    pos_rows: int = 0
    gate: tuple = None
    gate_rows: int = 0
    res: tuple = None
    ldres: int = 0
    sRes: int = 0
    A_lo: tuple = None
    B_lo: tuple = None
    small_tiles: int = 0
    note: dict = field(default_factory=dict)

    @property
    def ldpos(self):
        return self.N                  # engine.hip Gemm(): ldpos = N

    @property
    def ldgate(self):
        return self.N                  # ldgate = N

    def esz(self):
        return 4 if self.dtype == 1 else 2


def _rup(x, a=256):
    return (x + a - 1) // a * a


def prepare_group_size(G, docs):
    """engine_prepare_docs: documents per patch-embedding group (the prepare scratch from p_col to the end of p_tok32)."""
    T = (G // 2) ** 2
    avail = (_rup(512 * 512 * 576 * 4) + 2 * _rup(512 * 512 * 64 * 4) + _rup(T * 1536 * 4) + _rup(T * HID * 4))
    per_doc = T * (1536 + HID) * 4
    return max(1, min(docs, avail // per_doc))


def calls(G, docs, hyp, split_weights=True, ffn_lo=True):
    """The engine's GEMM launches with its default options (dither on large grids, small_tiles from the grid)."""
    T = (G // 2) ** 2
    N = docs * hyp
    NT = T * N
    small = T <= 1024                     # dvd_engine_create
    dither = not small
    F16 = (3 if NT >= 16384 else 2) if small else 0      # enqueue_step's F16 code -> (dtype 0, small_tiles)
    F16S = 2

    def dt(code):
        return {0: (0, 0), 1: (1, 0), 2: (0, 1), 3: (0, 2)}[code]

    def H(w, wide=False):                 # Engine::W16(...).hi  (wide: TensorSpec::wide)
        return (("w16dith:" + w), 0) if (dither and wide) else (w, 0)

    def L(w, wide=False, ffn=False):      # Engine::W16(...).lo ((hi, lo) pairs are adjacent tensors)
        if ffn and not ffn_lo:
            return None
        return (w + "_lo", 0) if (split_weights and not (dither and wide)) else None

    W = lambda w: (w, 0)                  # noqa: E731  (Engine::F)
    out = []

    def add(site, code, **kw):
        d, st = dt(code)
        out.append(Call(site=site, dtype=d, small_tiles=st, **kw))

    # ---- dvd_engine_prepare_docs ----
    for _ in range(docs):
        add("pyr_conv0", 1, M=512 * 512, N=PYR_COUT0, K=PYR_KP0, batch=1, A=("p_col", 0), lda=PYR_KP0, sA=0,
            B=W("pyr0_w"), ldb=PYR_KP0, sB=0, C32=("p_actA", 0), ldc=PYR_COUT0, bias=W("pyr0_b"), act=2)
    gmax = prepare_group_size(G, docs)
    for d0 in range(0, docs, gmax):
        gd = min(gmax, docs - d0)
        tok_g = ("p_col", gd * T * 1536 * 4)
        for c, w, b, k16, vt16 in ((256, "c_w", "c_b", "kc16", "vtc16"), (384, "m_w", "m_b", "km16", "vtm16"),
                                   (64, "l_w", "l_b", "kl16", "vtl16")):
            K4 = 4 * c
            add("patch_embed", 1, M=gd * T, N=HID, K=K4, batch=1, A=("p_col", 0), lda=K4, sA=0, B=W(w), ldb=K4, sB=0,
                C32=tok_g, ldc=HID, bias=W(b), pos=W("pos"), pos_rows=T, note={"stream": w, "group": d0})
            add("ca_k32", 1, M=gd * T, N=HID, K=HID, batch=1, A=tok_g, lda=HID, sA=0, B=W("ca_wk32"), ldb=HID, sB=0,
                C16=(k16, d0 * T * HID * 2), ldc16=HID, bias=W("ca_bk"), note={"stream": w, "group": d0})
            add("ca_vt32", 1, M=HID, N=T, K=HID, batch=gd, A=W("ca_wv32"), lda=HID, sA=0, B=tok_g, ldb=HID, sB=T * HID,
                C16=(vt16, d0 * T * HID * 2), ldc16=T, sC16=T * HID, bias=W("ca_bv"), bias_row=1,
                note={"stream": w, "group": d0})

    # ---- enqueue_step ----
    g_a, g_m = ("mod", 2 * HID * 4), ("mod", 5 * HID * 4)
    add("r_embed", F16, M=NT, N=HID, K=RK, batch=1, A=("arows16", 0), lda=RK, sA=0, B=H("r_w16"), ldb=RK, sB=0,
        C16=("rtok16", 0), ldc16=HID, bias=W("r_b"), pos=W("pos"), pos_rows=T, B_lo=L("r_w16"))
    add("ca_q", F16, M=NT, N=HID, K=HID, batch=1, A=("xq16", 0), lda=HID, sA=0, B=H("ca_wq16"), ldb=HID, sB=0,
        C16=("q16", 0), ldc16=HID, bias=W("ca_bq"), B_lo=L("ca_wq16"))
    add("ca_k", F16, M=NT, N=HID, K=HID, batch=1, A=("rtok16", 0), lda=HID, sA=0, B=H("ca_wk16"), ldb=HID, sB=0,
        C16=("kr16", 0), ldc16=HID, bias=W("ca_bk"), B_lo=L("ca_wk16"))
    add("ca_vt", F16S, M=HID, N=T, K=HID, batch=N, A=H("ca_wv16", True), lda=HID, sA=0, B=("rtok16", 0), ldb=HID,
        sB=T * HID, C16=("vtr16", 0), ldc16=T, sC16=HID * T, bias=W("ca_bv"), bias_row=1, A_lo=L("ca_wv16", True))
    add("ca_out", F16, M=NT, N=HID, K=HID, batch=4, A=("att16", 0), lda=HID, sA=NT * HID, B=H("ca_wo16"), ldb=HID, sB=0,
        C32=("z", 0), ldc=DEC, sC32=HID, bias=W("ca_bo"), res=("xtok32", 0), ldres=HID, sRes=0, B_lo=L("ca_wo16"))
    add("sa_qk", F16, M=4 * NT, N=2 * HID, K=HID, batch=1, A=("h16", 0), lda=HID, sA=0, B=H("sa_wqk16", True), ldb=HID,
        sB=0, C16=("qk16", 0), ldc16=2 * HID, bias=W("sa_bqk"), B_lo=L("sa_wqk16", True))
    add("sa_vt", F16S, M=HID, N=T, K=HID, batch=4 * N, A=H("sa_wv16", True), lda=HID, sA=0, B=("h16", 0), ldb=HID,
        sB=T * HID, C16=("vt16", 0), ldc16=T, sC16=HID * T, bias=W("sa_bv"), bias_row=1, A_lo=L("sa_wv16", True))
    add("sa_proj", F16, M=NT, N=HID, K=HID, batch=4, A=("att16", 0), lda=HID, sA=NT * HID, B=H("sa_wp16"), ldb=HID,
        sB=0, C32=("z", 0), ldc=DEC, sC32=HID, bias=W("sa_bp"), gate=g_a, gate_rows=NT, res=("z", 0), ldres=DEC,
        sRes=HID, B_lo=L("sa_wp16"))
    add("fc1", F16, M=4 * NT, N=4 * HID, K=HID, batch=1, A=("h16", 0), lda=HID, sA=0, B=H("fc1_w16", True), ldb=HID,
        sB=0, C16=("mlp16", 0), ldc16=4 * HID, bias=W("fc1_b"), act=1, B_lo=L("fc1_w16", True))
    add("fc2", F16, M=NT, N=HID, K=4 * HID, batch=4, A=("mlp16", 0), lda=4 * HID, sA=NT * 4 * HID, B=H("fc2_w16"),
        ldb=4 * HID, sB=0, C32=("z", 0), ldc=DEC, sC32=HID, bias=W("fc2_b"), gate=g_m, gate_rows=NT, res=("z", 0),
        ldres=DEC, sRes=HID, B_lo=L("fc2_w16"))
    f1, f2 = ("mlp16", 0), ("mlp16", NT * FFN * 2)
    for j in range(6):
        p = f"d{j}_"
        add("dec_qk", F16, M=NT, N=2 * DEC, K=DEC, batch=1, A=("h16", 0), lda=DEC, sA=0, B=H(p + "wqk16", True), ldb=DEC,
            sB=0, C16=("qk16", 0), ldc16=2 * DEC, B_lo=L(p + "wqk16", True), note={"layer": j})
        add("dec_vt", F16, M=DEC, N=T, K=DEC, batch=N, A=H(p + "wv16", True), lda=DEC, sA=0, B=("h16", 0), ldb=DEC,
            sB=T * DEC, C16=("vt16", 0), ldc16=T, sC16=DEC * T, A_lo=L(p + "wv16", True), note={"layer": j})
        add("dec_fc", F16, M=NT, N=DEC, K=DEC, batch=1, A=("att16", 0), lda=DEC, sA=0, B=H(p + "wfc16", True), ldb=DEC,
            sB=0, C32=("z", 0), ldc=DEC, res=("z", 0), ldres=DEC, B_lo=L(p + "wfc16", True), note={"layer": j})
        add("dec_conv1", F16, M=NT, N=FFN, K=DEC, batch=1, A=("h16", 0), lda=DEC, sA=0, B=H(p + "c1w16", True), ldb=DEC,
            sB=0, C16=f1, ldc16=FFN, bias=W(p + "c1b"), act=2, B_lo=L(p + "c1w16", True, ffn=True), note={"layer": j})
        add("dec_conv2", F16, M=NT, N=DEC, K=FFN, batch=1, A=f2, lda=FFN, sA=0, B=H(p + "c2w16", True), ldb=FFN, sB=0,
            C32=("z", 0), ldc=DEC, bias=W(p + "c2b"), act=2, res=("z", 0), ldres=DEC, B_lo=L(p + "c2w16", True, ffn=True),
            note={"layer": j})
    return out


PTR_FIELDS = ("A", "B", "C32", "C16", "bias", "pos", "gate", "res", "A_lo", "B_lo")


def descriptor(call, address):
    """A dvd_amd.lib.GemmDesc for `call`, the engine's gemm() helper's way; address((buffer, byte offset)) -> int."""
    from dvd_amd import lib
    d = lib.GemmDesc()
    d.dtype, d.M, d.N, d.K, d.batch = call.dtype, call.M, call.N, call.K, call.batch
    d.lo_scale = 1.0
    d.lda, d.strideA, d.ldb, d.strideB = call.lda, call.sA, call.ldb, call.sB
    d.ldc, d.strideC32, d.ldc16, d.strideC16 = call.ldc, call.sC32, call.ldc16, call.sC16
    d.bias_row, d.act = call.bias_row, call.act
    d.ldpos, d.pos_rows = call.ldpos, call.pos_rows
    d.ldgate, d.gate_rows = call.ldgate, call.gate_rows
    d.ldres, d.strideRes = call.ldres, call.sRes
    d.small_tiles = call.small_tiles
    for f in PTR_FIELDS:
        v = getattr(call, f)
        setattr(d, f, None if v is None else address(v))
    return d
