"""Every attn() call of dvd_amd/csrc/engine.hip as a dvd_attn_desc, written out as the engine builds it.

`calls(G, docs, hyp)` returns one `Call` per launch of one enqueue_step, in engine order: the three cross-attentions of the
shared query against the documents' K / V^T (kv_batch_div = hyp), the cross-attention against r, the gated self-attention of
the four streams (batch 4N, Q and K the column halves of one [4N, T, 2C] projection) and the six decoder layers (head_dim
256, Q and K again the halves of one buffer).  Pointers are `(buffer, element offset)` pairs in f16 elements: the buffer is
a workspace buffer of plan(), the offset the engine's own pointer arithmetic (the output slab s * NT * HID inside att16,
the + HID / + DEC of the K half).

Keep this table in step with engine.hip: test_attention_model_cpu.py counts the `TRY(attn(` lines against SITES.
"""
from __future__ import annotations

from dataclasses import dataclass, field

HID, DEC, HEADS, DEC_LAYERS = 384, 1536, 6, 6        # engine.hip constants

# one entry per `TRY(attn(` line of engine.hip, in source order: (site id, launches per step)
SITES = [("ca_doc", 3), ("ca_r", 1), ("sa", 1), ("dec", DEC_LAYERS)]


@dataclass
class Call:
    site: str
    head_dim: int
    heads: int
    batch: int
    tq: int
    tk: int
    kv_div: int
    scale: float
    Q: tuple
    ldq: int
    sQ: int
    K: tuple
    ldk: int
    sK: int
    Vt: tuple
    ldvt: int
    sVt: int
    O: tuple
    ldo: int
    sO: int
    note: dict = field(default_factory=dict)

    @property
    def C(self):
        return self.heads * self.head_dim

    @property
    def kv_batch(self):
        return (self.batch + self.kv_div - 1) // self.kv_div


def calls(G, docs, hyp):
    T = (G // 2) ** 2
    N = docs * hyp
    NT = N * T
    TH, TD = T * HID, T * DEC
    out = []
    # streams cond, msk6, line against the documents' K / V^T (shared by a document's hypotheses), then r
    for s, (k16, vt16) in enumerate((("kc16", "vtc16"), ("km16", "vtm16"), ("kl16", "vtl16"))):
        out.append(Call("ca_doc", 64, HEADS, N, T, T, hyp, 0.125, Q=("q16", 0), ldq=HID, sQ=TH, K=(k16, 0), ldk=HID, sK=TH,
                        Vt=(vt16, 0), ldvt=T, sVt=TH, O=("att16", s * NT * HID), ldo=HID, sO=TH, note={"stream": s}))
    out.append(Call("ca_r", 64, HEADS, N, T, T, 1, 0.125, Q=("q16", 0), ldq=HID, sQ=TH, K=("kr16", 0), ldk=HID, sK=TH,
                    Vt=("vtr16", 0), ldvt=T, sVt=TH, O=("att16", 3 * NT * HID), ldo=HID, sO=TH, note={"stream": 3}))
    out.append(Call("sa", 64, HEADS, 4 * N, T, T, 1, 0.125, Q=("qk16", 0), ldq=2 * HID, sQ=2 * TH, K=("qk16", HID),
                    ldk=2 * HID, sK=2 * TH, Vt=("vt16", 0), ldvt=T, sVt=TH, O=("att16", 0), ldo=HID, sO=TH))
    for j in range(DEC_LAYERS):
        out.append(Call("dec", 256, HEADS, N, T, T, 1, 0.0625, Q=("qk16", 0), ldq=2 * DEC, sQ=2 * TD, K=("qk16", DEC),
                        ldk=2 * DEC, sK=2 * TD, Vt=("vt16", 0), ldvt=T, sVt=TD, O=("att16", 0), ldo=DEC, sO=TD,
                        note={"layer": j}))
    return out


def att16_elements(G, docs, hyp):
    """plan(): att16 holds the four cross-attention slabs [4, NT, HID] (= the self-attention's [4N, T, HID]
    = the decoder's [NT, DEC])."""
    return 4 * docs * hyp * (G // 2) ** 2 * HID


def extent(call, f):
    """Elements from the pointer to one past the last one the kernel may touch."""
    if f == "Q":
        return (call.batch - 1) * call.sQ + (call.tq - 1) * call.ldq + call.C
    if f == "K":
        return (call.kv_batch - 1) * call.sK + (call.tk - 1) * call.ldk + call.C
    if f == "Vt":
        return (call.kv_batch - 1) * call.sVt + (call.C - 1) * call.ldvt + call.tk
    if f == "O":
        return (call.batch - 1) * call.sO + (call.tq - 1) * call.ldo + call.C
    raise KeyError(f)


def descriptor(call, address):
    """A dvd_amd.lib.AttnDesc for `call`, engine.hip's Attn helper's way; address((buffer, element offset)) -> int."""
    from dvd_amd import lib
    d = lib.AttnDesc()
    d.head_dim, d.heads, d.batch, d.tq, d.tk, d.kv_batch_div = (call.head_dim, call.heads, call.batch, call.tq, call.tk,
                                                               call.kv_div)
    d.Q, d.ldq, d.strideQ = address(call.Q), call.ldq, call.sQ
    d.K, d.ldk, d.strideK = address(call.K), call.ldk, call.sK
    d.Vt, d.ldvt, d.strideVt = address(call.Vt), call.ldvt, call.sVt
    d.O, d.ldo, d.strideO = address(call.O), call.ldo, call.sO
    d.scale = call.scale
    return d
