"""CPU model of the flash-attention kernels (dvd_amd/csrc/attention.hip and its generated loops): a float64 reference, two
probes whose exact answer needs no reference, a per-element error bound read off the kernels' arithmetic, and an f32 / f16
emulation of the tile loop that can be made wrong on purpose (the project's kernels never are).

Layout everywhere: q [B, Tq, heads * hd], k and v [Bkv, Tk, heads * hd] (v NOT transposed), f16; query batch b reads the
K / V of batch b // kv_div.

What the six product kernels do differently (FAMILY; read off attention.hip, gen_attn_r64x.py and gen_attn_h64x.py):
  tile        keys per online-softmax step: 64 (flash_attn_kernel, flash_attn_glds_kernel), 32 (r64x, h64x)
  wave_rows   query rows that share one deferred-rescale decision (`__any` / vcc over the wave): 32 or 64
  prescale    head_dim 64 on the LDS-DMA kernels: Q is multiplied by c = scale * log2(e) in f32 and rounded to f16 ONCE, the
              scores come out of the MFMA as q' . k - m (-m rides in the C operand); the others form fma(s, c, -m) in f32
  pipelined   r64x / h64x: the rescale is decided on tile t + 1 while P(t) is already packed, and the rare block scales the
              packed P(t) in f16 by f16(alpha) (v_cvt_pk_f16_f32 + v_pk_mul_f16): two more f16 roundings on those keys
  l_from_f16  h64x<0, true>: the row sum is ones . P on the matrix pipe, i.e. the sum of the f16-rounded P
"""
from __future__ import annotations

import math

import torch

L2E = 1.4426950408889634
THR = 10.0                       # RESCALE_THR of every kernel (log2 units)

FAMILY = {
    "flash_attn_kernel<64>": dict(tile=64, wave_rows=32, prescale=False, pipelined=False, l_from_f16=False),
    "flash_attn_kernel<256>": dict(tile=64, wave_rows=32, prescale=False, pipelined=False, l_from_f16=False),
    "flash_attn_glds_kernel<64, 0>": dict(tile=64, wave_rows=32, prescale=True, pipelined=False, l_from_f16=False),
    "flash_attn_glds_kernel<256, 0>": dict(tile=64, wave_rows=32, prescale=False, pipelined=False, l_from_f16=False),
    "flash_attn_r64x_kernel<0>": dict(tile=32, wave_rows=64, prescale=False, pipelined=True, l_from_f16=False),
    "flash_attn_h64x_kernel<0, true>": dict(tile=32, wave_rows=64, prescale=True, pipelined=True, l_from_f16=True),
}
# the plain emulation with l taken from the f16 P (no product kernel of its own: h64x's row sum on the 64-key loop)
EMULATION_ONLY = {
    "plain<64>, l from f16": dict(FAMILY["flash_attn_kernel<64>"], l_from_f16=True),
    "plain<256>, l from f16": dict(FAMILY["flash_attn_kernel<256>"], l_from_f16=True),
}
MODELS = {**FAMILY, **EMULATION_ONLY}
HEAD_DIM = {n: (256 if "256" in n or "r64x" in n else 64) for n in MODELS}
MUTATIONS = ("vswap", "l_norescale", "dropkey", "dupl", "stale_tile")


def kernel_rule(hd, tq, tk):
    """The product library's choice, written out independently of attention.hip's attn_kernel()."""
    if tk % 64:
        return f"flash_attn_kernel<{hd}>"
    if tq >= 5376:
        return "flash_attn_r64x_kernel<0>" if hd == 256 else "flash_attn_h64x_kernel<0, true>"
    return f"flash_attn_glds_kernel<{hd}, 0>"


def c32(scale):
    """p.c as dvd_flash_attn computes it: an f32 product of the f32 scale and the f32 log2(e)."""
    return torch.tensor(scale, dtype=torch.float32) * torch.tensor(L2E, dtype=torch.float32)


def prescaled_q(q, scale):
    """Q * c in f32, one f16 rounding (flash_attn_glds_kernel<64>, h64x_load_q)."""
    return (q.float() * c32(scale)).half()


def _heads(t, heads, hd):
    return t.reshape(t.shape[0], t.shape[1], heads, hd).permute(0, 2, 1, 3)            # [B, heads, T, hd]


def ref(q, k, v, heads, hd, scale, kv_div, rows=None):
    """float64 softmax(Q K^T scale) V on the f16-rounded operands; `rows`: a 1-D index tensor of the query rows to compute."""
    if rows is not None:
        q = q[:, rows]
    qh, kh, vh = (_heads(t.double(), heads, hd) for t in (q, k, v))
    out = torch.empty(qh.shape, dtype=torch.float64)
    for b in range(qh.shape[0]):
        a = torch.softmax(qh[b] @ kh[b // kv_div].transpose(-1, -2) * scale, dim=-1)
        out[b] = a @ vh[b // kv_div]
    return out.permute(0, 2, 1, 3).reshape(q.shape[0], q.shape[1], heads * hd)


# ---------------------------------------------------------------------------------------------------------------------
# probes
# ---------------------------------------------------------------------------------------------------------------------
def _code(idx, nbits):
    return (((idx[..., None] >> torch.arange(nbits)) & 1) * 2 - 1).double()


def selector_probe(B, Bkv, tq, tk, heads, hd, seed, gap_rows=64):
    """Every query picks exactly one key.  K[j] = the +-1 binary code of j ^ mask (mask per (kv batch, head), so another
    head's or batch's K selects another key), `nbits` bits repeated `reps` times, the other dims 0; Q[i] = A code(pi(i) ^
    mask); pi a seeded map per (batch, head), onto the keys whenever tq >= tk.  12 bits x 5 (hd 64) or x 21 (hd 256) up
    to 4096 keys, 13 bits x 4 or x 19 above.  V is random f16 without zeros, per-column scales 2^-8 .. 2^4, per (kv batch,
    head).
    Returns q, k, v, want (= the gathered V rows, f16) and `gap`: the smallest lead of the winning score over any other,
    in log2 units - two distinct codes differ in >= 1 bit, i.e. by 2 A reps scale log2(e) - checked in float64 on the f16
    operands for `gap_rows` queries of every (batch, head) and asserted >= 45."""
    assert B % Bkv == 0 and hd in (64, 256)
    nbits = 12 if tk <= 4096 else 13
    assert tk <= 1 << nbits
    reps, A = (hd - 4) // nbits, (32.0 if hd == 64 else 16.0)
    scale = 1.0 / math.sqrt(hd)
    g = torch.Generator().manual_seed(seed)
    kv_div = B // Bkv
    C = heads * hd
    mask = torch.randint(0, 1 << nbits, (Bkv, heads), generator=g)
    # keys must stay distinct under the mask: j ^ mask is a bijection of [0, 2^nbits)
    q = torch.zeros(B, tq, C)
    k = torch.zeros(Bkv, tk, C)
    v = torch.empty(Bkv, tk, C)
    pi = torch.empty(B, heads, tq, dtype=torch.long)
    keys = torch.arange(tk)
    for kb in range(Bkv):
        for h in range(heads):
            k[kb, :, h * hd:h * hd + nbits * reps] = _code(keys ^ mask[kb, h], nbits).repeat(1, reps)
            colscale = torch.exp2(torch.randint(-8, 5, (hd,), generator=g).float())
            v[kb, :, h * hd:(h + 1) * hd] = torch.randn(tk, hd, generator=g) * colscale
    for b in range(B):
        for h in range(heads):
            if tq >= tk:
                p = torch.cat([torch.randperm(tk, generator=g), torch.randint(0, tk, (tq - tk,), generator=g)])
                p = p[torch.randperm(tq, generator=g)]
            else:
                p = torch.randperm(tk, generator=g)[:tq]
            pi[b, h] = p
            q[b, :, h * hd:h * hd + nbits * reps] = A * _code(p ^ mask[b // kv_div, h], nbits).repeat(1, reps)
    q, k, v = q.half(), k.half(), v.half()
    # no zeros of either sign: V + the other keys' shares (< 2^-30 in all; half of f16's finest spacing is 2^-25) must round
    # back to V, and a zero would take the sign of that remainder
    v[v == 0] = 2.0 ** -14
    want = torch.empty(B, tq, C, dtype=torch.float16)
    gap = math.inf
    rows = torch.linspace(0, tq - 1, min(tq, gap_rows)).long().unique()
    for b in range(B):
        for h in range(heads):
            hs = slice(h * hd, (h + 1) * hd)
            want[b, :, hs] = v[b // kv_div, pi[b, h], hs]
            if tk > 1:
                s = q[b, rows, hs].double() @ k[b // kv_div, :, hs].double().T * (scale * L2E)
                top = s.gather(1, pi[b, h, rows, None])
                s.scatter_(1, pi[b, h, rows, None], -math.inf)
                gap = min(gap, float((top[:, 0] - s.max(1).values).min()))
    assert gap >= 45.0, f"selector probe: the winner leads by {gap} log2 units only"
    return dict(q=q, k=k, v=v, want=want, pi=pi, gap=gap, scale=scale, kv_div=kv_div, heads=heads, hd=hd)


def census_probe(B, Bkv, tq, tk, heads, hd, seed):
    """Uniform weights: Q = 0, K random, V[j, d] = 1 if j % 64 == d % 64 else 0.  Every P is exactly 1, l exactly tk and every
    accumulator the count of keys j = d mod 64: for tk % 64 == 0 the output is f16(1 / 64) bit for bit (the 1 / l factor is off
    by <= 2^-24 relative, far below half an f16 ulp); for ragged tk it is count / tk (`want`, float64), within one f16 ulp."""
    assert B % Bkv == 0
    g = torch.Generator().manual_seed(seed)
    C = heads * hd
    q = torch.zeros(B, tq, C, dtype=torch.float16)
    k = torch.randn(Bkv, tk, C, generator=g).half()
    j, d = torch.arange(tk)[:, None], torch.arange(C)[None]
    v = ((j % 64) == (d % hd % 64)).half()[None].repeat(Bkv, 1, 1)
    want = (v[0].double().sum(0) / tk)[None, None].expand(B, tq, C)
    return dict(q=q, k=k, v=v, want=want, exact=tk % 64 == 0, scale=1.0 / math.sqrt(hd), kv_div=B // Bkv, heads=heads, hd=hd)


def f16_ulp(x):
    """The spacing of f16 at |x| (float64 tensor), 2^-24 in the subnormal range."""
    x = x.abs().clamp_min(2.0 ** -14)
    return torch.exp2(torch.floor(torch.log2(x)) - 10)


def census_ok(out, prob):
    """out [B, tq, C] f16 -> (passes, largest |out - want| in f16 ulps of want)."""
    want = prob["want"]
    if prob["exact"]:
        return bool(torch.equal(out, want.half())), float(((out.double() - want).abs() / f16_ulp(want)).max())
    err = ((out.double() - want).abs() / f16_ulp(want)).max()
    return bool(err <= 1.0), float(err)


def random_case(B, Bkv, tq, tk, heads, hd, amp, seed, planted=6, q=None):
    """The bound's test inputs: q, k ~ amp N(0, 1); v ~ N(0, 1) with per-column scales 2^-8 .. 2^4; `planted` dominant keys
    (k[j] = q[i] (3 + 2 n) / max(1, amp^2): one key takes the row, at rising margins, wherever it falls in the tile order).
    `q`: the queries of another case (the engine's cross-attentions share one Q)."""
    g = torch.Generator().manual_seed(seed)
    C = heads * hd
    q0 = (torch.randn(B, tq, C, generator=g) * amp).half()
    q = q0 if q is None else q
    k = (torch.randn(Bkv, tk, C, generator=g) * amp).half()
    v = (torch.randn(Bkv, tk, C, generator=g) * torch.exp2(torch.randint(-8, 5, (Bkv, 1, C), generator=g).float())).half()
    kv_div = B // Bkv
    for n in range(planted):
        b, i, j, h = (int(torch.randint(0, hi, (1,), generator=g)) for hi in (B, tq, tk, heads))
        hs = slice(h * hd, (h + 1) * hd)
        k[b // kv_div, j, hs] = (q[b, i, hs].float() * (3 + 2 * n) / max(1.0, amp * amp)).half()
    return dict(q=q, k=k, v=v, scale=1.0 / math.sqrt(hd), kv_div=kv_div, heads=heads, hd=hd)


# ---------------------------------------------------------------------------------------------------------------------
# the per-element bound
# ---------------------------------------------------------------------------------------------------------------------
def bound(q, k, v, heads, hd, scale, kv_div, kernel, rows=None, ideal=False):
    """(ref, bnd), both [B, R, C] float64: |kernel output - ref| <= bnd for every element, for the arithmetic of `kernel` (a key
    of MODELS).  With u = 2^-24 (f32 unit roundoff), per query i, key j, in log2 units:
      scores      f16 x f16 products are exact; f32 accumulation of hd terms in an unknown order: hd u sum_d |q_d k_d| c.
                  prescale kernels: the f16 rounding of q c is reproduced exactly (q'), the model's weights a and its ideal
                  output r' use q' . k, and |r' - ref| enters the bound as it is; the accumulation carries -m as well:
                  (hd + 1) u (sum_d |q'_d k_d| + |m|), |m| <= |row max| + THR
      argument    fma(s, c, -m) (or the rare block's s - delta): one rounding of a number of size <= |s c - max| + THR + 1
      c           f32(scale) f32(log2 e) rounded to f32: 2 u relative; only (s - s_max) c matters, a row's common shift cancels
                  (m itself is a common reference of P and l and cancels exactly, whatever its rounding)
      v_exp_f32   1 ulp; taken as 4 u relative
    -> eps_s(j) = ln 2 delta(j) + 4 u, common to P and l.  Then
      P -> f16    2^-11 relative (half an ulp; P in (0, 2^10] under the deferred rescale, no overflow), on the numerator and -
                  l_from_f16 - on l too.  A P below 2^-14 is subnormal: 2^-25 absolute instead; since l >= 1 (the reference
                  maximum is a row's own score), p_j >= a_ij, so only keys with a_ij < 2^-13 can be.
      pipelined   the rare block multiplies the packed P(t) by f16(alpha): 2 more f16 roundings, on the keys of a tile t
                  whose successor can raise the row's maximum: max(tile t + 1) > max(tiles <= t) - THR (a necessary condition:
                  m >= the running maximum - THR; alpha = 1 is exact).  The kernel decides on its computed scores, the
                  model on the float64 ones: both sides of the comparison are scores minus a reference, each within
                  max_j delta(j) of the model's, so the model widens the condition by 2 max_j delta(j) (some 1e-3)
      sums        f32 accumulation of tk terms and at most one rescale multiplication per tile: (tk + 2 tiles + 4) u on
                  sum_j a_ij |v_jd| (numerator) and on |out| (l)
      1 / l, o * inv   4 u |out|
      out -> f16  half an f16 ulp at |ref| + everything above (2^-25 in the subnormal range)
    The error of p_j enters as sum_j a_ij (eps_P(j) |v_jd| + eps_l(j) |out_id|).
    ideal=True returns (ref, bnd, r', bnd') instead: r' the float64 output of the kernel's own operands (q' for the prescale
    kernels, else r' = ref) and bnd' the bound around it, i.e. bnd without |r' - ref| - the sharper statement of the two."""
    fam = MODELS[kernel]
    u = 2.0 ** -24
    if rows is not None:
        q = q[:, rows]
    B, R, C = q.shape
    tk = k.shape[1]
    tile = fam["tile"]
    nt = (tk + tile - 1) // tile
    c = scale * L2E
    qh, kh, vh = (_heads(t.double(), heads, hd) for t in (q, k, v))
    qp = _heads(prescaled_q(q, scale).double(), heads, hd) if fam["prescale"] else None
    r_out = torch.empty(B, heads, R, hd, dtype=torch.float64)
    e_out, rk_out, ek_out = torch.empty_like(r_out), torch.empty_like(r_out), torch.empty_like(r_out)
    for b in range(B):
        for h in range(heads):
            K, V = kh[b // kv_div, h], vh[b // kv_div, h]
            absV = V.abs()
            s = qh[b, h] @ K.T * c
            r = torch.softmax(s * math.log(2), -1) @ V
            if fam["prescale"]:
                sk = qp[b, h] @ K.T
                absqk = qp[b, h].abs() @ K.abs().T
            else:
                sk, absqk = s, qh[b, h].abs() @ K.abs().T * c
            smax = sk.max(1, keepdim=True).values
            a = torch.softmax(sk * math.log(2), -1)
            rk = a @ V
            drift = (rk - r).abs()
            if fam["prescale"]:
                delta = (hd + 1) * u * (absqk + smax.abs() + THR)
            else:
                delta = hd * u * absqk + 2 * u * (sk - smax).abs()
            delta = delta + u * ((sk - smax).abs() + THR + 1)
            eps_s = math.log(2) * delta + 4 * u
            eps_p = torch.full_like(sk, 2.0 ** -11)
            if fam["pipelined"] and nt > 1:
                pad = nt * tile - tk
                M = torch.nn.functional.pad(sk, (0, pad), value=-math.inf).reshape(R, nt, tile).max(2).values
                run = torch.cummax(M, 1).values
                # the kernel compares its own f32 numbers: each side is off by at most the row's largest delta
                hit = M[:, 1:] > run[:, :-1] - THR - 2 * delta.max(1, keepdim=True).values
                hit = torch.cat([hit, torch.zeros(R, 1, dtype=torch.bool)], 1).repeat_interleave(tile, 1)[:, :tk]
                eps_p = eps_p + hit * (2 * 2.0 ** -11 * (1 + 2.0 ** -9))
            eps_P = eps_s + eps_p
            eps_l = eps_s + (eps_p if fam["l_from_f16"] else 0.0)
            small = (a < 2.0 ** -13).double() * (2.0 ** -25 * (2 if fam["pipelined"] else 1))
            gam = (tk + 2 * nt + 4) * u
            e = (a * (eps_P + gam) + small) @ absV               # the three numerator terms in one product
            e = e + ((a * eps_l).sum(1, keepdim=True) + gam + 4 * u) * rk.abs()
            if fam["l_from_f16"]:
                e = e + small.sum(1, keepdim=True) * rk.abs()
            e = e * (1 + 2.0 ** -8)                            # second-order terms of the products of the relative errors
            tiny = torch.tensor(2.0 ** -25, dtype=torch.float64)
            ek = e + torch.maximum(0.5 * f16_ulp(rk.abs() + e), tiny)
            e = e + drift
            e = e + torch.maximum(0.5 * f16_ulp(r.abs() + e), tiny)
            r_out[b, h], e_out[b, h], rk_out[b, h], ek_out[b, h] = r, e, rk, ek
    fold = lambda t: t.permute(0, 2, 1, 3).reshape(B, R, C)    # noqa: E731
    if ideal:
        return fold(r_out), fold(e_out), fold(rk_out), fold(ek_out)
    return fold(r_out), fold(e_out)


# ---------------------------------------------------------------------------------------------------------------------
# emulation of the tile loop (one (batch, head): q [Tq, hd], k, v [Tk, hd], f16)
# ---------------------------------------------------------------------------------------------------------------------
def emulate(q, k, v, scale, l_from_f16, mutate=None, tile=64, wave_rows=32, prescale=False, pipelined=False):
    """f32 / f16 emulation of the kernels' tile loop: `tile`-key tiles, the deferred rescale with THR 10 decided per `wave_rows`
    query rows, P rounded to f16 for PV, l from the f32 P or (l_from_f16) from the f16 P; prescale / pipelined as in FAMILY.
    `mutate` makes THE EMULATION wrong: "vswap" two V rows of tile 1 exchanged (a kappa slip), "l_norescale" l not rescaled
    after tile 0, "dropkey" the last key missing from PV, "dupl" the last key twice in l, "stale_tile" tile 2 multiplies the V
    of tile 1 (a ring pointer one tile behind)."""
    assert mutate is None or mutate in MUTATIONS
    f32 = torch.float32
    c = c32(scale)
    Tq, hd = q.shape
    Tk = k.shape[0]
    nt = (Tk + tile - 1) // tile
    qf = prescaled_q(q, scale).float() if prescale else q.float()
    kf, vf = k.float(), v.float()
    o, l = torch.zeros(Tq, hd, dtype=f32), torch.zeros(Tq, dtype=f32)
    m = torch.full((Tq,), -1e30, dtype=f32)

    def scores(t):
        s = qf @ kf[t * tile:(t + 1) * tile].T
        return s, (s.max(1).values if prescale else s.max(1).values * c)

    def args(s):
        if prescale:
            return s - m[:, None]
        return (s.double() * c.double() - m.double()[:, None]).to(f32)       # fma: one rounding

    def rescale(t, mx, p16):
        """the wave-uniform decision; scales o, l (and the packed P of the previous tile)"""
        nonlocal o, l, m
        for w0 in range(0, Tq, wave_rows):
            sl = slice(w0, w0 + wave_rows)
            if t == 0 or bool(((mx[sl] - m[sl]) > THR).any()):
                mn = torch.maximum(m[sl], mx[sl])
                al = torch.exp2(m[sl] - mn)
                m[sl] = mn
                if not (mutate == "l_norescale" and t >= 1):
                    l[sl] *= al
                o[sl] *= al[:, None]
                if p16 is not None:
                    p16[sl] = (p16[sl] * al.half().float()[:, None]).half().float()

    def pv(t, p16):
        nonlocal o, l
        vt = vf[t * tile:(t + 1) * tile]
        if mutate == "vswap" and t == 1:
            vt = vt.clone()
            vt[[4, 8]] = vt[[8, 4]]
        if mutate == "stale_tile" and t == 2:
            vt = vf[(t - 1) * tile:t * tile][:vt.shape[0]]
        pp = p16
        if mutate == "dropkey" and t == nt - 1:
            pp = p16.clone()
            pp[:, -1] = 0
        o += pp @ vt
        if l_from_f16:
            l += p16.sum(1)
            if mutate == "dupl" and t == nt - 1:
                l += p16[:, -1]

    def form(t, s):
        nonlocal l
        p = torch.exp2(args(s))
        if not l_from_f16:
            l += p.sum(1)
            if mutate == "dupl" and t == nt - 1:
                l += p[:, -1]
        return p.half().float()

    if not pipelined:
        for t in range(nt):
            s, mx = scores(t)
            rescale(t, mx, None)
            pv(t, form(t, s))
    else:
        s, mx = scores(0)
        rescale(0, mx, None)
        p16 = form(0, s)
        for t in range(nt):
            if t + 1 < nt:
                s, mx = scores(t + 1)
                rescale(t + 1, mx, p16)
            pv(t, p16)
            if t + 1 < nt:
                p16 = form(t + 1, s)
    return (o * (1.0 / l)[:, None]).half()


def emulate_all(prob, kernel=None, mutate=None, **kw):
    """emulate() over every (batch, head) of a probe / random case -> [B, Tq, C] f16; `kernel`: a key of MODELS."""
    if kernel is not None:
        kw = {**MODELS[kernel], **kw}
    q, k, v, heads, hd, kv_div = (prob[n] for n in ("q", "k", "v", "heads", "hd", "kv_div"))
    out = torch.empty(q.shape, dtype=torch.float16)
    for b in range(q.shape[0]):
        for h in range(heads):
            hs = slice(h * hd, (h + 1) * hd)
            out[b, :, hs] = emulate(q[b, :, hs], k[b // kv_div, :, hs], v[b // kv_div, :, hs], prob["scale"], mutate=mutate, **kw)
    return out
