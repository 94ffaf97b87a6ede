#!/usr/bin/env python3
"""Time a batch of documents of DIFFERENT sizes through the ragged entry points (ops.unwarp_u8_ragged,
ops.ingest_u8_ragged: one launch per stage) against the per-document loop they replace (ops.unwarp_u8, ops.ingest_u8),
in one process, interleaved, with device events (the method of benchmarks/warp_time.py).  Sizes: a fixed list around
3508 x 2480 +- 30 %, odd widths included.  usage: python benchmarks/ragged_time.py [n ...]   (default: 8 32)"""
import os, sys
sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__))); import _lab; LIBSEL = _lab.which()   # --lab selects the lab build
import torch
from dvd_amd import ops

NS = [int(a) for a in sys.argv[1:]] or [8, 32]
G, REPS = 288, 9
# (h, w): 0.7 .. 1.3 x (3508, 2480); widths 1737, 2481, 2999, 3223 are odd, 2050 and 2790 are even but not multiples of 4
SIZES = [(3508, 2480), (2456, 1737), (4560, 3224), (3000, 2481), (3508, 2050), (2800, 2999), (4200, 2480), (2640, 1984),
         (3900, 2790), (3507, 3223), (2480, 3508), (4096, 2304), (3100, 1900), (3333, 2222), (2900, 2900), (4400, 1760)]


def timed(f):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); f(); b.record()
    return a, b


def stats(ev):
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    return ms[len(ms) // 2], ms[0], ms[-1]


for n in NS:
    gen = torch.Generator(device="cuda").manual_seed(3)
    shapes = [SIZES[d % len(SIZES)] for d in range(n)]
    ctrl = (torch.rand(n, 2, 6, 6, device="cuda", generator=gen) - 0.5) * 0.1
    flow = torch.nn.functional.interpolate(ctrl, size=(G, G), mode="bicubic", align_corners=True).contiguous()
    flows = [flow[d:d + 1].contiguous() for d in range(n)]
    srcs = [torch.randint(0, 256, (h, w, 3), device="cuda", dtype=torch.uint8, generator=gen) for h, w in shapes]
    legs = {
        "tail loop": lambda: [ops.unwarp_u8(flows[d], srcs[d]) for d in range(n)],
        "tail ragged": lambda: ops.unwarp_u8_ragged(flow, srcs),
        "ingest loop": lambda: [ops.ingest_u8(s, swap_rb=False, out_size=512, want_rgb=True) for s in srcs],
        "ingest ragged": lambda: ops.ingest_u8_ragged(srcs, swap_rb=False, out_size=512, want_rgb=True),
    }
    # same bytes first (also the warm-up of every shape)
    for a, b in zip(legs["tail loop"](), legs["tail ragged"]()):
        assert torch.equal(a, b)
    y = legs["ingest ragged"]()[0]
    for d, (yd, _) in enumerate(legs["ingest loop"]()):
        assert torch.equal(y[d], yd)
    for f in legs.values():
        f()
    torch.cuda.synchronize()
    ev = {k: [] for k in legs}
    for _ in range(REPS):                                  # interleaved: every repeat runs all four legs
        for k, f in legs.items():
            ev[k].append(timed(f))
        torch.cuda.synchronize()
    launches = {"tail loop": n, "tail ragged": -(-n // 64), "ingest loop": 3 * n, "ingest ragged": 2 * -(-n // 64)}
    fast = sum(1 for h, w in shapes if w % 4 == 0)
    mpx = sum(h * w for h, w in shapes) / 1e6
    print(f"n = {n} documents, {mpx:.0f} Mpx, {fast} on the fast tail path (w % 4 == 0), {n - fast} on the scalar one; "
          f"G = {G}; lib = {LIBSEL}; median [min .. max] of {REPS} interleaved repeats")
    res = {k: stats(v) for k, v in ev.items()}
    for k, (med, lo, hi) in res.items():
        print(f"  {k:14s} {launches[k]:4d} launches  {med:9.3f} ms  [{lo:9.3f} .. {hi:9.3f}]  spread {hi - lo:7.3f} ms")
    for stage in ("tail", "ingest"):
        loop, rag = res[f"{stage} loop"], res[f"{stage} ragged"]
        print(f"  {stage}: ragged - loop = {rag[0] - loop[0]:+.3f} ms (median); spread of the loop's repeats {loop[2] - loop[1]:.3f} ms")
    del srcs, legs, ev
    torch.cuda.empty_cache()
