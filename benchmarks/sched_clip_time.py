"""Time dvd_sched_step, dvd_sched_step_clip and (dvd_sched_step + a separate in-place clamp launch) at N = 16, G = 288
with HIP events in one process, interleaved:    python benchmarks/sched_clip_time.py"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch
from dvd_amd import ops, schedule

N, G, REP, ROUNDS = 16, 288, 200, 7
tab = schedule.Tables(schedule.named_betas("cosine", 50))
c = tab.ddim_coef(25)
x_t = torch.randn(N, 2, G, G, device="cuda")
x0 = torch.randn(N, 2, G, G, device="cuda") * 1.5
out = torch.empty_like(x_t)
variants = {
    "plain": lambda: ops.sched_step(c, x_t, x0, out=out),
    "clip": lambda: ops.sched_step(c, x_t, x0, out=out, clip=True),
    "plain+clamp_": lambda: (x0.clamp_(-1, 1), ops.sched_step(c, x_t, x0, out=out)),
}
for f in variants.values():
    for _ in range(20):
        f()
torch.cuda.synchronize()
res = {k: [] for k in variants}
for r in range(ROUNDS):
    for k, f in variants.items():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(REP):
            f()
        b.record()
        torch.cuda.synchronize()
        res[k].append(a.elapsed_time(b) / REP * 1e3)
for k, v in res.items():
    v = sorted(v)
    print(f"{k:14s} median {v[len(v)//2]:.2f} us  min {v[0]:.2f}  max {v[-1]:.2f}   (back-to-back launches, {REP} per sample, {ROUNDS} rounds)")
