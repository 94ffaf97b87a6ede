"""Times the local-distortion (LD) protocol for ONE pair on one MI355X: a 3508 x 2480 prediction against a 3508 x 2480 ground
truth, both resized to 598 400 pixels (920 x 650), gray, then the SIFT-flow chain of DESIGN.md 4.7 at its defaults (4 levels,
windows 10 / 2, 60 / 30 iterations):

  prepare             ops.resize_gray_u8 x 2 (shared with MS-SSIM)
  descriptors         ops.dense_sift_u8 on both planes of level 0
  cost level l        ops.sflow_cost on level l's size
  level l             ops.sflow_level on level l's size: cost + all BP iterations + argmin
  level l, 1 iter     the same with ONE iteration: (level - this) / (iters - 1) is one BP iteration, the rest cost + argmin
  chain               ops.sift_flow: planes to u8, pyramid, descriptors and the four levels, LD (no read-back of the flow)
  ms_ssim             ops.ssim_scales on the same two planes, for scale

The stage rows run on planes of the right SIZE (level 0's plane cut to the level's size) with window centres of zero: no kernel
of the chain has a data-dependent loop, and the cost kernel's only branch is `q inside the plane`.  The routes are timed
INTERLEAVED in one process, each call between two HIP events, after a warm-up of all of them; the table gives the median and
the spread over --reps calls.  The BP rows also give bytes per iteration (a pixel reads its cost and four messages and writes
four: 18 L bytes, plus 4 of offsets) and the rate that makes.  Needs a GPU: there is no fallback.

    python benchmarks/ld_time.py [--out profiles/ld_time.txt]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def time_interleaved(calls, reps, warmup):
    import torch
    for _ in range(warmup):
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()
    events = {k: [] for k in calls}
    for _ in range(reps):
        for k, fn in calls.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            events[k].append((a, b))
    torch.cuda.synchronize()
    return {k: [a.elapsed_time(b) for a, b in v] for k, v in events.items()}


def bp_bytes(h, w, win):
    """bytes one BP iteration moves at the least: per pixel the cost and four messages in, four messages out (u16), offsets"""
    return h * w * (18 * (2 * win + 1) ** 2 + 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=3508)
    ap.add_argument("--width", type=int, default=2480)
    ap.add_argument("--area", type=int, default=598400)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from dvd_amd import ops
    if not torch.cuda.is_available():
        sys.exit("ld_time.py needs a GPU: a time taken elsewhere says nothing")
    h, w = a.height, a.width
    gen = torch.Generator().manual_seed(0)
    gt = torch.randint(0, 256, (h, w, 3), generator=gen, dtype=torch.uint8).cuda()
    pred = (gt.float() * 0.8 + torch.randint(0, 52, (h, w, 3), generator=gen).cuda()).to(torch.uint8).contiguous()
    th, tw = ops.msssim_target_size(h, w, a.area)
    p = ops.SFLOW_DEFAULTS
    gx, gy = ops.resize_gray_u8(pred[None], th, tw), ops.resize_gray_u8(gt[None], th, tw)
    calls = {"prepare (2 x resize + gray)": lambda: (ops.resize_gray_u8(pred[None], th, tw), ops.resize_gray_u8(gt[None], th, tw)),
             "descriptors level 0 (2 planes)": lambda: (ops.dense_sift_u8(gy), ops.dense_sift_u8(gx))}
    dims, lh, lw = [], th, tw
    for lv in range(p["levels"]):
        dims.append((lh, lw))
        lh, lw = (lh + 1) // 2, (lw + 1) // 2
    stage = {}
    for lv, (lh, lw) in enumerate(dims):
        top = lv == p["levels"] - 1
        win, iters = (p["w_top"], p["iters_top"]) if top else (p["w"], p["iters"])
        da = ops.dense_sift_u8(gy[:, :lh, :lw].contiguous())[0]
        db = ops.dense_sift_u8(gx[:, :lh, :lw].contiguous())[0]
        off = torch.zeros(2, lh, lw, dtype=torch.int16, device="cuda")
        stage[lv] = (win, iters)
        calls[f"cost level {lv} ({lh} x {lw}, L {(2 * win + 1) ** 2})"] = lambda da=da, db=db, off=off, win=win: ops.sflow_cost(da, db, off, win)
        calls[f"level {lv} ({iters} iterations)"] = lambda da=da, db=db, off=off, win=win, iters=iters: ops.sflow_level(da, db, off, win, iters)
        calls[f"level {lv} (1 iteration)"] = lambda da=da, db=db, off=off, win=win: ops.sflow_level(da, db, off, win, 1)
    calls["chain (ops.sift_flow)"] = lambda: ops.sift_flow(gy, gx)
    calls["ms_ssim (5 scales), for scale"] = lambda: ops.ssim_scales(gx, gy, "docunet")
    ld = float(ops.local_distortion(gy, gx)[0])
    t = time_interleaved(calls, a.reps, a.warmup)
    med = {k: statistics.median(v) for k, v in t.items()}
    lines = [f"# benchmarks/ld_time.py on {torch.cuda.get_device_name(0)}: one pair {h} x {w} -> {th} x {tw} ({th * tw} px), defaults "
             f"{p}; {a.reps} interleaved calls per route after {a.warmup} warm-up(s), HIP events; each call includes the wrappers' "
             "allocations; ops.sift_flow also reads LD back (8 bytes)",
             f"# LD of the pair: {ld:.6f}",
             f"{'route':<44} {'median ms':>10} {'min ms':>9} {'max ms':>9}"]
    for name, ms in t.items():
        lines.append(f"{name:<44} {med[name]:>10.3f} {min(ms):>9.3f} {max(ms):>9.3f}")
    lines.append("# one BP iteration = (level - level with 1 iteration) / (iterations - 1); bytes = 18 L + 4 per pixel")
    for lv, (lh, lw) in enumerate(dims):
        win, iters = stage[lv]
        per = (med[f"level {lv} ({iters} iterations)"] - med[f"level {lv} (1 iteration)"]) / (iters - 1)
        nbytes = bp_bytes(lh, lw, win)
        lines.append(f"BP iteration level {lv}: {per:.4f} ms, {nbytes / 1e6:.1f} MB -> {nbytes / 1e6 / max(per, 1e-9):.0f} GB/s")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
