"""Times the map score on one MI355X at a full page, 3508 x 2480 from a G = 288 map with H = 2 hypotheses,
against a ground-truth field of that size:

  map_errors       ops.map_errors: the kernel that writes the planes e and sigma and the block partials, one launch
  map_metrics      ops.map_metrics: that kernel, the finalize workgroup and the read-back of seven words
  select e, sigma  ops.select_kth_desc of the 50 ranks on either plane: eight launches each, no read-back
  bins e, sigma    the 50 thresholds (selected outside the window) and dvd_sparsify_bins for either key, two launches each
  sparsification   ops.sparsification: both selections, both bins, one read-back of 408 integers, the curves on the host
  map_score        ops.map_score: everything, as the document loop calls it
  host route       what the device route replaces: the prediction's and the hypotheses' fields copied to the host
                   (ops.flow_full_uv(...).cpu(): four 70 MB fields with the ground truth), then tests/mapscore_model.py

HIP events around each device leg (the read-backs they contain included), wall-clock for the host route; the legs INTERLEAVED in
one process after a warm-up of each; the host route runs --host_reps times only, after the device rounds, with one untimed
device call after each.  The table gives the median and the spread.  Needs a GPU: there is no fallback.

    python benchmarks/mapscore_time.py [--reps 9] [--host_reps 2] [--out profiles/mapscore_time.txt]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--host_reps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--size", type=int, nargs=2, default=(3508, 2480))
    ap.add_argument("--grid", type=int, default=288)
    ap.add_argument("--hyps", type=int, default=2)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import numpy as np
    import torch
    import mapscore_model as M
    from dvd_amd import ops, synth
    if not torch.cuda.is_available():
        sys.exit("mapscore_time.py needs a GPU: a time taken elsewhere says nothing")
    h, w = a.size
    g = a.grid

    def coarse(name, lo, hi, n=None):
        shape = (2, g, g) if n is None else (n, 2, g, g)
        return torch.from_numpy(synth.uniform(f"mapscore_time/{name}", shape, lo, hi, 1)).cuda()
    flow = coarse("flow", -0.05, 0.05)
    px = 1.0 / max(h, w)
    gt = ops.flow_full_uv((flow + coarse("gt", -4 * px, 4 * px)).contiguous(), h, w)          # a ground truth a few pixels away
    hyps = (flow[None] + coarse("hyps", -2 * px, 2 * px, a.hyps)).contiguous()
    e, sigma = ops.map_errors(flow, gt, hyps)
    n_valid = ops.map_valid_count(e)
    ranks = ops.map_ranks(n_valid)
    head = ops._map_head(e.device)
    thr = {name: ops.select_kth_desc(key, ranks, n_valid).view(torch.int32) for name, key in (("e", e), ("sigma", sigma))}

    def host_route():
        fields = [ops.flow_full_uv(x, h, w).cpu().numpy() for x in (flow, *hyps)]
        return M.score(M.errors(fields[0], gt.cpu().numpy(), np.stack(fields[1:])))

    legs = {
        "map_errors": lambda: ops.map_errors(flow, gt, hyps),
        "map_metrics": lambda: ops.map_metrics(flow, gt, hyps),
        "select e": lambda: ops.select_kth_desc(e, ranks, n_valid),
        "select sigma": lambda: ops.select_kth_desc(sigma, ranks, n_valid),
        "bins e": lambda: ops._map_bins(e, e, thr["e"], head),
        "bins sigma": lambda: ops._map_bins(e, sigma, thr["sigma"], head),
        "sparsification": lambda: ops.sparsification(e, sigma, n_valid),
        "map_score": lambda: ops.map_score(flow, gt, hyps),
    }
    for _ in range(a.warmup):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    t = {name: [] for name in legs}
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(a.reps):
        for name, fn in legs.items():
            start.record()
            fn()
            stop.record()
            stop.synchronize()
            t[name].append(start.elapsed_time(stop))
    t["host route"] = []
    for _ in range(a.host_reps):
        t0 = time.perf_counter()
        host = host_route()
        t["host route"].append(1e3 * (time.perf_counter() - t0))
        legs["map_score"]()                     # untimed: the host route leaves the device idle for seconds
        torch.cuda.synchronize()
    dev = ops.map_score(flow, gt, hyps)
    lines = [f"# benchmarks/mapscore_time.py on {torch.cuda.get_device_name(0)}: {h} x {w} from G = {g}, H = {a.hyps}, {n_valid} valid pixels; "
             f"{a.reps} interleaved rounds after {a.warmup} warm-up ({a.host_reps} of the host route); HIP events around each device leg, "
             "wall-clock for the host route; ms per call",
             f"{'leg':<18} {'median ms':>10} {'min ms':>10} {'max ms':>10}"]
    for name, ms in t.items():
        if ms:
            lines.append(f"{name:<18} {statistics.median(ms):>10.3f} {min(ms):>10.3f} {max(ms):>10.3f}")
    med = {name: statistics.median(ms) for name, ms in t.items() if ms}
    stages = {k: med[k] for k in ("map_metrics", "select e", "select sigma", "bins e", "bins sigma")}
    top = max(stages, key=stages.get)
    lines.append(f"# of the stages of map_score ({' + '.join(stages)} = {sum(stages.values()):.3f} ms) the largest is {top}: {stages[top]:.3f} ms")
    plane = 4 * h * w
    lines.append(f"# map_errors reads the {2 * plane / 1e6:.1f} MB ground truth and writes two planes of {plane / 1e6:.1f} MB: "
                 f"{4 * plane / (med['map_errors'] * 1e-3) / 1e9:.0f} GB/s at the median, allocation of the workspace included")
    if t["host route"]:
        same = all(dev[k] == host[k] for k in ("n_valid", "pck1", "pck3", "pck5", "fl")) and \
            all(dev["AUSE"][m] == host["AUSE"][m] for m in M.METRICS) and abs(dev["epe"] - host["epe"]) <= 1e-9 * host["epe"]
        lines.append(f"# the device's counts and AUSE equal the host route's, its EPE lies within 1e-9 of it: {same}")
        lines.append(f"# map_score against the host route: {med['host route'] / med['map_score']:.0f} x")
    lines.append(f"# epe {dev['epe']:.6f} pck1 {dev['pck1']:.6f} pck5 {dev['pck5']:.6f} fl {dev['fl']:.6f} ause_epe {dev['ause_epe']:.6f}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
