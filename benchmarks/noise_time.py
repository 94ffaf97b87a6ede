"""Times the keyed sampler noise against torch.randn on one MI355X, at the two shapes the sampling loop draws:
[16,2,288,288] (8 documents x 2 hypotheses at G = 288) and [2,2,64,64].  `ops.randn_keyed` is timed twice: from a list of keys
(the wrapper uploads them: one small host-to-device copy per call) and from keys already on the device (what the loop does
after its first draw), both into a fresh tensor like torch.randn; `ops.map_deviation` on 8 documents is beside them.  HIP events
around each call, the routes INTERLEAVED in one process after a warm-up of each; the table gives the median and the spread over
--reps rounds.  Needs a GPU: there is no fallback.

    python benchmarks/noise_time.py [--reps 25] [--out profiles/noise_time.txt]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from dvd_amd import ops
    if not torch.cuda.is_available():
        sys.exit("noise_time.py needs a GPU: a time taken elsewhere says nothing")
    routes = {}
    for docs, hyp, g in ((8, 2, 288), (1, 2, 64)):
        keys = [ops.corruption_key(1992, f"doc{i}") for i in range(docs)]
        keys_dev = ops.noise_keys_tensor(keys, "cuda")
        shape = (docs * hyp, 2, g, g)
        routes[("torch.randn", shape)] = lambda shape=shape: torch.randn(shape, device="cuda")
        routes[("randn_keyed, keys uploaded", shape)] = lambda keys=keys, hyp=hyp, g=g: ops.randn_keyed(keys, hyp, g, 0)
        routes[("randn_keyed, device keys", shape)] = lambda keys=keys_dev, hyp=hyp, g=g: ops.randn_keyed(keys, hyp, g, 0)
    maps = torch.randn(2, 8, 2, 288, 288, device="cuda")
    routes[("map_deviation", (8, 2, 288, 288))] = lambda: ops.map_deviation(maps[0], maps[1])
    for _ in range(a.warmup):
        for fn in routes.values():
            fn()
    torch.cuda.synchronize()
    t = {name: [] for name in routes}
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(a.reps):
        for name, fn in routes.items():
            start.record()
            fn()
            stop.record()
            stop.synchronize()
            t[name].append(start.elapsed_time(stop))
    lines = [f"# benchmarks/noise_time.py on {torch.cuda.get_device_name(0)}: {a.reps} interleaved rounds after {a.warmup} warm-ups; "
             "HIP events around each call (allocation of the result included; map_deviation: its read-back too), ms per call",
             f"{'route':<28} {'shape':>18} {'median ms':>10} {'min ms':>10} {'max ms':>10}"]
    for (name, shape), ms in t.items():
        lines.append(f"{name:<28} {'x'.join(str(v) for v in shape):>18} {statistics.median(ms):>10.4f} {min(ms):>10.4f} {max(ms):>10.4f}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
