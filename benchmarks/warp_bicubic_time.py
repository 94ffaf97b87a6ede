"""Times the bicubic warps beside their bilinear siblings on one MI355X, at the product size 3508 x 2480:

  drop-in   ops.grid_sample(mode=...) on [N,3,3508,2480] f32 with a smooth dewarping grid      (N = --docs-f32, default 2)
  u8 tail   ops.unwarp_u8_batch(mode=...) on [8,3508,2480,3] u8 with a G = 64 flow             (--docs-u8, default 8)

The two modes of a pair are timed INTERLEAVED in one process (bilinear, bicubic, bilinear, ...), each launch between two
HIP events, after a warm-up of both; the table gives the median and the spread over --reps launches.  GB/s is on
ALGORITHMIC bytes - what the operation must move whatever the filter: the grid read once, every source element read once
and every output element written once (drop-in: 2 + 3 + 3 planes of 4 B per pixel = 32 B/px; tail: 3 B read + 3 B
written = 6 B/px, the flow is L2-resident).  A 16-tap filter re-reads its neighbours from LDS / L2, not from HBM, so the
same byte count is the fair yardstick for both modes.  Needs a GPU: there is no fallback.

    python benchmarks/warp_bicubic_time.py [--out profiles/warp_bicubic_time.txt]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def smooth_grid(n, h, w, device):
    import torch
    ys = torch.linspace(-1, 1, h, device=device)[None, :, None].expand(n, h, w)
    xs = torch.linspace(-1, 1, w, device=device)[None, None, :].expand(n, h, w)
    dx = 0.05 * torch.sin(2.1 * ys + 0.3) * torch.cos(1.7 * xs + 1.1)
    dy = 0.05 * torch.cos(1.3 * ys + 2.0) * torch.sin(2.6 * xs + 0.7)
    return (torch.stack([xs + dx, ys + dy], 1) * 0.987).contiguous()


def time_interleaved(calls, reps, warmup):
    """calls: {name: fn}.  Returns {name: [ms per launch]}; the launches alternate between the names."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=3508)
    ap.add_argument("--width", type=int, default=2480)
    ap.add_argument("--docs-f32", type=int, default=2)
    ap.add_argument("--docs-u8", type=int, default=8)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from dvd_amd import ops
    if not torch.cuda.is_available():
        sys.exit("warp_bicubic_time.py needs a GPU: a time taken elsewhere says nothing")
    dev = "cuda"
    h, w = a.height, a.width
    gen = torch.Generator().manual_seed(0)
    rows = []

    n = a.docs_f32
    src = (torch.rand((n, 3, h, w), generator=gen) * 255.0).to(dev)
    grid = smooth_grid(n, h, w, dev)
    t = time_interleaved({m: (lambda m=m: ops.grid_sample(src, grid, mode=m)) for m in ("bilinear", "bicubic")}, a.reps, a.warmup)
    nbytes = n * h * w * 32
    for m, ms in t.items():
        rows.append((f"drop-in f32 {m}", f"{n} x 3 x {h} x {w}", ms, nbytes))
    del src, grid

    n = a.docs_u8
    src8 = torch.randint(0, 256, (n, h, w, 3), generator=gen, dtype=torch.uint8).to(dev)
    flow = ((torch.rand((n, 2, 64, 64), generator=gen) - 0.5) * 0.1).to(dev)
    t = time_interleaved({m: (lambda m=m: ops.unwarp_u8_batch(flow, src8, mode=m)) for m in ("bilinear", "bicubic")}, a.reps, a.warmup)
    nbytes = n * h * w * 6
    for m, ms in t.items():
        rows.append((f"u8 tail {m}", f"{n} x {h} x {w} x 3", ms, nbytes))

    lines = [f"# benchmarks/warp_bicubic_time.py on {torch.cuda.get_device_name(0)}: {a.reps} interleaved launches per mode after "
             f"{a.warmup} warm-ups, HIP events; GB/s on algorithmic bytes (32 B/px drop-in, 6 B/px tail); each launch includes the "
             "wrapper's output allocation",
             f"{'kernel':<24} {'shape':<24} {'median ms':>10} {'min ms':>9} {'max ms':>9} {'GB/s (median)':>14}"]
    for name, shape, ms, nb in rows:
        med = statistics.median(ms)
        lines.append(f"{name:<24} {shape:<24} {med:>10.3f} {min(ms):>9.3f} {max(ms):>9.3f} {nb / med / 1e6:>14.0f}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
