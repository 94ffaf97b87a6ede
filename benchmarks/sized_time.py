"""Times the page at a chosen size on one MI355X: one photograph of 3508 x 2480 under a smooth G = 288 map,
rendered to the photograph's own size, to half and to an eighth of its sides.

  sized 1/1, 1/2, 1/8   ops.unwarp_u8_sized with the three counts (its memset, launch and 24-byte read-back)
  unwarp_u8             the project's yardstick gather: the native tail at the photograph's size
  host BOX, LANCZOS     what a user does today for a smaller page: ops.unwarp_u8, the page copied to the host, PIL's resize

HIP events around each device leg, wall-clock (ending in the copy, which synchronises) for the host routes; the legs INTERLEAVED
in one process after a warm-up of each; the host routes run --host_reps times per size after the device rounds.  Beside each
time: the bytes the leg must move - a sized page reads every texel of the photograph once (3 B/px) and writes 3 B per page
pixel; the map is 8 G^2 bytes - and the rate that implies.  The taps' repeated fetches (12 rx ry bytes per page pixel) mostly
hit cache and are not counted.  Needs a GPU: there is no fallback.

    python benchmarks/sized_time.py [--reps 9] [--host_reps 3] [--out profiles/sized_time.txt]
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
    ap.add_argument("--host_reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--size", type=int, nargs=2, default=(3508, 2480))
    ap.add_argument("--grid", type=int, default=288)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import numpy as np
    import torch
    from PIL import Image
    from dvd_amd import ops, synth
    if not torch.cuda.is_available():
        sys.exit("sized_time.py needs a GPU: a time taken elsewhere says nothing")
    h, w = a.size
    g = a.grid
    yy, xx = np.meshgrid(np.linspace(0, 1, g), np.linspace(0, 1, g), indexing="ij")
    base = np.stack([0.03 * np.sin(2 * np.pi * yy) * np.cos(np.pi * xx) + 0.02, 0.03 * np.cos(np.pi * yy) * np.sin(2 * np.pi * xx) - 0.01])
    flow = torch.from_numpy(base.astype(np.float32)).cuda()
    photo = torch.from_numpy(synth.uniform("sized_time/src", (h, w, 3), 0, 255, 2).astype(np.uint8)).cuda()
    sizes = {"1/1": (h, w), "1/2": (max(1, h // 2), max(1, w // 2)), "1/8": (max(1, h // 8), max(1, w // 8))}   # 1754 x 1240, 438 x 310

    legs = {f"sized {k}": (lambda s=s: ops.unwarp_u8_sized(flow, photo, s, return_stats=True)) for k, s in sizes.items()}
    legs["unwarp_u8"] = lambda: ops.unwarp_u8(flow[None], photo)
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

    def host_route(size, resample):
        page = ops.unwarp_u8(flow[None], photo).cpu().numpy()                 # the copy synchronises
        return np.asarray(Image.fromarray(page).resize((size[1], size[0]), resample))

    host = {}
    for k in ("1/2", "1/8"):
        for label, resample in (("BOX", Image.BOX), ("LANCZOS", Image.LANCZOS)):
            name = f"host {label} {k}"
            t[name] = []
            for _ in range(a.host_reps):
                t0 = time.perf_counter()
                host[name] = host_route(sizes[k], resample)
                t[name].append(1e3 * (time.perf_counter() - t0))
    n = h * w
    moved = {f"sized {k}": 3 * n + 3 * s[0] * s[1] + 8 * g * g for k, s in sizes.items()}   # every texel of the photograph once
    moved["unwarp_u8"] = 6 * n + 8 * g * g
    for k in ("1/2", "1/8"):
        for label in ("BOX", "LANCZOS"):
            moved[f"host {label} {k}"] = 6 * n + 8 * g * g + 3 * n            # the native tail, and the page across the bus
    lines = [f"# benchmarks/sized_time.py on {torch.cuda.get_device_name(0)}: a photograph of {h} x {w}, G = {g}; {a.reps} interleaved rounds "
             f"after {a.warmup} warm-up ({a.host_reps} of each host route, {torch.get_num_threads()} threads); HIP events around each device leg, "
             "wall-clock for the host routes; ms per call; MB = the bytes the leg must move once (taps that hit cache are not counted)",
             f"{'leg':<20} {'page':>12} {'median ms':>10} {'min ms':>10} {'max ms':>10} {'MB':>8} {'GB/s':>8}"]
    med = {}
    for name, ms in t.items():
        med[name] = statistics.median(ms)
        key = name.split()[-1]
        page = sizes.get(key, (h, w))
        lines.append(f"{name:<20} {page[0]:>6}x{page[1]:<5} {med[name]:>10.3f} {min(ms):>10.3f} {max(ms):>10.3f} {moved[name] / 1e6:>8.1f} "
                     f"{moved[name] / med[name] * 1e-6:>8.1f}")
    for k, s in sizes.items():
        foot = ops.sized_footprint(flow, (h, w), s).int()
        r = torch.maximum(foot & 255, foot >> 8)
        hist = {int(v): int((r == v).sum()) for v in torch.unique(r)}
        _, cnt = ops.unwarp_u8_sized(flow, photo, s, return_stats=True)
        lines.append(f"# sized {k}: the larger radius per page pixel: " + ", ".join(f"{v}: {c}" for v, c in hist.items()) + f"; counts {cnt}")
    lines.append(f"# sized 1/1 against unwarp_u8, the yardstick gather: {med['sized 1/1'] / med['unwarp_u8']:.2f} x its time")
    for k in ("1/2", "1/8"):
        mine = ops.unwarp_u8_sized(flow, photo, sizes[k]).cpu().numpy().astype(int)
        for label in ("BOX", "LANCZOS"):
            name = f"host {label} {k}"
            diff = np.abs(mine - host[name].astype(int))
            lines.append(f"# {name}: {med[name] / med[f'sized {k}']:.1f} x the time of sized {k}; the pages differ by at most {diff.max()} levels, "
                         f"{diff.mean():.2f} on average (random bytes: another filter is another page)")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
