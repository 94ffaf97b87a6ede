"""Times the synthetic-document render on one MI355X at a full page: one photograph of 3508 x 2480 from a smooth
G = 288 map, mesh step 8.

  map_invert        ops.map_invert: the forward field the render reads (with the read-back of its six counts)
  render 1x         ops.synth_render from a scan of the photograph's size: every radius 1, the bilinear path
  render 2x         ops.synth_render from a scan of twice the sides: radii 2 and 3, the general tent loop
  render + jpeg     render 1x and ops.jpeg_encode_to_file: the photograph as a file
  unwarp_u8         the project's yardstick gather at the same size: ops.unwarp_u8 of a photograph through the same map
  host route        what the device route replaces: torch's CPU grid_sample (bilinear) of the scan through fwd

HIP events around each device leg, wall-clock for the host route; the legs INTERLEAVED in one process after a warm-up of each;
the host route runs --host_reps times only, after the device rounds.  The table gives the median and the spread and, beside
each render, the bytes it must move - fwd 8 B, the background 3 B and the photograph 3 B per pixel, plus the scan's texels once -
and the rate that implies; the texel fetches (12 rx ry bytes per covered pixel) mostly hit cache.  Needs a GPU: there is no
fallback.

    python benchmarks/synth_time.py [--reps 9] [--host_reps 1] [--out profiles/synth_time.txt]
"""
import argparse
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--host_reps", type=int, default=1)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--size", type=int, nargs=2, default=(3508, 2480))
    ap.add_argument("--grid", type=int, default=288)
    ap.add_argument("--step", type=int, default=8)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import numpy as np
    import torch
    from dvd_amd import ops, synth, synth_docs
    if not torch.cuda.is_available():
        sys.exit("synth_time.py needs a GPU: a time taken elsewhere says nothing")
    h, w = a.size
    g = a.grid
    yy, xx = np.meshgrid(np.linspace(0, 1, g), np.linspace(0, 1, g), indexing="ij")
    base = np.stack([0.03 * np.sin(2 * np.pi * yy) * np.cos(np.pi * xx) + 0.02, 0.03 * np.cos(np.pi * yy) * np.sin(2 * np.pi * xx) - 0.01])
    flow = torch.from_numpy(base.astype(np.float32)).cuda()
    key = synth_docs.document_key(0, "synth_time")
    scans = {1: torch.from_numpy(synth_docs.procedural_page(key, h, w)).cuda(), 2: torch.from_numpy(synth_docs.procedural_page(key, 2 * h, 2 * w)).cuda()}
    bg = torch.from_numpy(synth_docs.noise_background(key, h, w)).cuda()
    photo_in = torch.from_numpy(synth.uniform("synth_time/src", (h, w, 3), 0, 255, 2).astype(np.uint8)).cuda()
    fwd, stats = ops.map_invert(flow, h, w, step=a.step)
    shading = dict(l0=1.0, lgx=0.2, lgy=-0.1, k=-0.3)
    jpg = os.path.join(tempfile.mkdtemp(), "photo.jpg")

    legs = {
        "map_invert": lambda: ops.map_invert(flow, h, w, step=a.step),
        "render 1x": lambda: ops.synth_render(scans[1], fwd, background=bg),
        "render 1x shaded": lambda: ops.synth_render(scans[1], fwd, background=bg, shading=dict(shading, a_ref=h * w / stats["covered"])),
        "render 2x": lambda: ops.synth_render(scans[2], fwd, background=bg),
        "render + jpeg": lambda: ops.jpeg_encode_to_file(ops.synth_render(scans[1], fwd, background=bg), jpg),
        "unwarp_u8": lambda: ops.unwarp_u8(flow, photo_in),
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

    def host_route():
        import torch.nn.functional as nnf
        f = fwd.cpu()
        covered = f.view(torch.int32)[..., 0] != ops.MAP_INVALID
        grid = torch.stack([f[..., 0] / (w - 1) * 2 - 1, f[..., 1] / (h - 1) * 2 - 1], dim=-1)
        grid[~covered] = 2.0
        src = scans[1].cpu().permute(2, 0, 1)[None].float()
        out = nnf.grid_sample(src, grid[None], mode="bilinear", padding_mode="border", align_corners=True)[0].permute(1, 2, 0)
        out = torch.where(covered[..., None], out, bg.cpu().float())
        return (out + 0.5).clamp(0, 255).to(torch.uint8), covered

    t["host route"] = []
    host = None
    for _ in range(a.host_reps):
        t0 = time.perf_counter()
        host = host_route()
        t["host route"].append(1e3 * (time.perf_counter() - t0))
        legs["render 1x"]()                       # untimed: the host route leaves the device idle
        torch.cuda.synchronize()
    n = h * w
    moved = {"render 1x": 14 * n + 3 * n, "render 1x shaded": 14 * n + 3 * n, "render 2x": 14 * n + 12 * n, "unwarp_u8": 6 * n + 8 * g * g}
    lines = [f"# benchmarks/synth_time.py on {torch.cuda.get_device_name(0)}: {h} x {w} from G = {g}, step {a.step}; {a.reps} interleaved "
             f"rounds after {a.warmup} warm-up ({a.host_reps} of the host route); HIP events around each device leg, wall-clock for the host "
             "route; ms per call; MB = fwd 8 + background 3 + photograph 3 B/px + the scan once (unwarp_u8: source and page 3 B/px each)",
             f"{'leg':<18} {'median ms':>10} {'min ms':>10} {'max ms':>10} {'MB':>8} {'GB/s':>8}"]
    med = {}
    for name, ms in t.items():
        if not ms:
            continue
        med[name] = statistics.median(ms)
        tail = f" {moved[name] / 1e6:>8.1f} {moved[name] / med[name] * 1e-6:>8.0f}" if name in moved else ""
        lines.append(f"{name:<18} {med[name]:>10.3f} {min(ms):>10.3f} {max(ms):>10.3f}{tail}")
    lines.append(f"# fwd: covered {stats['covered']} of {n} pixels, fold_px {stats['fold_px']}, skipped {stats['skipped_tris']}")
    for mult in (1, 2):
        radii = ops.synth_footprint((mult * h, mult * w), fwd)
        r = radii.max(dim=2).values
        hist = {int(k): int((r == k).sum()) for k in torch.unique(r) if int(k) > 0}
        lines.append(f"# render {mult}x: the larger radius per covered pixel: " + ", ".join(f"{k}: {v}" for k, v in hist.items()) +
                     f"; at the cap ({ops.SYNTH_MAX_RADIUS}): {hist.get(ops.SYNTH_MAX_RADIUS, 0)}")
    lines.append(f"# render 1x against unwarp_u8, the yardstick gather: {med['render 1x'] / med['unwarp_u8']:.2f} x its time; "
                 f"render 2x against render 1x: {med['render 2x'] / med['render 1x']:.2f} x")
    if host is not None:
        mine = ops.synth_render(scans[1], fwd, background=bg).cpu()
        inner = host[1].clone()
        for dy in (-1, 0, 1):                     # where the 3 x 3 window is covered: no edge blend on the device's side
            for dx in (-1, 0, 1):
                inner &= torch.roll(host[1], (dy, dx), (0, 1))
        inner[0], inner[-1], inner[:, 0], inner[:, -1] = False, False, False, False      # off the image counts as uncovered
        diff = (mine.int() - host[0].int()).abs()[inner].max().item()
        lines.append(f"# host route: torch.nn.functional.grid_sample on the CPU ({torch.get_num_threads()} threads); inside the page the "
                     f"device's photograph lies within {diff} levels of it; render 1x against the host route: "
                     f"{med['host route'] / med['render 1x']:.0f} x")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
