"""Times the map inverse on one MI355X at a full page, 3508 x 2480 from a G = 288 map, at mesh steps 8 and 1:

  map_invert s      ops.map_invert: lattice, fill, raster, resolve, the count finalize and the read-back of six words
  cycle s           ops.map_cycle_error on that forward map: two launches and the read-back of three words
  overlay           ops.mesh_overlay: one launch
  overlay + png     ops.mesh_overlay_to_file: the picture through the device PNG encoder into a file
  host route        what the device route replaces: the lattice's positions on the host and scipy.interpolate.griddata(linear)
                    of the page coordinates at every photograph pixel (step 8); without scipy, tests/mapinv_model.py

HIP events around each device leg (the read-backs they contain included), wall-clock for the host route; the legs INTERLEAVED in
one process after a warm-up of each; the host route runs --host_reps times only, after the device rounds, with one untimed device
call after each.  The kernels of map_invert are timed by pass in a torch.profiler window of their own (--passes calls per step),
never together with the event timing.  The table gives the median and the spread.  Needs a GPU: there is no fallback.

    python benchmarks/mapinv_time.py [--reps 9] [--host_reps 1] [--out profiles/mapinv_time.txt]
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

PASSES = ("lattice_kernel", "fill_kernel", "raster_kernel", "resolve_kernel", "stats_kernel")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--host_reps", type=int, default=1)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--size", type=int, nargs=2, default=(3508, 2480))
    ap.add_argument("--grid", type=int, default=288)
    ap.add_argument("--steps", type=int, nargs="+", default=(8, 1))
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import numpy as np
    import torch
    import mapinv_model as M
    from dvd_amd import ops, synth
    if not torch.cuda.is_available():
        sys.exit("mapinv_time.py needs a GPU: a time taken elsewhere says nothing")
    h, w = a.size
    g = a.grid
    # a smooth page warp (low frequencies, a few per cent of the side) plus a little grid-scale roughness
    yy, xx = np.meshgrid(np.linspace(0, 1, g), np.linspace(0, 1, g), indexing="ij")
    base = np.stack([0.03 * np.sin(2 * np.pi * yy) * np.cos(np.pi * xx) + 0.02, 0.03 * np.cos(np.pi * yy) * np.sin(2 * np.pi * xx) - 0.01])
    flow = torch.from_numpy((base + synth.uniform("mapinv_time/flow", (2, g, g), -2e-4, 2e-4, 1)).astype(np.float32)).cuda()
    src = torch.from_numpy(synth.uniform("mapinv_time/src", (h, w, 3), 0, 255, 2).astype(np.uint8)).cuda()
    fwd = {s: ops.map_invert(flow, h, w, step=s) for s in a.steps}
    tmp = tempfile.mkdtemp()
    png = os.path.join(tmp, "mesh.png")

    def host_route():
        step = max(a.steps)
        x, y = M.positions(flow.cpu().numpy(), h, w)
        rows, cols = M.lattice_axis(h, step), M.lattice_axis(w, step)
        try:
            from scipy.interpolate import griddata
        except ImportError:
            return "tests/mapinv_model.py", M.invert(flow.cpu().numpy(), h, w, step)[0]
        pv, pu = np.meshgrid(rows.astype(np.float64), cols.astype(np.float64), indexing="ij")
        at = np.stack([x[rows][:, cols].reshape(-1), y[rows][:, cols].reshape(-1)], axis=1).astype(np.float64)
        qy, qx = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
        out = griddata(at, np.stack([pu.reshape(-1), pv.reshape(-1)], axis=1), (qx, qy), method="linear")
        return "scipy.interpolate.griddata(linear)", out.astype(np.float32)

    legs = {}
    for s in a.steps:
        legs[f"map_invert s{s}"] = lambda s=s: ops.map_invert(flow, h, w, step=s)
        legs[f"cycle s{s}"] = lambda s=s: ops.map_cycle_error(flow, fwd[s][0])
    first = a.steps[0]
    legs["overlay"] = lambda: ops.mesh_overlay(src, fwd[first][0])
    legs["overlay + png"] = lambda: ops.mesh_overlay_to_file(src, fwd[first][0], png)
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
    how, host = "", None
    for _ in range(a.host_reps):
        t0 = time.perf_counter()
        how, host = host_route()
        t["host route"].append(1e3 * (time.perf_counter() - t0))
        legs[f"map_invert s{first}"]()            # untimed: the host route leaves the device idle for seconds
        torch.cuda.synchronize()
    # the passes of map_invert, in a profiler window of their own
    by_pass = {}
    try:
        from torch.profiler import ProfilerActivity, profile
        for s in a.steps:
            torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                for _ in range(a.passes):
                    ops.map_invert(flow, h, w, step=s)
                torch.cuda.synchronize()
            rows = {}
            for ev in prof.key_averages():
                for name in PASSES:
                    if name in ev.key:
                        total = getattr(ev, "device_time_total", None)
                        total = ev.cuda_time_total if total is None else total
                        rows[name] = total / max(ev.count, 1)
            by_pass[s] = rows
    except Exception as e:                        # a profiler that cannot trace here: the table says so
        by_pass = {"error": repr(e)}
    n = h * w
    lines = [f"# benchmarks/mapinv_time.py on {torch.cuda.get_device_name(0)}: {h} x {w} from G = {g}; {a.reps} interleaved rounds after "
             f"{a.warmup} warm-up ({a.host_reps} of the host route); HIP events around each device leg, wall-clock for the host route; ms per call",
             f"{'leg':<18} {'median ms':>10} {'min ms':>10} {'max ms':>10}"]
    for name, ms in t.items():
        if ms:
            lines.append(f"{name:<18} {statistics.median(ms):>10.3f} {min(ms):>10.3f} {max(ms):>10.3f}")
    med = {name: statistics.median(ms) for name, ms in t.items() if ms}
    for s in a.steps:
        stats = fwd[s][1]
        c = ops.map_cycle_error(flow, fwd[s][0])
        lines.append(f"# step {s}: {stats['tris']} triangles, covered {stats['covered']} of {n} pixels, fold_px {stats['fold_px']}, flipped "
                     f"{stats['flipped_tris']}, skipped {stats['skipped_tris']}; cycle_mean {c['cycle_mean']:.6f} cycle_max {c['cycle_max']:.6f}")
        rows = by_pass.get(s)
        if rows:
            lines.append(f"# step {s} by pass, us per launch (torch.profiler, {a.passes} calls): " +
                         ", ".join(f"{k.replace('_kernel', '')} {rows[k]:.1f}" for k in PASSES if k in rows))
            if "raster_kernel" in rows:
                lines.append(f"# step {s}: the raster pass issues one u32 atomicMin per covered pixel per covering triangle, {stats['covered'] + stats['fold_px']} "
                             f"at least: {(stats['covered'] + stats['fold_px']) / rows['raster_kernel'] * 1e-3:.2f} G atomics/s over the pass (edge tests included)")
            if "fill_kernel" in rows and "resolve_kernel" in rows:
                lines.append(f"# step {s}: byte floor 16 B/px = {16 * n / 1e9:.3f} GB; fill ({5 * n / 1e6:.0f} MB) runs at "
                             f"{5 * n / rows['fill_kernel'] * 1e-3:.0f} GB/s, resolve ({13 * n / 1e6:.0f} MB) at {13 * n / rows['resolve_kernel'] * 1e-3:.0f} GB/s")
    if "error" in by_pass:
        lines.append(f"# by pass: the profiler could not trace here ({by_pass['error']})")
    if host is not None:
        cov = M.covered_of(fwd[max(a.steps)][0].cpu().numpy()) & np.isfinite(host[..., 0])
        diff = np.abs(fwd[max(a.steps)][0].cpu().numpy()[cov] - host[cov]).max()
        lines.append(f"# host route: {how}; where both cover, the device's fwd (step {max(a.steps)}) lies within {diff:.4f} page pixels of it; "
                     f"map_invert s{max(a.steps)} against the host route: {med['host route'] / med[f'map_invert s{max(a.steps)}']:.0f} x")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
