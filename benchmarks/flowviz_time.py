"""Times the flow pictures on one MI355X at a full page, 3508 x 2480 from a G = 288 map:

  picture, diag    ops.flow_picture(norm='diag'): the fused up-sample-and-colour kernel alone, one launch
  picture          ops.flow_picture(norm='max') alone: the radius reduction, then the fused up-sample-and-colour kernel
  picture to file  ops.flow_picture_to_file: those kernels, the PNG encoder and the copy of the compressed file (to a temporary
                   directory)
  .flo             ops.flow_write_flo: the field kernel, the 70 MB copy to the host and the file
  host route       what the device route replaces: the field copied to the host, tests/flowviz_model.py (NumPy) on it, PIL's
                   Image.save

HIP events around each call for the device legs (the read-backs they contain included), wall-clock for the host route; the legs
INTERLEAVED in one process after a warm-up of each (the host route last, and one untimed picture after it); the table gives the median and the spread over --reps rounds, and for the
picture the achieved GB/s of its 3 B/px of stores.  Needs a GPU: there is no fallback.

    python benchmarks/flowviz_time.py [--reps 9] [--out profiles/flowviz_time.txt]
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
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--size", type=int, nargs=2, default=(3508, 2480))
    ap.add_argument("--grid", type=int, default=288)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import numpy as np
    import torch
    from PIL import Image
    import flowviz_model as M
    from dvd_amd import ops, synth
    if not torch.cuda.is_available():
        sys.exit("flowviz_time.py needs a GPU: a time taken elsewhere says nothing")
    h, w = a.size
    flow = torch.from_numpy(synth.uniform("flowviz_time/flow", (2, a.grid, a.grid), -0.05, 0.05, 1)).cuda()
    tmp = tempfile.mkdtemp(prefix="flowviz_time_")

    def host_route():
        field = ops.flow_full_uv(flow, h, w).cpu().numpy()
        Image.fromarray(M.flow_to_image(field, norm="max")).save(os.path.join(tmp, "host.png"))

    legs = {
        "picture, diag": lambda: ops.flow_picture(flow, h, w, norm="diag"),
        "picture": lambda: ops.flow_picture(flow, h, w, norm="max"),
        "picture to file": lambda: ops.flow_picture_to_file(flow, h, w, os.path.join(tmp, "dev.png"), norm="max"),
        ".flo": lambda: ops.flow_write_flo(flow, h, w, os.path.join(tmp, "dev.flo")),
        "host route": host_route,
    }
    for _ in range(a.warmup):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    t = {name: [] for name in legs}
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(a.reps):
        for name, fn in legs.items():
            t0 = time.perf_counter()
            start.record()
            fn()
            stop.record()
            stop.synchronize()
            t[name].append(start.elapsed_time(stop) if name != "host route" else 1e3 * (time.perf_counter() - t0))
        legs["picture"]()                       # untimed: the host route leaves the device idle for seconds, and the leg that
        torch.cuda.synchronize()                # follows it would be timed on a device that is still waking up
    lines = [f"# benchmarks/flowviz_time.py on {torch.cuda.get_device_name(0)}: {h} x {w} from G = {a.grid}, {a.reps} interleaved rounds "
             f"after {a.warmup} warm-up; HIP events around each device leg, wall-clock for the host route; ms per call",
             f"{'leg':<18} {'median ms':>10} {'min ms':>10} {'max ms':>10}"]
    for name, ms in t.items():
        lines.append(f"{name:<18} {statistics.median(ms):>10.3f} {min(ms):>10.3f} {max(ms):>10.3f}")
    stores = 3 * h * w
    lines.append(f"# picture, diag: {stores / (statistics.median(t['picture, diag']) * 1e-3) / 1e9:.0f} GB/s of stores at the median "
                 "(one launch, allocation of the result included)")
    lines.append(f"# picture: {stores / 1e6:.1f} MB of stores (the G = {a.grid} map, {8 * a.grid ** 2 / 1e6:.2f} MB, is read from cache, "
                 f"twice): {stores / (statistics.median(t['picture']) * 1e-3) / 1e9:.0f} GB/s at the median, allocation of the "
                 "result and both launches of the reduction included")
    lines.append(f"# files: dev.png {os.path.getsize(os.path.join(tmp, 'dev.png'))} bytes, host.png "
                 f"{os.path.getsize(os.path.join(tmp, 'host.png'))} bytes, dev.flo {os.path.getsize(os.path.join(tmp, 'dev.flo'))} bytes")
    same = np.array_equal(np.asarray(Image.open(os.path.join(tmp, "dev.png"))), np.asarray(Image.open(os.path.join(tmp, "host.png"))))
    lines.append(f"# the device picture and the host route's picture hold the same pixels: {same}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
