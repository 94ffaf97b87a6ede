"""Times the scan-like page on one MI355X: one text-like page of 3508 x 2480 under shading and a colour cast.

  background s          ops.page_background: the cell maxima (one pass over the page) and the closing and tent on the coarse plane
  flatten s             ops.page_flatten with that estimate given: the flatten kernel alone, with its two counts
  estimate+flatten s    ops.page_flatten as a user calls it
  binarize r            ops.page_binarize of the RGB page, with its count
  chain                 ops.page_clean(binarize=True): estimate, flatten (which also writes its gray plane), binarise
  copy, unwarp_u8       the yardsticks: a device-to-device copy of the page's bytes, and the native unwarp tail
  host                  what a user does today: the page copied to the host, scipy.ndimage maximum, minimum and uniform filters
                        over the same windows in pixels, NumPy division

HIP events around each device leg, wall-clock (beginning with the copy, which synchronises) for the host route; the legs
INTERLEAVED in one process after a warm-up of each.  Beside each time: the bytes the leg must move once - halo re-reads that hit
cache are not counted - and the rate that implies.  The first outputs are held to tests/clean_model.py once.  Needs a GPU: there
is no fallback.

    python benchmarks/clean_time.py [--reps 9] [--host_reps 2] [--out profiles/clean_time.txt]
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
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import numpy as np
    import torch
    from dvd_amd import ops
    import clean_fixtures as X
    import clean_model as M
    if not torch.cuda.is_available():
        sys.exit("clean_time.py needs a GPU: a time taken elsewhere says nothing")
    h, w = a.size
    n = h * w
    host_page = X.text_page(h, w)["page"]
    page = torch.from_numpy(np.array(host_page)).cuda()
    flow = torch.zeros((1, 2, a.grid, a.grid), dtype=torch.float32, device="cuda")
    spare = torch.empty_like(page)
    bgs = {s: ops.page_background(page, cell=s) for s in (8, 16)}

    # the first outputs against the definition, once
    want_bg = M.background(host_page, 16)
    want_flat, want_fs = M.flatten(host_page, want_bg, 16)
    want_plane, want_ink = M.binarize(want_flat)
    got_flat, got_fs = ops.page_flatten(page, return_stats=True)
    got_plane, got_st = ops.page_clean(page, binarize=True, return_stats=True)
    checked = (np.array_equal(bgs[16].cpu().numpy(), want_bg) and np.array_equal(got_flat.cpu().numpy(), want_flat) and got_fs == want_fs
               and np.array_equal(got_plane.cpu().numpy(), want_plane) and got_st == {**want_fs, **want_ink})
    if not checked:
        sys.exit("clean_time.py: the device's page differs from tests/clean_model.py: no time is worth printing")

    legs, moved = {}, {}
    for s in (8, 16):
        coarse = 3 * -(-h // s) * -(-w // s)
        legs[f"background s={s}"] = lambda s=s: ops.page_background(page, cell=s)
        moved[f"background s={s}"] = 3 * n + 3 * coarse
        legs[f"flatten s={s}"] = lambda s=s: ops.page_flatten(page, cell=s, background=bgs[s], return_stats=True)
        moved[f"flatten s={s}"] = 6 * n + coarse
        legs[f"estimate+flatten s={s}"] = lambda s=s: ops.page_flatten(page, cell=s, return_stats=True)
        moved[f"estimate+flatten s={s}"] = 9 * n + 4 * coarse
    for r in (7, 15, 63):
        legs[f"binarize r={r}"] = lambda r=r: ops.page_binarize(page, radius=r, return_stats=True)
        moved[f"binarize r={r}"] = 4 * n
    legs["chain"] = lambda: ops.page_clean(page, binarize=True, return_stats=True)
    moved["chain"] = 12 * n                                     # 3 n estimate, 6 n flatten, n + n its gray plane, n the plane
    legs["copy"] = lambda: spare.copy_(page)
    moved["copy"] = 6 * n
    legs["unwarp_u8"] = lambda: ops.unwarp_u8(flow, page)
    moved["unwarp_u8"] = 6 * n + 8 * a.grid * a.grid
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

    def host_route(s=16, k=2, b=2):
        from scipy import ndimage as ndi
        img = page.cpu().numpy()                                 # the copy synchronises
        win, tent = (s * (2 * k + 1), s * (2 * k + 1), 1), (s * (2 * b + 1), s * (2 * b + 1), 1)
        bg = ndi.minimum_filter(ndi.maximum_filter(img, size=win, mode="nearest"), size=win, mode="nearest")
        bg = ndi.uniform_filter(bg.astype(np.float32), size=tent, mode="nearest")
        return np.clip(np.rint(img * (255.0 / np.maximum(bg, 1.0))), 0, 255).astype(np.uint8)

    t["host s=16"] = []
    for _ in range(a.host_reps):
        t0 = time.perf_counter()
        host_flat = host_route()
        t["host s=16"].append(1e3 * (time.perf_counter() - t0))
    moved["host s=16"] = 6 * n

    lines = [f"# benchmarks/clean_time.py on {torch.cuda.get_device_name(0)}: a text-like page of {h} x {w}; {a.reps} interleaved rounds after "
             f"{a.warmup} warm-up ({a.host_reps} of the host route, {torch.get_num_threads()} threads); HIP events around each device leg, "
             "wall-clock for the host route; ms per call; MB = the bytes the leg must move once (halo re-reads that hit cache are not "
             "counted); background, flattened page, plane and counts at the defaults equal tests/clean_model.py",
             f"{'leg':<26} {'median ms':>10} {'min ms':>10} {'max ms':>10} {'MB':>8} {'GB/s':>8}"]
    med = {}
    for name, ms in t.items():
        med[name] = statistics.median(ms)
        lines.append(f"{name:<26} {med[name]:>10.3f} {min(ms):>10.3f} {max(ms):>10.3f} {moved[name] / 1e6:>8.1f} {moved[name] / med[name] * 1e-6:>8.1f}")
    diff = np.abs(host_flat.astype(int) - want_flat.astype(int))
    lines.append(f"# counts at the defaults: {got_st}")
    lines.append(f"# host s=16: {med['host s=16'] / med['estimate+flatten s=16']:.0f} x the time of estimate+flatten s=16; its page (a box filter "
                 f"where the device has a tent, float division) differs by {diff.mean():.2f} levels on average")
    lines.append(f"# flatten s=16 against copy, the yardstick of the same bytes: {med['flatten s=16'] / med['copy']:.2f} x its time")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
