"""Times getting ONE page from a PNG file's bytes to [H,W,3] uint8 RGB on the device, on one MI355X and its host: a
3508 x 2480 page, noisy and with exactly flat white margins, written by PIL at its default level, through

  hip/decode      dvd_png_decode_rgb8 with the file already on the device and preallocated buffers; host clock around the call
                  and a synchronise (the call itself reads back the candidate count, the candidate table, 4 bytes per group of
                  doubling rounds and the status word, so HIP events around it would time the same span)
  hip/+upload     the same plus the host-to-device copy of the FILE (what env.png_decoder='hip' does, less the file system)
  PIL             Image.open + exif_transpose + convert('RGB') on the host (what env.png_decoder='pil' does)
  PIL/+upload     the same plus the host-to-device copy of the 26 MB of PIXELS

The routes are timed INTERLEAVED in one process after a warm-up of each; the table gives the median and the spread over --reps
rounds, the decoder's statistics and whether the device's pixels equal PIL's.  Needs a GPU: there is no fallback.

    python benchmarks/pngdec_time.py [--reps 7] [--out profiles/pngdec_time.txt]

Time by stage comes from a kernel trace, taken in a run of its own (tracing slows the host):

    rocprofv3 --kernel-trace --stats -d <dir> -- python benchmarks/pngdec_time.py --decodes 5
    python benchmarks/pngdec_time.py --stages <dir> --decodes 5 [--out profiles/pngdec_time.txt, appended]
"""
import argparse
import csv
import glob
import io
import os
import statistics
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

STAGES = (("gather + CRC-32", ("pngdec_gather_kernel", "pngdec_crc_kernel")),
          ("finder", ("pngdec_find_kernel", "pngdec_candscan_kernel", "pngdec_scatter_kernel")),
          ("count", ("pngdec_count_kernel",)),
          ("write", ("pngdec_write_kernel",)),
          ("doubling", ("pngdec_double_kernel",)),
          ("resolve + Adler-32 + bands", ("pngdec_resolve_kernel", "pngdec_bands_kernel")),
          ("unfilter", ("pngdec_unfilter_kernel", "pngdec_final_kernel")))


def page(h, w, seed=5):
    """A page-like picture: a noisy body (uniform noise of 48 levels on a ramp) inside exactly flat white margins."""
    import numpy as np
    rng = np.random.RandomState(seed)
    img = np.full((h, w, 3), 255, np.uint8)
    my, mx = h // 12, w // 10
    yy, xx = np.mgrid[0:h - 2 * my, 0:w - 2 * mx]
    img[my:h - my, mx:w - mx] = ((yy // 7 + xx // 5)[..., None] + rng.randint(0, 48, (h - 2 * my, w - 2 * mx, 3))).astype(np.uint8)
    return img


def stage_table(trace_dir, decodes):
    """rocprofv3's kernel statistics under trace_dir (*kernel_stats.csv, or the *_results.db it writes by default) -> lines:
    kernel time per stage and decode."""
    total = {}
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_stats.csv"), recursive=True):
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                total[row["Name"]] = total.get(row["Name"], 0.0) + float(row["TotalDurationNs"])
    for path in glob.glob(os.path.join(trace_dir, "**", "*_results.db"), recursive=True):
        import sqlite3
        with sqlite3.connect(path) as db:
            for name, ns in db.execute("select name, sum(end - start) from kernels group by name"):
                total[name] = total.get(name, 0.0) + float(ns)
    if not total:
        sys.exit(f"no kernel statistics under {trace_dir}")
    lines = [f"# time by stage: rocprofv3 --kernel-trace --stats over {decodes} decodes of the page, kernel time per decode",
             f"{'stage':<28} {'ms':>10}"]
    for stage, kernels in STAGES:
        ns = sum(v for name, v in total.items() if any(k in name for k in kernels))
        lines.append(f"{stage:<28} {ns / decodes / 1e6:>10.3f}")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=3508)
    ap.add_argument("--width", type=int, default=2480)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--decodes", type=int, default=0, help="only decode the page this many times (for a kernel trace)")
    ap.add_argument("--stages", default="", help="directory of a rocprofv3 kernel trace of a --decodes run: append the stage table")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.stages:
        text = "\n".join(stage_table(a.stages, max(1, a.decodes)))
        print(text)
        if a.out:
            with open(a.out, "a") as f:
                f.write(text + "\n")
        return
    import ctypes as C
    import numpy as np
    import torch
    from PIL import Image
    from dvd_amd import lib, ops
    if not torch.cuda.is_available():
        sys.exit("pngdec_time.py needs a GPU: a time taken elsewhere says nothing")
    h, w = a.height, a.width
    buf = io.BytesIO()
    Image.fromarray(page(h, w)).save(buf, format="PNG")
    data = buf.getvalue()
    host = np.frombuffer(bytearray(data), dtype=np.uint8)
    host_t = torch.from_numpy(host).pin_memory()
    info = ops.png_probe(data)
    file_dev = host_t.cuda()
    out = torch.empty(3 * h * w, dtype=torch.uint8, device="cuda")
    scratch = torch.empty(info["scratch_bytes"], dtype=torch.uint8, device="cuda")
    stats = lib.PngDecStats()

    def hip_decode():
        rc = lib.raw().dvd_png_decode_rgb8(host.ctypes.data, lib.ptr(file_dev), host.size, lib.ptr(out), out.numel(), 0,
                                           C.byref(stats), lib.ptr(scratch), lib.stream_ptr())
        assert rc == 0, lib.raw().dvd_last_error()
        torch.cuda.synchronize()

    if a.decodes:
        for _ in range(a.decodes):
            hip_decode()
        return

    def hip_upload():
        file_dev.copy_(host_t, non_blocking=True)
        hip_decode()

    def pil():
        return ops.pil_decode_rgb8(data)

    def pil_upload():
        px = torch.from_numpy(pil()).cuda()
        torch.cuda.synchronize()
        return px

    routes = {"hip/decode": hip_decode, "hip/+upload": hip_upload, "PIL": pil, "PIL/+upload": pil_upload}
    for _ in range(a.warmup):
        for fn in routes.values():
            fn()
    equal = bool(torch.equal(out.view(h, w, 3), pil_upload()))
    t = {k: [] for k in routes}
    for _ in range(a.reps):
        for k, fn in routes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            t[k].append((time.perf_counter() - t0) * 1e3)
    lines = [f"# benchmarks/pngdec_time.py on {torch.cuda.get_device_name(0)}: one page {h} x {w}, noisy with flat margins, written by "
             f"PIL at its default level; {a.reps} interleaved rounds after {a.warmup} warm-ups; host clock",
             f"{'route':<12} {'median ms':>10} {'min ms':>10} {'max ms':>10}"]
    for k, ms in t.items():
        lines.append(f"{k:<12} {statistics.median(ms):>10.3f} {min(ms):>10.3f} {max(ms):>10.3f}")
    lines.append(f"# file {len(data)} bytes in {info['idat_chunks']} IDAT chunks, scratch {info['scratch_bytes']} bytes; candidates "
                 f"{stats.candidates}, segments {stats.segments}, doubling rounds {stats.rounds}, bands {stats.bands}; pixels equal "
                 f"PIL's: {equal}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
