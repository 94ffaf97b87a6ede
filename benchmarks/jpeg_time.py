"""Times getting ONE dewarped page into a file's bytes on one MI355X and its host: the 3508 x 2480 page of benchmarks/png_time.py
(`page_image`: the page-like picture of dvd_amd/synth.py plus 4 % uniform noise), through

  jpeg hip/kernels   ops.jpeg_encode's four launches into preallocated buffers (dvd_jpeg_encode_rgb8), HIP events
  jpeg hip/+copy     the same plus the length read-back and the device-to-host copy of the file only, host clock around a call
                     that ends in the copy's synchronise (what env.page_format='jpeg' does, less the file system)
  png hip/kernels    dvd_png_encode_rgb8's four launches, HIP events
  png hip/+copy      the same plus read-back and copy (env.png_encoder='hip')
  PIL jpeg           the device-to-host copy of the 26 MB page + Image.save(format='JPEG') at the same quality and subsampling,
                     optimize=False, restart_marker_rows=1, into memory, host clock
  PIL png level 6    the copy of the page + Image.save(format='PNG') (env.png_encoder='pil', the reference's route), host clock

The routes are timed INTERLEAVED in one process after a warm-up of each; the table gives the median and the spread over --reps
rounds and the file sizes beside the times.  Needs a GPU: there is no fallback.

    python benchmarks/jpeg_time.py [--reps 7] [--quality 90] [--subsampling 420] [--out profiles/jpeg_time.txt]
"""
import argparse
import io
import os
import statistics
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=3508)
    ap.add_argument("--width", type=int, default=2480)
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--subsampling", default="420", choices=("420", "444"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import numpy as np
    import torch
    from PIL import Image
    from dvd_amd import lib, ops
    from png_time import page_image
    if not torch.cuda.is_available():
        sys.exit("jpeg_time.py needs a GPU: a time taken elsewhere says nothing")
    h, w = a.height, a.width
    quality, flag = ops.jpeg_settings(a.quality, a.subsampling)
    page = page_image(h, w)
    dev = torch.from_numpy(page).cuda()
    nbytes = torch.zeros(1, dtype=torch.int64, device="cuda")
    jcap = ops.jpeg_bound(h, w, a.subsampling)
    jout = torch.empty(jcap, dtype=torch.uint8, device="cuda")
    jscratch = torch.empty(ops._size_query("dvd_jpeg_scratch_bytes", h, w, flag), dtype=torch.uint8, device="cuda")
    pcap = ops.png_bound(h, w)
    pout = torch.empty(pcap, dtype=torch.uint8, device="cuda")
    pscratch = torch.empty(ops._size_query("dvd_png_scratch_bytes", h, w), dtype=torch.uint8, device="cuda")
    sizes = {}

    def jpeg_kernels():
        lib.call("dvd_jpeg_encode_rgb8", lib.ptr(dev), h, w, quality, flag, lib.ptr(jout), jcap, lib.ptr(nbytes), lib.ptr(jscratch),
                 lib.stream_ptr())

    def png_kernels():
        lib.call("dvd_png_encode_rgb8", lib.ptr(dev), h, w, lib.ptr(pout), pcap, lib.ptr(nbytes), lib.ptr(pscratch), lib.stream_ptr())

    def with_copy(kernels, out, key):
        def run():
            kernels()
            data = out[:int(nbytes.item())].cpu()
            sizes[key] = data.numel()
            return data
        return run

    def pil_jpeg():
        buf = io.BytesIO()
        Image.fromarray(dev.cpu().numpy()).save(buf, format="JPEG", quality=quality, subsampling={"420": 2, "444": 0}[a.subsampling],
                                                optimize=False, restart_marker_rows=1)
        sizes["PIL jpeg"] = len(buf.getvalue())
        return buf.getvalue()

    def pil_png():
        buf = io.BytesIO()
        Image.fromarray(dev.cpu().numpy()).save(buf, format="PNG")
        sizes["PIL png level 6"] = len(buf.getvalue())

    events = {"jpeg hip/kernels": jpeg_kernels, "png hip/kernels": png_kernels}
    host = {"jpeg hip/+copy": with_copy(jpeg_kernels, jout, "jpeg hip/+copy"), "png hip/+copy": with_copy(png_kernels, pout, "png hip/+copy"),
            "PIL jpeg": pil_jpeg, "PIL png level 6": pil_png}
    for _ in range(a.warmup):
        for fn in list(events.values()) + list(host.values()):
            fn()
    torch.cuda.synchronize()

    def psnr(data):
        got = np.asarray(Image.open(io.BytesIO(data)).convert("RGB")).astype(np.float64)
        return 10 * np.log10(255.0 ** 2 / np.mean((got - page) ** 2))
    ours = host["jpeg hip/+copy"]().numpy().tobytes()
    psnr_ours, psnr_pil = psnr(ours), psnr(pil_jpeg())
    t = {k: [] for k in list(events) + list(host)}
    for _ in range(a.reps):
        for k, fn in events.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            t[k].append(e0.elapsed_time(e1))
        for k, fn in host.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            t[k].append((time.perf_counter() - t0) * 1e3)
    sizes["jpeg hip/kernels"], sizes["png hip/kernels"] = sizes["jpeg hip/+copy"], sizes["png hip/+copy"]
    lines = [f"# benchmarks/jpeg_time.py on {torch.cuda.get_device_name(0)}: one page {h} x {w} ({page.size} raw bytes), quality "
             f"{quality}, 4:{a.subsampling[1:2]}:{a.subsampling[2:]}, {a.reps} interleaved rounds after {a.warmup} warm-ups; */kernels by HIP "
             "events, the rest by the host clock",
             f"{'route':<18} {'median ms':>10} {'min ms':>10} {'max ms':>10} {'file bytes':>12}"]
    for k, ms in t.items():
        lines.append(f"{k:<18} {statistics.median(ms):>10.3f} {min(ms):>10.3f} {max(ms):>10.3f} {sizes[k]:>12d}")
    lines.append(f"# PSNR of the decoded file against the page: HIP jpeg {psnr_ours:.3f} dB, PIL jpeg {psnr_pil:.3f} dB; "
                 f"worst-case buffers: file {jcap} bytes, scratch {jscratch.numel()} bytes")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
