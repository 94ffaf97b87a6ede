"""Times getting ONE input photograph from a JPEG file's bytes to [H,W,3] uint8 RGB on the device, on one MI355X and its host:
the 3508 x 2480 page of benchmarks/png_time.py (`page_image`: a page-like picture plus 4 % uniform noise) and the same page
with exactly flat white margins (long runs that never self-synchronise: DESIGN.md 4.6), written by PIL at quality 90, 4:2:0,
no restart markers, through

  hip/decode      dvd_jpeg_decode_rgb8 with the file already on the device and preallocated buffers; host clock around the call
                  and a synchronise (the call itself reads 4 bytes back after every 16 fixpoint iterations and once after the
                  count pass, so HIP events around it would time the same span)
  hip/+upload     the same plus the host-to-device copy of the FILE (what env.image_decoder='hip' does, less the file system)
  PIL             Image.open + exif_transpose + convert('RGB') on the host (what env.image_decoder='pil' does in the loader)
  PIL/+upload     the same plus the host-to-device copy of the 26 MB of PIXELS

The routes are timed INTERLEAVED in one process after a warm-up of each; the table gives the median and the spread over --reps
rounds, the fixpoint's iteration count and whether the device's pixels equal PIL's.  Needs a GPU: there is no fallback.

    python benchmarks/jpegdec_time.py [--reps 7] [--out profiles/jpegdec_time.txt]
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
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import ctypes as C
    import numpy as np
    import torch
    from PIL import Image
    from dvd_amd import lib, ops
    from png_time import page_image
    if not torch.cuda.is_available():
        sys.exit("jpegdec_time.py needs a GPU: a time taken elsewhere says nothing")
    h, w = a.height, a.width
    noisy = page_image(h, w)
    margins = noisy.copy()
    my, mx = h // 12, w // 10
    margins[:my], margins[-my:], margins[:, :mx], margins[:, -mx:] = 255, 255, 255, 255
    lines = [f"# benchmarks/jpegdec_time.py on {torch.cuda.get_device_name(0)}: one page {h} x {w}, quality {a.quality}, 4:2:0, written "
             f"by PIL; {a.reps} interleaved rounds after {a.warmup} warm-ups; host clock",
             f"{'page':<14} {'route':<12} {'median ms':>10} {'min ms':>10} {'max ms':>10}"]
    for name, page in (("noisy", noisy), ("flat margins", margins)):
        buf = io.BytesIO()
        Image.fromarray(page).save(buf, format="JPEG", quality=a.quality, subsampling=2)
        data = buf.getvalue()
        host = np.frombuffer(bytearray(data), dtype=np.uint8)
        host_t = torch.from_numpy(host).pin_memory()
        info = ops.jpeg_probe(data)
        file_dev = host_t.cuda()
        out = torch.empty(3 * h * w, dtype=torch.uint8, device="cuda")
        scratch = torch.empty(info["scratch_bytes"], dtype=torch.uint8, device="cuda")
        iters = C.c_int(0)

        def hip_decode():
            rc = lib.raw().dvd_jpeg_decode_rgb8(host.ctypes.data, lib.ptr(file_dev), host.size, lib.ptr(out), out.numel(), 0,
                                                C.byref(iters), lib.ptr(scratch), lib.stream_ptr())
            assert rc == 0, lib.raw().dvd_last_error()
            torch.cuda.synchronize()

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
        for k, ms in t.items():
            lines.append(f"{name:<14} {k:<12} {statistics.median(ms):>10.3f} {min(ms):>10.3f} {max(ms):>10.3f}")
        lines.append(f"# {name}: file {len(data)} bytes, {info['scan_bytes'] // lib.JPEGDEC_SUBSEQ + 1} subsequences, {iters.value} fixpoint "
                     f"iterations, scratch {info['scratch_bytes']} bytes, pixels equal PIL's: {equal}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
