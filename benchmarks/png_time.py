"""Times the PNG write of ONE dewarped page on one MI355X and its host: a 3508 x 2480 page,
    page = uint8(255 * clip(synth.smooth_image("png_time/page", H, W) + 0.04 * (uniform01("png_time/noise") - 0.5), 0, 1))
(the page-like picture of dvd_amd/synth.py, its own 6 % texture plus 4 % of extra uniform noise), through

  hip/kernels   ops.png_encode's four launches into preallocated buffers (dvd_png_encode_rgb8_huff, fixed blocks), HIP events
  hip/dynamic   the same four launches with DVD_PNG_HUFFMAN_DYNAMIC (per segment the smaller of a dynamic and the fixed block),
                HIP events
  hip/+copy     hip/kernels plus the length read-back and the device-to-host copy of the compressed bytes only, host clock
                around a call that ends in the copy's synchronise
  hip/dyn+copy  the same for hip/dynamic
  PIL level 6   the device-to-host copy of the 26 MB page + Image.save(compress_level=6) into memory (what env.png_encoder='pil'
                does, less the file system), host clock
  PIL level 1   the same at compress_level=1

The routes are timed INTERLEAVED in one process after a warm-up of each; the table gives the median and the spread over --reps
rounds and the file sizes beside the times.  It also prints the size ratios of both block types against PIL level 1 for the
page, an all-zero page and a uniform-random page of --small-side pixels square.  Needs a GPU: there is no fallback.

    python benchmarks/png_time.py [--reps 5] [--out profiles/png_time.txt]
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


def page_image(h, w):
    import numpy as np
    from dvd_amd import synth
    img = synth.smooth_image("png_time/page", h, w).transpose(1, 2, 0)
    noise = synth.uniform01("png_time/noise", h * w * 3).reshape(h, w, 3)
    return (255.0 * np.clip(img + 0.04 * (noise - 0.5), 0.0, 1.0)).astype(np.uint8)


def pil_bytes(arr, level):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, format="PNG", compress_level=level)
    return buf.getvalue()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=3508)
    ap.add_argument("--width", type=int, default=2480)
    ap.add_argument("--small-side", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import numpy as np
    import torch
    from dvd_amd import lib, ops
    if not torch.cuda.is_available():
        sys.exit("png_time.py needs a GPU: a time taken elsewhere says nothing")
    h, w = a.height, a.width
    page = page_image(h, w)
    dev = torch.from_numpy(page).cuda()
    cap = ops.png_bound(h, w)
    out = torch.empty(cap, dtype=torch.uint8, device="cuda")
    nbytes = torch.zeros(1, dtype=torch.int64, device="cuda")
    scratch = torch.empty(ops._size_query("dvd_png_scratch_bytes_huff", h, w, lib.PNG_HUFFMAN_DYNAMIC), dtype=torch.uint8,
                          device="cuda")
    sizes = {}

    def kernels(huffman=lib.PNG_HUFFMAN_FIXED):
        lib.call("dvd_png_encode_rgb8_huff", lib.ptr(dev), h, w, lib.ptr(out), cap, lib.ptr(nbytes), lib.ptr(scratch), huffman,
                 lib.stream_ptr())

    def kernels_dynamic():
        kernels(lib.PNG_HUFFMAN_DYNAMIC)

    def hip_copy(huffman=lib.PNG_HUFFMAN_FIXED, key="hip"):
        kernels(huffman)
        data = out[:int(nbytes.item())].cpu()
        sizes[key] = data.numel()
        return data

    def hip_dyn_copy():
        return hip_copy(lib.PNG_HUFFMAN_DYNAMIC, "hipdyn")

    def pil(level):
        def run():
            sizes[f"pil{level}"] = len(pil_bytes(dev.cpu().numpy(), level))
        return run

    events = {"hip/kernels": kernels, "hip/dynamic": kernels_dynamic}
    host = {"hip/+copy": hip_copy, "hip/dyn+copy": hip_dyn_copy, "PIL level 6": pil(6), "PIL level 1": pil(1)}
    for _ in range(a.warmup):
        for fn in list(events.values()) + list(host.values()):
            fn()
    torch.cuda.synchronize()
    from PIL import Image
    for fn in (hip_copy, hip_dyn_copy):
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(fn().numpy().tobytes()))), page), "the file does not decode to the page"
    t = {**{k: [] for k in events}, **{k: [] for k in host}}
    for _ in range(a.reps):
        for k, fn in events.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
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
    size_of = {"hip/kernels": sizes["hip"], "hip/dynamic": sizes["hipdyn"], "hip/+copy": sizes["hip"], "hip/dyn+copy": sizes["hipdyn"],
               "PIL level 6": sizes["pil6"], "PIL level 1": sizes["pil1"]}
    lines = [f"# benchmarks/png_time.py on {torch.cuda.get_device_name(0)}: one page {h} x {w} ({page.size} raw bytes), "
             f"{a.reps} interleaved rounds after {a.warmup} warm-up; hip/kernels and hip/dynamic by HIP events, the rest by the host clock",
             f"{'route':<14} {'median ms':>10} {'min ms':>10} {'max ms':>10} {'file bytes':>12}"]
    for k, ms in t.items():
        lines.append(f"{k:<14} {statistics.median(ms):>10.2f} {min(ms):>10.2f} {max(ms):>10.2f} {size_of[k]:>12d}")
    n = a.small_side
    small = {"page": page, "all-zero": np.zeros((n, n, 3), np.uint8),
             "uniform-random": np.random.RandomState(0).randint(0, 256, (n, n, 3)).astype(np.uint8)}
    lines.append("# file bytes: HIP fixed / PIL level 1, HIP dynamic / PIL level 1")
    for k, img in small.items():
        hip_n = ops.png_encode(torch.from_numpy(img).cuda()).numel()
        dyn_n = ops.png_encode(torch.from_numpy(img).cuda(), huffman="dynamic").numel()
        pil_n = len(pil_bytes(img, 1))
        lines.append(f"{k:<14} {img.shape[0]} x {img.shape[1]}: {hip_n} / {pil_n} = {hip_n / pil_n:.3f}, "
                     f"{dyn_n} / {pil_n} = {dyn_n / pil_n:.3f}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
