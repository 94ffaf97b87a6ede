"""Times the corruption stage of the document loop on one MI355X: every delivered kind at severity 5 on 1 and on
32 documents of 512 x 512, HIP events around `ops.corrupt_rgb8` (the one launch, the allocation of its output and the upload of
the keys; for jpeg_compression the codec's launches and its read-back of each file's length), the two ends of the stage
(`unit_to_rgb8`, `rgb8_to_unit`) and, for scale, the pre-stage nets (`prestage.conditioning`, G = 64, synthetic weights) that
the stage feeds.  The routes are timed INTERLEAVED in one process after a warm-up of each; the table gives the median and the
spread over --reps rounds.  Needs a GPU: there is no fallback.

    python benchmarks/corrupt_time.py [--reps 9] [--out profiles/corrupt_time.txt]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--severity", type=int, default=5)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 32])
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import numpy as np
    import torch
    from dvd_amd import ops, prestage, synth
    if not torch.cuda.is_available():
        sys.exit("corrupt_time.py needs a GPU: a time taken elsewhere says nothing")
    tt = lambda sd: {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}  # noqa: E731
    dewarp, seg, line = prestage.GeoTr_Seg_Inf(), prestage.Seg(), prestage.UNet(n_channels=3, n_classes=1)
    dewarp.msk.load_state_dict(tt(synth.synth_convnet_state_dict("u2netp", 11)), strict=True)
    seg.load_state_dict(tt(synth.synth_convnet_state_dict("u2netp", 22, prefix="msk.")), strict=True)
    line.load_state_dict(tt(synth.synth_convnet_state_dict("unet", 13)), strict=True)
    for m in (dewarp, seg, line):
        m.to("cuda")
        m.eval()
    kinds = [k for k in range(len(ops.CORRUPTIONS)) if ops.corruption_supported(k)]
    routes = {}
    for b in a.batches:
        page = np.stack([(synth.smooth_image(f"ct/img{i}", 512, 512, 3 + i).transpose(1, 2, 0) * 255).astype(np.uint8) for i in range(b)])
        img = torch.from_numpy(np.ascontiguousarray(page)).cuda()
        y = ops.rgb8_to_unit(img)
        keys = [ops.corruption_key(1992, f"doc{i}") for i in range(b)]
        for k in kinds:
            routes[(ops.CORRUPTIONS[k], b)] = lambda k=k, img=img, keys=keys: ops.corrupt_rgb8(img, k, a.severity, keys)
        routes[("unit_to_rgb8", b)] = lambda y=y: ops.unit_to_rgb8(y)
        routes[("rgb8_to_unit", b)] = lambda img=img: ops.rgb8_to_unit(img)
        routes[("pre-stage nets", b)] = lambda y=y: prestage.conditioning(dewarp, seg, line, y, 64)
    for _ in range(a.warmup):
        for fn in routes.values():
            fn()
    torch.cuda.synchronize()
    t = {name: [] for name in routes}
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(a.reps):
        for name, fn in routes.items():
            start.record()
            fn()
            stop.record()
            stop.synchronize()
            t[name].append(start.elapsed_time(stop))
    lines = [f"# benchmarks/corrupt_time.py on {torch.cuda.get_device_name(0)}: documents of 512 x 512, severity {a.severity}; "
             f"{a.reps} interleaved rounds after {a.warmup} warm-ups; HIP events around each call, ms per call",
             f"{'route':<20} {'documents':>9} {'median ms':>10} {'min ms':>10} {'max ms':>10} {'ms / document':>14}"]
    for (name, b), ms in t.items():
        med = statistics.median(ms)
        lines.append(f"{name:<20} {b:>9} {med:>10.3f} {min(ms):>10.3f} {max(ms):>10.3f} {med / b:>14.4f}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
