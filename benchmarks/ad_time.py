"""Times the aligned-distortion (AD) protocol for ONE pair on one MI355X: a 3508 x 2480 prediction against a 3508 x 2480 ground
truth, both resized to 598 400 pixels (920 x 650), gray, then the chain of DESIGN.md 4.8 at the SIFT-flow defaults:

  LD chain            ops.sift_flow: one SIFT-flow pass and LD (benchmarks/ld_time.py splits it further)
  AD chain            ops.aligned_distortion: flow 1, fit, align, flow 2, weighted mean; AD and LD read back (16 bytes)
  fit                 ops.ad_fit on the first flow: partial sums + finalize (sums and Q16 coefficients stay on the device)
  align               ops.ad_align: the page resampled through the fitted map
  weighted mean       ops.ad_weighted on the second flow: partials + finalize, AD read back (8 bytes)

The expectation to check is AD = 2 x the LD chain + the three small stages; the last lines give the measured ratio and the
remainder from the same run.  The routes are timed INTERLEAVED in one process, each call between two HIP events, after a warm-up
of all of them; the table gives the median and the spread over --reps calls.  Needs a GPU: there is no fallback.

    python benchmarks/ad_time.py [--out profiles/ad_time.txt]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from benchmarks.ld_time import time_interleaved  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=3508)
    ap.add_argument("--width", type=int, default=2480)
    ap.add_argument("--area", type=int, default=598400)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from dvd_amd import ops
    if not torch.cuda.is_available():
        sys.exit("ad_time.py needs a GPU: a time taken elsewhere says nothing")
    h, w = a.height, a.width
    gen = torch.Generator().manual_seed(0)
    gt = torch.randint(0, 256, (h, w, 3), generator=gen, dtype=torch.uint8).cuda()
    moved = torch.roll(gt, (11, -7), dims=(0, 1))                        # about (3, -2) pixels at the working size
    pred = (moved.float() * 0.8 + torch.randint(0, 52, (h, w, 3), generator=gen).cuda()).to(torch.uint8).contiguous()
    th, tw = ops.msssim_target_size(h, w, a.area)
    gx, gy = ops.resize_gray_u8(pred[None], th, tw), ops.resize_gray_u8(gt[None], th, tw)
    ad, ld, x = ops.aligned_distortion(gy, gx, intermediates=True)
    flow1, coef, flow2 = x["flow1"], x["coef"], x["flow2"]
    calls = {"LD chain (ops.sift_flow)": lambda: ops.sift_flow(gy, gx),
             "AD chain (ops.aligned_distortion)": lambda: ops.aligned_distortion(gy, gx),
             "fit (ops.ad_fit)": lambda: ops.ad_fit(flow1),
             "align (ops.ad_align)": lambda: ops.ad_align(gx, coef),
             "weighted mean (ops.ad_weighted)": lambda: ops.ad_weighted(gy, flow2)}
    t = time_interleaved(calls, a.reps, a.warmup)
    med = {k: statistics.median(v) for k, v in t.items()}
    lines = [f"# benchmarks/ad_time.py on {torch.cuda.get_device_name(0)}: one pair {h} x {w} -> {th} x {tw} ({th * tw} px), defaults "
             f"{ops.SFLOW_DEFAULTS}; {a.reps} interleaved calls per route after {a.warmup} warm-up(s), HIP events; each call includes "
             "the wrappers' allocations and read-backs",
             f"# of the pair: LD {float(ld[0]):.6f}, AD {float(ad[0]):.6f}, fitted map (ax, bx, ay, by) / 65536 = "
             f"{[round(v / 65536, 4) for v in coef[0].tolist()]}",
             f"{'route':<44} {'median ms':>10} {'min ms':>9} {'max ms':>9}"]
    for name, ms in t.items():
        lines.append(f"{name:<44} {med[name]:>10.3f} {min(ms):>9.3f} {max(ms):>9.3f}")
    ld_ms, ad_ms = med["LD chain (ops.sift_flow)"], med["AD chain (ops.aligned_distortion)"]
    small = sum(med[k] for k in ("fit (ops.ad_fit)", "align (ops.ad_align)", "weighted mean (ops.ad_weighted)"))
    lines.append(f"# AD chain / LD chain = {ad_ms / ld_ms:.3f}; AD chain - 2 x LD chain = {ad_ms - 2 * ld_ms:.3f} ms; the three stages "
                 f"alone = {small:.3f} ms")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
