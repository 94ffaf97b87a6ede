"""Times the MS-SSIM protocol for ONE pair on one MI355X: a 3508 x 2480 prediction against a 3508 x 2480 ground truth, both
resized to 598 400 pixels (920 x 650), gray, five scales (ops.ms_ssim_u8 without its final read-back):

  hip       ops.resize_gray_u8 x 2 + ops.ssim_scales                       (dvd_amd/csrc/metrics.hip)
  hip/ssim  ops.ssim_scales alone on the two gray planes
  torch     a plain-torch restatement of the five scales on the same device: F.conv2d with the separable window on the five
            moment planes, the rationals and the means as tensor expressions, the reduce as F.conv2d with stride 2

The routes are timed INTERLEAVED in one process (hip, hip/ssim, torch, hip, ...), each call between two HIP events, after a
warm-up of all of them; the table gives the median and the spread over --reps calls.  The torch route has no resize (torch has
no anti-aliased triangle resize with this rounding), so it is to be read against hip/ssim.  Needs a GPU: there is no fallback.

    python benchmarks/msssim_time.py [--preset docunet] [--out profiles/msssim_time.txt]
"""
import argparse
import math
import os
import statistics
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def torch_scales(x, y, preset):
    """[N,H,W] f32 planes -> [N,5,2]: the definition of DESIGN 4.3 in ATen calls."""
    import torch
    import torch.nn.functional as F
    d = torch.arange(11, dtype=torch.float64) - 5.0
    g = torch.exp(-(d * d) / 4.5)
    g = (g / g.sum()).float().to(x.device)
    valid = preset == "wang"
    red = (torch.tensor([0.5, 0.5]) if valid else torch.tensor([1.0, 4.0, 6.0, 4.0, 1.0]) / 16.0).to(x.device)

    def blur(p):                                    # p [M,1,H,W]
        if not valid:
            p = F.pad(p, (5, 5, 5, 5), mode="replicate")
        return F.conv2d(F.conv2d(p, g.view(1, 1, 1, 11)), g.view(1, 1, 11, 1))

    def reduce2(p):
        h, w = p.shape[-2:]
        if valid:
            p = F.pad(p, (0, w % 2, 0, h % 2), mode="replicate")
        else:
            p = F.pad(p, (2, 2 - (w + 1) % 2, 2, 2 - (h + 1) % 2), mode="replicate")
        k = red.numel()
        return F.conv2d(F.conv2d(p, red.view(1, 1, 1, k), stride=(1, 2)), red.view(1, 1, k, 1), stride=(2, 1))

    c1, c2 = 6.5025, 58.5225
    x, y = x[:, None], y[:, None]
    out = []
    for s in range(5):
        a, b = x - 127.5, y - 127.5
        mx, my, exx, eyy, exy = blur(a), blur(b), blur(a * a), blur(b * b), blur(a * b)
        cs = (2 * (exy - mx * my) + c2) / ((exx - mx * mx) + (eyy - my * my) + c2)
        ux, uy = mx + 127.5, my + 127.5
        ssim = cs * (2 * ux * uy + c1) / (ux * ux + uy * uy + c1)
        out.append(torch.stack([ssim.mean(dim=(1, 2, 3)), cs.mean(dim=(1, 2, 3))], -1))
        if s < 4:
            x, y = reduce2(x), reduce2(y)
    return torch.stack(out, 1)


def time_interleaved(calls, reps, warmup):
    import torch
    for _ in range(warmup):
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()
    events = {k: [] for k in calls}
    for _ in range(reps):
        for k, fn in calls.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            events[k].append((a, b))
    torch.cuda.synchronize()
    return {k: [a.elapsed_time(b) for a, b in v] for k, v in events.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=3508)
    ap.add_argument("--width", type=int, default=2480)
    ap.add_argument("--area", type=int, default=598400)
    ap.add_argument("--preset", default="docunet", choices=("docunet", "wang"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from dvd_amd import ops
    if not torch.cuda.is_available():
        sys.exit("msssim_time.py needs a GPU: a time taken elsewhere says nothing")
    h, w = a.height, a.width
    gen = torch.Generator().manual_seed(0)
    gt = torch.randint(0, 256, (h, w, 3), generator=gen, dtype=torch.uint8).cuda()
    pred = (gt.float() * 0.8 + torch.randint(0, 52, (h, w, 3), generator=gen).cuda()).to(torch.uint8).contiguous()
    th, tw = ops.msssim_target_size(h, w, a.area)
    gx, gy = ops.resize_gray_u8(pred[None], th, tw), ops.resize_gray_u8(gt[None], th, tw)

    def hip():
        return ops.ssim_scales(ops.resize_gray_u8(pred[None], th, tw), ops.resize_gray_u8(gt[None], th, tw), a.preset)

    calls = {"hip (resize + gray + 5 scales)": hip,
             "hip/ssim (5 scales)": lambda: ops.ssim_scales(gx, gy, a.preset),
             "torch (5 scales)": lambda: torch_scales(gx, gy, a.preset)}
    diff = float((calls["hip/ssim (5 scales)"]() - calls["torch (5 scales)"]()).abs().max())
    t = time_interleaved(calls, a.reps, a.warmup)
    lines = [f"# benchmarks/msssim_time.py on {torch.cuda.get_device_name(0)}: one pair {h} x {w} -> {th} x {tw} "
             f"({th * tw} px), preset {a.preset}; {a.reps} interleaved calls per route after {a.warmup} warm-ups, HIP events; "
             "each call includes the wrappers' allocations and no read-back",
             f"# largest difference of the ten numbers between hip/ssim and torch: {diff:.2e}",
             f"{'route':<34} {'median ms':>10} {'min ms':>9} {'max ms':>9}"]
    for name, ms in t.items():
        lines.append(f"{name:<34} {statistics.median(ms):>10.3f} {min(ms):>9.3f} {max(ms):>9.3f}")
    text = "\n".join(lines)
    print(text)
    assert math.isfinite(diff)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
