#!/usr/bin/env python3
"""Generate tests/golden/mapscore.npz by running the REAL reference's train_settings/validation/metrics_flow.py and
metrics_uncertainty.py (torch on the CPU) on small fields.

TEST INFRASTRUCTURE, like tests/tools/gen_flowviz_golden.py: it needs the reference tree, which the GPU machines do not have;
what it writes is committed.

    python tests/tools/gen_mapscore_golden.py --ref PATH

Both files are imported unmodified, as the package `validation` of <ref>/train_settings.  Per case `pred_<name>`, `gt_<name>`
[h,w,2] f32, `sigma_<name>` [h,w] f32 and what the reference makes of the valid pixels: `epe_`, `std_` (compute_epe),
`pck1_`, `pck3_`, `pck5_` (correct_correspondences / N), `fl_` (Fl_kitti_2015 / N), `sparse_`, `opt_` [3,51] and `ause_` [3]
(compute_aucs, intervals = 50; rows EPE, PCK1, PCK5), and `subs_` [2,50]: the sizes of the reference's kept sets.

  smooth    33 x 31   errors from sub-pixel to 8 px, sigma follows the error closely
  page      67 x 45   errors to 12 px, sigma = the error times a random factor
  invalid  100 x 75   a block of NaN, +-inf and 1e10 ground-truth pixels; sigma unrelated to the error
  anti      45 x 67   sigma falls where the error grows
  still     40 x 50   a ground truth with a region of exact zeros under errors above 3 px (Fl with m = 0)

Margin conditions, asserted here and again by the test: no e within 1e-4 of 1, 3 or 5; no e / m within 1e-4 (relative) of 0.05;
no two equal keys; the reference's kept sets have N - ceil(q (N - 1) / 100) pixels."""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(REPO, "tests"))
F = np.float32
METRICS = ("EPE", "PCK1", "PCK5")


def field(h, w, scale, seed):
    """[h,w,2] f32, smooth: a few low-frequency waves."""
    rng = np.random.default_rng(seed)
    ys, xs = np.meshgrid(np.linspace(0, 1, h), np.linspace(0, 1, w), indexing="ij")
    out = np.zeros((h, w, 2))
    for c in range(2):
        for _ in range(4):
            a, b, p = rng.uniform(-4, 4), rng.uniform(-4, 4), rng.uniform(0, 6.3)
            out[..., c] += rng.uniform(0.3, 1.0) * np.sin(a * xs + b * ys + p)
    return (scale * out / 2).astype(F)


def cases():
    rng = np.random.default_rng(11)
    out = {}

    def noise(shape, s):
        return rng.normal(0, s, shape).astype(F)
    gt = field(33, 31, 20, 1)
    pred = gt + field(33, 31, 6, 2) + noise(gt.shape, 0.3)
    out["smooth"] = [pred, gt, lambda e: e * rng.uniform(0.9, 1.1, e.shape) + 0.05]
    gt = field(67, 45, 40, 3)
    pred = gt + field(67, 45, 9, 4) + noise(gt.shape, 0.8)
    out["page"] = [pred, gt, lambda e: e * rng.uniform(0.3, 3.0, e.shape)]
    gt = field(100, 75, 60, 5)
    pred = gt + field(100, 75, 5, 6) + noise(gt.shape, 0.5)
    gt[10:30, 20:40, 0] = np.nan
    gt[30:35, 20:40, 1] = np.inf
    gt[35:40, 20:40, 0] = -np.inf
    gt[40:45, 20:40] = 1e10
    gt[45:47, 20:40, 1] = -2e9
    out["invalid"] = [pred, gt, lambda e: rng.uniform(0.0, 4.0, e.shape)]
    gt = field(45, 67, 30, 7)
    pred = gt + field(45, 67, 7, 8) + noise(gt.shape, 0.4)
    out["anti"] = [pred, gt, lambda e: 10.0 / (1.0 + e) + rng.uniform(0, 0.01, e.shape)]
    gt = field(40, 50, 2, 9)
    gt[5:25, 10:40] = 0.0
    pred = gt + field(40, 50, 8, 10) + noise(gt.shape, 0.2)
    out["still"] = [pred, gt, lambda e: e * rng.uniform(0.5, 2.0, e.shape)]
    return out


def margins_ok(e, m):
    with np.errstate(all="ignore"):
        near = np.zeros(e.shape, bool)
        for t in (1.0, 3.0, 5.0):
            near |= np.abs(e.astype(np.float64) - t) < 1e-4
        ratio = e.astype(np.float64) / m.astype(np.float64)
        near |= np.abs(ratio / 0.05 - 1) < 1e-4
    return ~near


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("DVD_REFERENCE", ""), help="reference checkout")
    a = ap.parse_args()
    if not a.ref:
        raise SystemExit("--ref PATH of the reference checkout is required")
    sys.path.insert(0, os.path.join(a.ref, "train_settings"))
    import torch
    import warnings
    from validation import metrics_flow as RF           # the reference's files, unmodified
    from validation import metrics_uncertainty as RU
    import mapscore_model as M
    warnings.simplefilter("ignore", DeprecationWarning)   # np.trapz in the reference
    out = {}
    for name, (pred, gt, sigma_of) in cases().items():
        for _ in range(20):                               # move the few pixels that sit on a threshold
            planes = M.errors(pred, gt)
            e = np.where(planes["valid"], planes["e"].view(F), F(0.5))
            bad = planes["valid"] & ~margins_ok(e, planes["m"])
            first = np.zeros(e.shape, bool)
            first[np.unique(e, return_index=True)[1]] = True
            bad |= planes["valid"] & ~first                 # and one of every two pixels with the same error
            if not bad.any():
                break
            pred.reshape(-1, 2)[bad, 0] += F(0.01)
        assert not bad.any(), name
        e = planes["e"].view(F).reshape(pred.shape[:2])
        sigma = np.where(planes["valid"].reshape(e.shape), sigma_of(np.nan_to_num(e.astype(np.float64))), 0.0).astype(F)
        ok = planes["valid"]
        n = int(ok.sum())
        for _ in range(20):                               # equal spreads: the later pixel moves up by one float
            flat = sigma.reshape(-1)
            first = np.zeros(flat.shape, bool)
            first[np.unique(flat, return_index=True)[1]] = True
            if not (ok & ~first).any():
                break
            flat[ok & ~first] = np.nextafter(flat[ok & ~first], F(np.inf))
        assert len(np.unique(sigma.ravel()[ok])) == n and len(np.unique(e.ravel()[ok])) == n, f"{name}: equal keys"
        p, g, s = (torch.from_numpy(x.reshape(-1, x.shape[-1] if x.ndim == 3 else 1)[ok].copy()) for x in (pred, gt, sigma))
        s = s[:, 0]
        epe, std = RF.compute_epe(p, g, mean=True, calculate_std=True)
        pck = {k: RF.correct_correspondences(p, g, alpha=float(k), img_size=1.0) / n for k in (1, 3, 5)}
        fl = RF.Fl_kitti_2015(p, g) / n
        aucs = RU.compute_aucs(g, p, s, intervals=50)
        # the sizes of the reference's kept sets, by its own two lines (metrics_uncertainty.py: thresholds, subs)
        subs = []
        for key in (-s, -torch.norm(g - p, p=2, dim=1)):
            thresholds = [np.percentile(key.cpu().numpy(), q) for q in [100. / 50 * t for t in range(0, 50)]]
            subs.append([int(key.ge(t).sum()) for t in thresholds])
        want = [n - hi for hi in M.ranks_desc(n)]
        assert subs[0] == want and subs[1] == want, f"{name}: the reference's kept sets are not N - hi"
        out[f"pred_{name}"], out[f"gt_{name}"], out[f"sigma_{name}"] = pred, gt, sigma
        out[f"epe_{name}"], out[f"std_{name}"] = np.float64(epe), np.float64(std)
        for k in (1, 3, 5):
            out[f"pck{k}_{name}"] = np.float64(pck[k])
        out[f"fl_{name}"] = np.float64(fl)
        out[f"sparse_{name}"] = np.asarray([aucs["sparse_curve"][m] for m in METRICS], np.float64)
        out[f"opt_{name}"] = np.asarray([aucs["opt_curve"][m] for m in METRICS], np.float64)
        out[f"ause_{name}"] = np.asarray([aucs["AUSE"][m] for m in METRICS], np.float64)
        out[f"subs_{name}"] = np.asarray(subs, np.int64)
        print(f"{name}: {pred.shape[0]} x {pred.shape[1]}, {n} valid, epe {epe:.4f} std {std:.4f} pck1 {pck[1]:.4f} pck5 {pck[5]:.4f} "
              f"fl {fl:.4f} AUSE {out[f'ause_{name}']}")
    path = os.path.join(REPO, "tests", "golden", "mapscore.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
