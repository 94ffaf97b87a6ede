"""The map score in NumPy: THE DEFINITION.  dvd_amd/csrc/mapscore_core.h is the same arithmetic for the kernels
of mapscore.hip and for the stand-alone CPU restatement mapscore_host_check.cpp.

A predicted map is scored against a ground-truth map at the ground truth's h x w: per valid pixel the end-point error
e = sqrt(du^2 + dv^2), the ground truth's length m and, with H >= 2 hypotheses, their spread sigma - all float32 with every
operation rounded on its own; then the reference's numbers (train_settings/validation/metrics_flow.py, metrics_uncertainty.py):
EPE, its unbiased standard deviation, PCK-1/3/5, Fl-KITTI-2015 and the sparsification curves with their AUSE.  Planes are handed
round as uint32 bit patterns: a non-negative finite float32 orders as its pattern, and an invalid pixel is 0xffffffff."""
import numpy as np

import flowviz_model as FV

F = np.float32
INVALID = np.uint32(0xffffffff)
UNKNOWN = F(1e9)                 # the Middlebury unknown-flow rule
INTERVALS = 50
FIX_CAP, FIX_SCALE = F(32768.0), F(1048576.0)     # e saturates at 2^15 px in the fixed-point sum: 2^28 px * 2^35 <= 2^63
METRICS = ("EPE", "PCK1", "PCK5")
NO_PIXELS = {"EPE": 0.0, "PCK1": 1.0, "PCK5": 1.0}


def _length(x, y):
    return np.sqrt((x * x).astype(F) + (y * y).astype(F)).astype(F)


def spread(hyp_fields):
    """[H,h,w,2] float32, H >= 2 -> (sigma [h,w] float32, ok [h,w]): sqrt((1/H) sum_h |d_h - mean|^2), sums over h = 0, 1, .."""
    d = np.asarray(hyp_fields, F)
    n = F(d.shape[0])
    with np.errstate(all="ignore"):
        total = np.zeros(d.shape[1:], F)
        for h in range(d.shape[0]):
            total = (total + d[h]).astype(F)
        mean = (total / n).astype(F)
        s = np.zeros(d.shape[1:3], F)
        for h in range(d.shape[0]):
            du, dv = (d[h, ..., 0] - mean[..., 0]).astype(F), (d[h, ..., 1] - mean[..., 1]).astype(F)
            s = (s + ((du * du).astype(F) + (dv * dv).astype(F)).astype(F)).astype(F)
        return np.sqrt((s / n).astype(F)).astype(F), np.isfinite(total).all(-1) & np.isfinite(s)


def errors(pred, gt, hyp_fields=None):
    """pred, gt [h,w,2] float32 displacement fields in pixels, hyp_fields [H,h,w,2] or None -> dict of flat arrays over the h w
    pixels: `e` and `sigma` (uint32 bit patterns, INVALID at an invalid pixel), `m` (float32) and `valid`."""
    pred, gt = np.asarray(pred, F), np.asarray(gt, F)
    assert pred.shape == gt.shape and pred.shape[-1] == 2
    with np.errstate(all="ignore"):
        valid = (np.isfinite(gt) & (np.abs(gt) <= UNKNOWN)).all(-1) & np.isfinite(pred).all(-1)
        if hyp_fields is not None and len(hyp_fields) >= 2:
            sigma, ok = spread(hyp_fields)
            valid &= ok
        else:
            sigma = np.zeros(pred.shape[:2], F)
        e = _length((gt[..., 0] - pred[..., 0]).astype(F), (gt[..., 1] - pred[..., 1]).astype(F))
        m = _length(gt[..., 0], gt[..., 1])
        valid &= np.isfinite(e)
    e_bits = np.where(valid, e.view(np.uint32), INVALID).ravel()
    s_bits = np.where(valid, sigma.view(np.uint32), INVALID).ravel()
    return {"e": e_bits, "sigma": s_bits, "m": m.ravel(), "valid": valid.ravel()}


def errors_of_maps(flow, gt, hyps, h, w):
    """The same from coarse maps: flow [2,G,G], hyps [H,2,G,G] or None, gt a field [h,w,2] or a coarse map [2,g,g]."""
    gt = np.asarray(gt, F)
    gt_field = gt if gt.shape == (h, w, 2) else FV.full_uv(gt, h, w)
    hyp_fields = None if hyps is None else np.stack([FV.full_uv(x, h, w) for x in hyps])
    return errors(FV.full_uv(flow, h, w), gt_field, hyp_fields)


def headline(planes):
    """The per-document numbers of the valid pixels: counts exact, sum e and sum e^2 in float64."""
    ok = planes["valid"]
    e = planes["e"][ok].view(F)
    m = planes["m"][ok]
    n = int(ok.sum())
    with np.errstate(all="ignore"):
        fl = int(((e > F(3)) & ((e / m).astype(F) > F(0.05))).sum())       # m = 0: e / m = inf, an outlier (the reference's)
    counts = {"n_valid": n, "n1": int((e <= F(1)).sum()), "n3": int((e <= F(3)).sum()), "n5": int((e <= F(5)).sum()), "n_fl": fl}
    e64 = e.astype(np.float64)
    return counts, float(e64.sum()), float((e64 * e64).sum())


def metrics_of(counts, se, se2):
    """(counts, sum e, sum e^2) -> epe, epe_std (unbiased, torch.std), pck1/3/5, fl, n_valid and the two sums.  No valid pixel:
    NaN; one: epe_std is NaN, as torch.std's."""
    n = counts["n_valid"]
    nan = float("nan")
    if n == 0:
        return {"epe": nan, "epe_std": nan, "pck1": nan, "pck3": nan, "pck5": nan, "fl": nan, "n_valid": 0, "sum_e": 0.0, "sum_e2": 0.0}
    var = max(se2 - se * se / n, 0.0) / (n - 1) if n > 1 else nan
    return {"epe": se / n, "epe_std": float(np.sqrt(var)), "pck1": counts["n1"] / n, "pck3": counts["n3"] / n,
            "pck5": counts["n5"] / n, "fl": counts["n_fl"] / n, "n_valid": n, "sum_e": se, "sum_e2": se2}


def ranks_desc(n_valid, intervals=INTERVALS):
    """hi = ceil(q (N - 1) / 100) for q = 0, 100 / intervals, ..: the descending rank whose key closes the kept set."""
    step = 100 // intervals
    return [(q * (n_valid - 1) + 99) // 100 for q in range(0, 100, step)]


def select_desc(keys, ranks):
    """keys uint32 (INVALID ones sort first in descending order and are skipped) -> keys_desc[ranks] among the valid ones."""
    valid = np.sort(keys[keys != INVALID])[::-1]
    return valid[np.asarray(ranks, np.int64)]


def fixed_of(e):
    return np.rint(np.minimum(e, FIX_CAP) * FIX_SCALE).astype(np.uint64)


def bins_of(e_bits, key_bits, thr):
    """[len(thr) + 1, 4] uint64: bin b = the valid pixels whose key is <= exactly b of the (non-increasing) thresholds:
    count, #(e <= 1), #(e <= 5), sum of rint(min(e, 2^15) 2^20)."""
    ok = e_bits != INVALID
    e, key = e_bits[ok].view(F), key_bits[ok]
    thr = np.asarray(thr, np.uint32)
    b = len(thr) - np.searchsorted(thr[::-1], key, side="left")          # how many thresholds are >= key
    out = np.zeros((len(thr) + 1, 4), np.uint64)
    fix = fixed_of(e)
    for j in range(len(thr) + 1):
        sel = b == j
        out[j] = (sel.sum(), (sel & (e <= F(1))).sum(), (sel & (e <= F(5))).sum(), fix[sel].sum(dtype=np.uint64))
    return out


def kept_sets(bins):
    """[k + 1, 4] bins -> [k, 4]: set j keeps the bins j + 1 .. k (suffix sums)."""
    return np.cumsum(bins[::-1].astype(np.uint64), axis=0, dtype=np.uint64)[::-1][1:]


def curve_of(kept):
    """[k, 4] integer sums of the kept sets -> {metric: k + 1 float64 values}, the value for no pixel appended."""
    cnt = kept[:, 0].astype(np.float64)
    vals = {"EPE": kept[:, 3].astype(np.float64) / float(FIX_SCALE) / cnt, "PCK1": kept[:, 1] / cnt, "PCK5": kept[:, 2] / cnt}
    return {m: np.append(vals[m], NO_PIXELS[m]) for m in METRICS}


def trapz(y, x):
    y, x = np.asarray(y, np.float64), np.asarray(x, np.float64)
    return float(((y[1:] + y[:-1]) * 0.5 * np.diff(x)).sum())


def ause_of(sparse, opt):
    """The reference's compute_aucs tail: both curves over max(opt) + 1e-6, AUSE = |trapz(sparse) - trapz(opt)|."""
    k = len(sparse["EPE"]) - 1
    plotx = [1.0 / k * t for t in range(k + 1)]
    out = {"sparse_curve": {}, "opt_curve": {}, "AUSE": {}}
    for m in METRICS:
        top = np.asarray(opt[m]).max() + 1e-6
        out["AUSE"][m] = abs(trapz(sparse[m] / top, plotx) - trapz(opt[m] / top, plotx))
        out["sparse_curve"][m], out["opt_curve"][m] = sparse[m] / top, opt[m] / top
    return out


def sparsification(e_bits, sigma_bits, detail=False):
    """The sparsification curves of compute_aucs(intervals = 50): the kept set of q is {p : key(p) <= key_desc[hi]}, hi =
    ceil(q (N - 1) / 100), all ties kept; key = sigma gives the method's curve, key = e the oracle's.

    This is what np.percentile(-key, q) followed by `ge` selects unless the reference's float32 interpolation
    a + (b - a) frac between the order statistics a < b of -key rounds down onto a: then the reference keeps the pixels of a as
    well (N - floor(r) of them, not N - hi).  That is the one case where the two part."""
    n = int((e_bits != INVALID).sum())
    ranks = ranks_desc(n)
    got = {}
    for name, keys in (("sparse", sigma_bits), ("opt", e_bits)):
        thr = select_desc(keys, ranks)
        bins = bins_of(e_bits, keys, thr)
        got[name] = (thr, bins, kept_sets(bins))
    out = ause_of(curve_of(got["sparse"][2]), curve_of(got["opt"][2]))
    if detail:
        out["detail"] = got
    return out


def score(planes, sparsify=True):
    """Everything of one document from its planes (`errors`): the headline numbers and, unless sparsify is False (H = 1) or no
    pixel is valid, sparse_curve, opt_curve, AUSE and ause_epe / ause_pck1 / ause_pck5."""
    out = metrics_of(*headline(planes))
    if sparsify and out["n_valid"] > 0:
        sp = sparsification(planes["e"], planes["sigma"])
        out.update(sp)
        out.update({f"ause_{m.lower()}": sp["AUSE"][m] for m in METRICS})
    return out
