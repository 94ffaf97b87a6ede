"""What tests/test_mapscore_cpu.py and tests/test_gpu_mapscore.py share: the goldens of the real reference
(tests/golden/mapscore.npz, written by tests/tools/gen_mapscore_golden.py), the measured bars, the hostile key sets of the
selection and the fields both files use."""
import os

import numpy as np

import mapscore_model as M

F = np.float32
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mapscore.npz")
CASES = ("smooth", "page", "invalid", "anti", "still")
# The model (float64 sums of float32 errors, fixed-point sums for the curves) against the reference (float32 throughout), MEASURED
# on the five goldens: EPE 7.6e-8 and std 4.8e-8 relative; curve values 2.6e-7 and AUSE 4.7e-8 absolute (both are normalised to
# about 1).  Counts (PCK, Fl, the sizes of the kept sets) are equal.  The bars are four times the measured values.
MEASURED = {"epe_rel": 7.6e-8, "std_rel": 4.8e-8, "curve_abs": 2.6e-7, "ause_abs": 4.7e-8}
BARS = {k: 4 * v for k, v in MEASURED.items()}
SUM_REL = 1e-9          # two float64 sums of the same float32 terms in different orders
ODD_SHAPES = ((1, 1), (1, 67), (67, 1), (33, 31), (257, 263))


def golden(name):
    """(pred, gt, sigma, {what the reference computed})."""
    z = np.load(GOLD)
    ref = {k: z[f"{k}_{name}"] for k in ("epe", "std", "pck1", "pck3", "pck5", "fl", "sparse", "opt", "ause", "subs")}
    return z[f"pred_{name}"], z[f"gt_{name}"], z[f"sigma_{name}"], ref


def golden_planes(name):
    """The model's planes of a golden, the golden's sigma field standing for the hypotheses' spread."""
    pred, gt, sigma, ref = golden(name)
    planes = M.errors(pred, gt)
    planes["sigma"] = np.where(planes["valid"], sigma.ravel().view(np.uint32), M.INVALID)
    return planes, ref


def margins_hold(planes):
    """No e within 1e-4 of 1, 3, 5; no e / m within 1e-4 relative of 0.05 (the conditions the goldens were made under)."""
    ok = planes["valid"]
    e, m = planes["e"][ok].view(F).astype(np.float64), planes["m"][ok].astype(np.float64)
    with np.errstate(all="ignore"):
        return all(np.abs(e - t).min() >= 1e-4 for t in (1.0, 3.0, 5.0)) and np.abs(e / m / 0.05 - 1).min() >= 1e-4


def check_against_reference(got, ref):
    """A score dict (the model's or the kernels') against a golden's reference values under the measured bars."""
    for k in ("pck1", "pck3", "pck5", "fl"):
        assert got[k] == float(ref[k]), k
    assert abs(got["epe"] / float(ref["epe"]) - 1) <= BARS["epe_rel"]
    assert abs(got["epe_std"] / float(ref["std"]) - 1) <= BARS["std_rel"]
    for i, m in enumerate(M.METRICS):
        assert np.abs(np.asarray(got["sparse_curve"][m]) - ref["sparse"][i]).max() <= BARS["curve_abs"], m
        assert np.abs(np.asarray(got["opt_curve"][m]) - ref["opt"][i]).max() <= BARS["curve_abs"], m
        assert abs(got["AUSE"][m] - ref["ause"][i]) <= BARS["ause_abs"], m


def check_against_model(got, want):
    """A score dict of the kernels against the model's: counts and integer-derived values equal, float64 sums within SUM_REL."""
    assert got["n_valid"] == want["n_valid"]
    for k in ("pck1", "pck3", "pck5", "fl"):
        assert got[k] == want[k] or (np.isnan(got[k]) and np.isnan(want[k])), k
    for k in ("sum_e", "sum_e2"):
        assert abs(got[k] - want[k]) <= SUM_REL * abs(want[k]), (k, got[k], want[k])
    n = want["n_valid"]
    if n:
        assert abs(got["epe"] - want["epe"]) <= SUM_REL * want["epe"]
    if n > 1:
        # epe_std from sums good to SUM_REL: the variance moves by at most d, the root by d / std or, near 0, by sqrt(d)
        d = SUM_REL * (want["sum_e2"] + 2 * want["sum_e"] ** 2 / n) / (n - 1)
        tol = np.sqrt(d) if want["epe_std"] ** 2 <= d else d / want["epe_std"]
        assert abs(got["epe_std"] - want["epe_std"]) <= tol, (got["epe_std"], want["epe_std"], tol)
    else:
        assert np.isnan(got["epe_std"]) and (n or np.isnan(got["epe"]))
    assert ("AUSE" in got) == ("AUSE" in want)
    if "AUSE" in want:
        for m in M.METRICS:
            assert np.array_equal(np.asarray(got["sparse_curve"][m]), want["sparse_curve"][m]), m
            assert np.array_equal(np.asarray(got["opt_curve"][m]), want["opt_curve"][m]), m
            assert got["AUSE"][m] == want["AUSE"][m], m


def key_sets():
    """{name: uint32 keys}: the hostile inputs of the selection.  Values are bit patterns of non-negative finite float32, or
    INVALID."""
    rng = np.random.default_rng(5)
    base = np.uint32(0x40a00000)                                             # 5.0
    sets = {
        "all_equal": np.full(1000, base, np.uint32),
        "two_values": np.where(rng.random(1500) < 0.3, base, np.uint32(0x3f800000)).astype(np.uint32),
        "low_byte": (base + rng.integers(0, 256, 3000).astype(np.uint32)).astype(np.uint32),
        "top24_groups": ((rng.integers(0, 7, 4000).astype(np.uint32) * np.uint32(0x01010100) + np.uint32(0x3e000000))
                         + rng.integers(0, 256, 4000).astype(np.uint32)).astype(np.uint32),
        "single": np.asarray([0x3fc00000], np.uint32),
        "few": rng.uniform(0, 9, 17).astype(F).view(np.uint32),
        "zeros": np.zeros(700, np.uint32),
        "random": rng.uniform(0, 100, 70001).astype(F).view(np.uint32),
    }
    holes = rng.uniform(0, 9, 2500).astype(F).view(np.uint32).copy()
    holes[rng.random(2500) < 0.4] = M.INVALID
    sets["with_invalid"] = holes
    return sets


def smooth_maps(g, n, seed, amp=0.3):
    """n coarse maps [n,2,g,g] in [-amp, amp], smooth enough to be a plausible backward map."""
    rng = np.random.default_rng(seed)
    ys, xs = np.meshgrid(np.linspace(0, 1, g), np.linspace(0, 1, g), indexing="ij")
    out = np.zeros((n, 2, g, g))
    for i in range(n):
        for c in range(2):
            a, b, p = rng.uniform(-3, 3, 3)
            out[i, c] = amp * np.sin(a * xs + b * ys + p) * rng.uniform(0.3, 1.0)
    return out.astype(F)


def document(h, w, g=8, n_hyp=3, seed=0, holes=True):
    """(flow [2,g,g], gt field [h,w,2], hyps [n_hyp,2,g,g]) of one synthetic document; the ground truth is the field of a map up
    to about 6 px away (errors on both sides of 1, 3 and 5 px), with a few unknown pixels where there is room; the hypotheses
    lie up to about 3 px around the prediction."""
    maps = smooth_maps(g, 2 + n_hyp, 100 * h + w + seed)
    import flowviz_model as FV
    px = F(1.0 / (0.3 * max(h, w, 2)))                       # one pixel of the longer side, per unit of a smooth map
    gt = FV.full_uv((maps[0] + F(6) * px * maps[1]).astype(F), h, w).copy()
    flat = gt.reshape(-1, 2)
    if holes and len(flat) > 8:
        flat[1] = (np.nan, 1.0)
        flat[3] = (np.inf, -np.inf)
        flat[5] = (2e9, 0.0)
        flat[7] = (0.0, 0.0)
    hyps = (maps[0][None] + F(3) * px * maps[2:]).astype(F)
    return maps[0], gt, hyps
