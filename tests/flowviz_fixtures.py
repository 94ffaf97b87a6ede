"""What tests/test_flowviz_cpu.py and tests/test_gpu_flowviz.py share: the goldens of the real reference
(tests/golden/flowviz.npz, written by tests/tools/gen_flowviz_golden.py), the measured bars and the fields both files use."""
import os

import numpy as np

F = np.float32
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "flowviz.npz")
CASES = ("smooth", "sides", "anchors", "clip", "bgr")
# Share of the goldens' bytes on which the float32 model and the reference's float64 differ (by 1 at most).  An arithmetic good
# to e in `col` moves floor(255 col) on about 2 * 255 * e of the bytes: 5e-4 at e = 2^-20.  MEASURED on the five goldens with
# this model: 0 of 24231 bytes.  The bar is twice the measured share.
MEASURED_SHARE = 0.0
SHARE_BAR = 2 * MEASURED_SHARE
# Largest error of the float32 up-sampling against float64 from exact coordinates, in ulp of the map's largest magnitude
# (measured with this model; the float32 source coordinate scale * index dominates it).  The bar is twice the measured value.
# Against torch's CPU F.interpolate the model differs on no element: that comparison is equality.
UPSAMPLE_SHAPES = ((8, 45, 67), (16, 100, 75))
MEASURED_ULP = {(8, 45, 67): 7.7, (16, 100, 75): 15.2}


def golden(name):
    z = np.load(GOLD)
    clip = float(z[f"clip_{name}"])
    return z[f"field_{name}"], z[f"image_{name}"], None if np.isnan(clip) else clip, bool(z[f"bgr_{name}"])


def coarse_maps(g, n=2):
    return np.random.default_rng(g).uniform(-0.3, 0.3, (n, 2, g, g)).astype(F)


def odd_field(h, w, seed=0):
    """A field with lengths on both sides of either rad_max, and NaN and +-inf pixels where there is room."""
    f = np.random.default_rng(seed + 1000 * h + w).normal(0, 0.6 * max(h, w), (h, w, 2)).astype(F)
    flat = f.reshape(-1, 2)
    if len(flat) > 8:
        flat[1] = (np.nan, 1.0)
        flat[3] = (np.inf, -np.inf)
        flat[5] = (2.0, -np.inf)
        flat[7] = (0.0, 0.0)
    return f
