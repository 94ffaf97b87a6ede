#!/usr/bin/env python3
"""Generate tests/golden/flowviz.npz by running the REAL reference's datasets/utils/flow_viz.py (pure NumPy) on the CPU.

TEST INFRASTRUCTURE, like tests/tools/gen_clip_golden.py: it needs the reference tree, which the GPU machines do not have;
what it writes is committed.

    python tests/tools/gen_flowviz_golden.py --ref PATH

The reference's file is loaded unmodified, by its path.  Every field is stored as float32 and handed to the reference as
float64, so that its arithmetic is float64 whatever NumPy's promotion rules of the day make of a float32 array and a float64
scalar.  Per case `field_<name>` [h,w,2] f32, `image_<name>` [h,w,3] u8, `clip_<name>` (NaN = None), `bgr_<name>`:

  smooth    37 x 53, a smooth field from sub-pixel to 10 px
  sides     64 x 48, radii on both sides of 1 after the 'diag' normalisation (rad_max = 40): up to 70 px
  anchors   6 x 10: column 0 and 9 zero, columns 1..8 the four axes and the four diagonals; rows = the lengths 0.25, 0.5, 1,
            2, 3 and, in the last row, length 1 with NEGATIVE zeros on the axes (arctan2 tells them apart).  All inside the
            unit radius: outside it a blend on an exact angle times 0.75 can be an exact integer over 255 (88 * 0.75 = 66 at
            fk = 40.5), where the reference's own last bit decides the byte.
  clip      37 x 53 with components from -6 to 8 and clip_flow = 3.0 (negative components become 0: the reference's quirk)
  bgr       33 x 31, convert_to_bgr = True

No golden pixel may have |rad - 1| < 1e-4 in the reference's float64: at that discontinuity a last-bit difference flips the
whole byte, and no rounding model is being tested there."""
import argparse
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.dont_write_bytecode = True


def smooth(h, w, lo, hi, phase=0.0):
    """[h,w,2] f32: direction turns smoothly over the image, length runs from lo to hi."""
    ys, xs = np.meshgrid(np.linspace(0, 1, h), np.linspace(0, 1, w), indexing="ij")
    ang = 2 * np.pi * (xs + 0.37 * ys + phase) + 0.8 * np.sin(3 * ys)
    length = lo + (hi - lo) * (0.5 + 0.5 * np.sin(2.3 * xs + 4.1 * ys + phase)) ** 2
    return np.stack([length * np.cos(ang), length * np.sin(ang)], axis=-1).astype(np.float32)


def anchors():
    s = np.float32(np.sqrt(0.5))
    dirs = [(1, 0), (0, 1), (-1, 0), (0, -1), (s, s), (-s, s), (-s, -s), (s, -s)]
    lengths = [0.25, 0.5, 1.0, 2.0, 3.0, 1.0]
    f = np.zeros((6, 10, 2), np.float32)
    for r, m in enumerate(lengths):
        for c, (dx, dy) in enumerate(dirs):
            f[r, 1 + c] = (np.float32(m) * np.float32(dx), np.float32(m) * np.float32(dy))
    f[5][f[5] == 0] = -0.0
    f[5, 0] = f[5, 9] = 0.0
    return f


def cases():
    clip = smooth(37, 53, 0.5, 8.0, phase=0.2)
    clip[..., 1] -= 2.0
    return {
        "smooth": (smooth(37, 53, 0.05, 10.0), None, False),
        "sides": (smooth(64, 48, 2.0, 70.0, phase=0.5), None, False),
        "anchors": (anchors(), None, False),
        "clip": (clip, 3.0, False),
        "bgr": (smooth(33, 31, 0.1, 12.0, phase=0.7), None, True),
    }


def reference_radius(field, clip):
    """rad as the reference's float64 has it (flow_to_image + flow_uv_to_colors)."""
    f = field.astype(np.float64)
    if clip is not None:
        f = np.clip(f, 0, clip)
    rad_max = np.sqrt(np.square(f.shape[1] // 2) + np.square(f.shape[0] // 2)) + 1e-5
    return np.sqrt(np.square(f[..., 0] / rad_max) + np.square(f[..., 1] / rad_max))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("DVD_REFERENCE", ""), help="reference checkout")
    a = ap.parse_args()
    if not a.ref:
        raise SystemExit("--ref PATH of the reference checkout is required")
    spec = importlib.util.spec_from_file_location("reference_flow_viz", os.path.join(a.ref, "datasets", "utils", "flow_viz.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    out = {}
    for name, (field, clip, bgr) in cases().items():
        rad = reference_radius(field, clip)
        assert np.abs(rad - 1).min() >= 1e-4, (name, float(np.abs(rad - 1).min()))
        image = ref.flow_to_image(field.astype(np.float64), clip_flow=clip, convert_to_bgr=bgr)
        assert image.dtype == np.uint8 and image.shape == field.shape[:2] + (3,)
        out[f"field_{name}"], out[f"image_{name}"] = field, image
        out[f"clip_{name}"], out[f"bgr_{name}"] = np.float64(np.nan if clip is None else clip), np.bool_(bgr)
        print(f"{name}: {field.shape[0]} x {field.shape[1]}, rad {rad.min():.4f} .. {rad.max():.4f}, "
              f"{int((rad > 1).sum())} of {rad.size} pixels beyond 1")
    rad = reference_radius(*cases()["sides"][:2])
    assert (rad > 1).mean() > 0.1 and (rad < 1).mean() > 0.1, "the 'sides' field must lie on both sides of rad = 1"
    path = os.path.join(REPO, "tests", "golden", "flowviz.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
