"""Flow visualisation at the reference's path, with its three names and signatures (datasets/utils/flow_viz.py):

    make_colorwheel()                                        -> [55, 3] float64, the Middlebury wheel
    flow_uv_to_colors(u, v, convert_to_bgr=False)            -> [H, W, 3] uint8 of NORMALISED components (radius 1 = full colour)
    flow_to_image(flow_uv, clip_flow=None, convert_to_bgr=False)   -> [H, W, 3] uint8 of a displacement field [H, W, 2]

The wheel is written from its published description (Baker et al., "A Database and Evaluation Methodology for Optical Flow",
ICCV 2007): 55 entries in six segments between red, yellow, green, cyan, blue and magenta.  The colours are computed on the
device by `dvd_amd.ops.flow_to_image` (dvd_flow_to_image_rgb8): NumPy in gives NumPy out, a CUDA tensor in
gives a device tensor out.  `flow_to_image` takes one more keyword, `norm`: 'diag' (the reference's rad_max, the default) |
'max' (the Middlebury rule).  Nothing of dvd_amd is imported until a function is called."""
from __future__ import annotations

import numpy as np

WHEEL_SEGMENTS = (("RY", 15), ("YG", 6), ("GC", 4), ("CB", 11), ("BM", 13), ("MR", 6))


def make_colorwheel():
    """[55, 3] float64.  Segment by segment one channel ramps by floor(255 i / n) - up from the first primary to the mixed
    colour, then the other one down to the next primary - while the remaining channels stay at 0 or 255."""
    wheel = np.zeros((sum(n for _, n in WHEEL_SEGMENTS), 3))
    # (channel held at 255, channel that ramps, whether it ramps down) per segment
    plan = ((0, 1, False), (1, 0, True), (1, 2, False), (2, 1, True), (2, 0, False), (0, 2, True))
    at = 0
    for (_, n), (full, ramp, down) in zip(WHEEL_SEGMENTS, plan):
        steps = np.floor(255 * np.arange(n) / n)
        wheel[at:at + n, full] = 255
        wheel[at:at + n, ramp] = 255 - steps if down else steps
        at += n
    return wheel


def _on_device(field, fn):
    """fn(device tensor [.., H, W, 2] f32) for a NumPy array (NumPy out) or a tensor (tensor out, on the device)."""
    import torch
    if torch.is_tensor(field):
        if not field.is_cuda:
            raise ValueError("flow_viz: a tensor must be on the device (a NumPy array is copied there)")
        return fn(field.to(torch.float32).contiguous())
    arr = np.ascontiguousarray(np.asarray(field), dtype=np.float32)
    return fn(torch.from_numpy(arr).cuda()).cpu().numpy()


def flow_uv_to_colors(u, v, convert_to_bgr=False):
    """Normalised components u, v [H, W] -> [H, W, 3] uint8: radius 1 is the fully saturated colour, beyond it the colour is
    dimmed.  The device kernel divides by the rad_max of norm 'diag', which the size fixes: the components are multiplied by it
    first, so the radius comes back to within an ulp."""
    import torch
    from dvd_amd import ops
    is_tensor = torch.is_tensor(u)
    uv = torch.stack([u, v], dim=-1) if is_tensor else np.stack([np.asarray(u), np.asarray(v)], axis=-1)
    if uv.ndim != 3:
        raise ValueError(f"flow_uv_to_colors: u and v must be [H, W], got {tuple(uv.shape[:-1])}")

    def run(field):
        # rad_max of norm 'diag' is fixed by the size; scale the field so that the division by it gives back u, v
        h, w = field.shape[:2]
        rad_max = float(np.float32(np.sqrt(np.float32((w // 2) ** 2 + (h // 2) ** 2))) + np.float32(1e-5))
        return ops.flow_to_image(field * rad_max, None, convert_to_bgr, "diag")
    return _on_device(uv, run)


def flow_to_image(flow_uv, clip_flow=None, convert_to_bgr=False, norm="diag"):
    """A displacement field [H, W, 2] in pixels -> [H, W, 3] uint8 (the reference's asserts, as ValueErrors)."""
    if getattr(flow_uv, "ndim", None) != 3:
        raise ValueError("input flow must have three dimensions")
    if flow_uv.shape[2] != 2:
        raise ValueError("input flow must have shape [H,W,2]")
    from dvd_amd import ops
    return _on_device(flow_uv, lambda field: ops.flow_to_image(field, clip_flow, convert_to_bgr, norm))
