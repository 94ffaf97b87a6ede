"""Unwarp any image with a saved coarse map (pred_flow/flow_<stem>.npy of a run with settings.flow_outputs = 'npy'):

    python -m dvd_amd.apply_map MAP.npy IMAGE OUT.png [--mode bicubic]

The image is decoded by PIL, unwarped on the device by ops.unwarp_u8 - the kernel that made the run's page - and written as
a PNG by PIL."""
import argparse

import numpy as np

from .run_options import WARP_MODES


def load_map(path):
    """The coarse map [2,G,G] of a .npy file as float32 [1,2,G,G]; anything else is a ValueError naming the file."""
    flow = np.load(path)
    if flow.ndim == 4 and flow.shape[0] == 1:
        flow = flow[0]
    if flow.ndim != 3 or flow.shape[0] != 2 or flow.shape[1] != flow.shape[2] or flow.shape[1] < 2 or flow.dtype.kind != "f":
        raise ValueError(f"{path}: expected a float map [2,G,G], got {flow.shape} {flow.dtype}")
    return np.ascontiguousarray(flow[None], dtype=np.float32)


def apply_map(map_path, image_path, out_path, mode="bilinear"):
    if mode not in WARP_MODES:
        raise ValueError(f"--mode must be one of {WARP_MODES}, got {mode!r}")
    flow = load_map(map_path)
    import torch
    from PIL import Image
    from . import ops
    src = torch.from_numpy(np.array(Image.open(image_path).convert("RGB"))).cuda()
    page = ops.unwarp_u8(torch.from_numpy(flow).cuda(), src, mode=mode)
    Image.fromarray(page.cpu().numpy()).save(out_path)
    return page


def main(argv=None):
    p = argparse.ArgumentParser(prog="python -m dvd_amd.apply_map", description="Unwarp an image with a saved coarse map.")
    p.add_argument("map", help="flow_<stem>.npy: the coarse map [2,G,G]")
    p.add_argument("image", help="the image to unwarp (any format PIL reads)")
    p.add_argument("out", help="the PNG to write")
    p.add_argument("--mode", default="bilinear", choices=WARP_MODES)
    a = p.parse_args(argv)
    apply_map(a.map, a.image, a.out, a.mode)


if __name__ == "__main__":
    main()
