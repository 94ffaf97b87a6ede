"""Unwarp any image with a saved coarse map (pred_flow/flow_<stem>.npy of a run with settings.flow_outputs = 'npy'):

    python -m dvd_amd.apply_map MAP.npy IMAGE OUT.png [--mode bicubic]

The image is decoded by PIL, unwarped on the device by ops.unwarp_u8 - the kernel that made the run's page - and written as
a PNG by PIL.

    python -m dvd_amd.apply_map MAP.npy IMAGE OUT.png --size SPEC [--max-radius R]

renders the page at a size of its own instead - SPEC is 'HxW', 'long:N' or 'xFACTOR' (ops.page_size) - through
ops.unwarp_u8_sized, which filters the photograph by the map's footprint (bilinear only, rounded not truncated),
and prints the three counts: pixels where the filter's radius was capped, whose centre is outside the photograph, and whose map
value is not finite.

    python -m dvd_amd.apply_map MAP.npy IMAGE OUT.txt --points PTS.txt --to page|photo [--step 8]

carries the N x 2 coordinates (x y per line, in pixels) of PTS.txt through the map instead: --to page takes positions on the
photograph IMAGE to the dewarped page (ops.map_invert, ops.transfer_points; "nan nan" where the page does not reach), --to photo
takes positions on the page to the photograph (ops.map_points).  IMAGE is opened for its size only.

    python -m dvd_amd.apply_map MAP.npy IMAGE OUT.png [--size SPEC] --clean flatten|binarize|flatten,binarize

cleans the page after the unwarp, at either size: `flatten` divides the illumination out by a paper estimate,
`binarize` writes Sauvola's black-and-white plane (of the flattened page where both are given), at ops.page_clean's defaults;
one more line prints the three counts: channel samples that saturated, samples whose paper estimate was raised, ink pixels."""
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


def clean_page(page, clean, out_path):
    """The page [H,W,3] uint8 after the stages of clean = (flatten, binarize), again [H,W,3] (a plane is repeated into RGB), and
    the counts, and the line that reports them."""
    from . import ops
    flatten, binarize = clean
    out, counts = ops.page_clean(page, flatten=flatten, binarize=binarize, return_stats=True)
    if binarize:
        out = out[:, :, None].expand(*out.shape, 3).contiguous()
    stages = ",".join(s for s, on in zip(ops.CLEAN_STAGES, clean) if on)
    return out, counts, f"{out_path}: {stages}; " + ", ".join(f"{s} {counts[s]}" for s in ops.CLEAN_STATS)


def apply_map(map_path, image_path, out_path, mode="bilinear", clean=None):
    if mode not in WARP_MODES:
        raise ValueError(f"--mode must be one of {WARP_MODES}, got {mode!r}")
    flow = load_map(map_path)
    import torch
    from PIL import Image
    from . import ops
    src = torch.from_numpy(np.array(Image.open(image_path).convert("RGB"))).cuda()
    page = ops.unwarp_u8(torch.from_numpy(flow).cuda(), src, mode=mode)
    if clean is not None:
        page, _, line = clean_page(page, clean, out_path)
    Image.fromarray(page.cpu().numpy()).save(out_path)
    if clean is not None:
        print(line)
    return page


class SizeRequestError(ValueError):
    """A --size or --max-radius the page cannot be rendered with: a usage error, unlike a broken map or image file."""


def apply_map_sized(map_path, image_path, out_path, size, max_radius=16, clean=None):
    """The page at the size `size` asks for (ops.page_size); returns (page, counts) and prints the counts in one line.  A bad
    request is refused before a file is opened."""
    from . import ops
    if isinstance(max_radius, bool) or not isinstance(max_radius, int) or not 1 <= max_radius <= ops.SIZED_MAX_RADIUS:
        raise SizeRequestError(f"--max-radius must be an integer 1..{ops.SIZED_MAX_RADIUS}, got {max_radius!r}")
    try:
        ops.parse_page_size(size)
    except ValueError as e:
        raise SizeRequestError(f"--size: {e}") from None
    flow = load_map(map_path)
    import torch
    from PIL import Image
    src = torch.from_numpy(np.array(Image.open(image_path).convert("RGB"))).cuda()
    try:
        hp, wp = ops.page_size(int(src.shape[0]), int(src.shape[1]), size)
    except ValueError as e:
        raise SizeRequestError(f"--size: {image_path} is {int(src.shape[0])} x {int(src.shape[1])}: {e}") from None
    page, counts = ops.unwarp_u8_sized(torch.from_numpy(flow[0]).cuda(), src, (hp, wp), max_radius=max_radius, return_stats=True)
    if clean is not None:
        page, cleaned, line = clean_page(page, clean, out_path)
    Image.fromarray(page.cpu().numpy()).save(out_path)
    print(f"{out_path}: {hp} x {wp} from {int(src.shape[0])} x {int(src.shape[1])}; capped {counts['capped']}, outside {counts['outside']}, "
          f"invalid {counts['invalid']}")
    if clean is not None:
        print(line)
        counts = {**counts, **cleaned}
    return page, counts


POINT_TARGETS = ("page", "photo")


def load_points(path):
    """The N x 2 coordinates of a text file (x y per line) as float32 [N,2]; anything else is a ValueError naming the file."""
    try:
        pts = np.loadtxt(path, dtype=np.float64, ndmin=2)
    except ValueError as e:
        raise ValueError(f"{path}: expected lines of two numbers: {e}") from None
    if pts.ndim != 2 or pts.shape[1] != 2:
        raise ValueError(f"{path}: expected N x 2 coordinates, got {pts.shape}")
    return np.ascontiguousarray(pts, dtype=np.float32)


def carry_points(flow, pts, h, w, to, step):
    """flow [1,2,G,G], pts [N,2] float32 on the host -> the carried points [N,2] float32 on the host, NaN where there is none."""
    import torch
    from . import ops
    dev_flow, dev_pts = torch.from_numpy(flow[0]).cuda(), torch.from_numpy(pts).cuda()
    if to == "page":
        fwd, _ = ops.map_invert(dev_flow, h, w, step=step)
        got = ops.transfer_points(fwd, dev_pts)
    else:
        got = ops.map_points(dev_flow, dev_pts, h, w)
    got = got.cpu().numpy()
    got[got.view(np.int32) == ops.MAP_INVALID] = np.nan
    return got


def apply_points(map_path, image_path, out_path, points_path, to="page", step=8):
    """Carry the points of `points_path` through the map at the size of `image_path`; writes and returns the N x 2 result
    (NaN where there is none)."""
    if to not in POINT_TARGETS:
        raise ValueError(f"--to must be one of {POINT_TARGETS}, got {to!r}")
    if isinstance(step, bool) or not isinstance(step, int) or step < 1:
        raise ValueError(f"--step must be a positive integer, got {step!r}")
    flow, pts = load_map(map_path), load_points(points_path)
    from PIL import Image
    with Image.open(image_path) as im:
        w, h = im.size
    got = carry_points(flow, pts, h, w, to, step)
    np.savetxt(out_path, got, fmt="%.4f")
    return got


def main(argv=None):
    p = argparse.ArgumentParser(prog="python -m dvd_amd.apply_map", description="Unwarp an image with a saved coarse map.")
    p.add_argument("map", help="flow_<stem>.npy: the coarse map [2,G,G]")
    p.add_argument("image", help="the image to unwarp (any format PIL reads)")
    p.add_argument("out", help="the PNG to write")
    p.add_argument("--mode", default="bilinear", choices=WARP_MODES)
    p.add_argument("--points", default=None, metavar="FILE", help="carry the N x 2 coordinates of FILE through the map; OUT is then "
                   "a text file and IMAGE gives the size only")
    p.add_argument("--to", default="page", choices=POINT_TARGETS, help="with --points: photograph -> page (default) or page -> photo")
    p.add_argument("--step", type=int, default=8, help="with --points --to page: the mesh step of the inverse")
    p.add_argument("--size", default=None, metavar="SPEC", help="render the page at this size: 'HxW', 'long:N' or 'xFACTOR' "
                   "(footprint-filtered, bilinear only)")
    p.add_argument("--max-radius", type=int, default=None, help="with --size: the filter's largest half-width in photograph pixels, "
                   "1..16 (default 16)")
    p.add_argument("--clean", default=None, metavar="STAGES", help="clean the page after the unwarp: 'flatten', 'binarize' or "
                   "'flatten,binarize'")
    a = p.parse_args(argv)
    clean = None
    if a.clean is not None:
        from . import ops
        if a.points is not None:
            p.error("--clean cleans a page: it cannot be combined with --points")
        try:
            clean = ops.parse_clean(a.clean)
        except ValueError as e:
            p.error(f"--clean: {e}")
    if a.size is not None:
        if a.points is not None:
            p.error("--size renders a page: it cannot be combined with --points")
        if a.mode != "bilinear":
            p.error(f"--size filters bilinearly: it cannot be combined with --mode {a.mode}")
        try:
            apply_map_sized(a.map, a.image, a.out, a.size, 16 if a.max_radius is None else a.max_radius, clean)
        except SizeRequestError as e:
            p.error(str(e))
        return
    if a.max_radius is not None:
        p.error("--max-radius needs --size")
    if a.points is not None:
        apply_points(a.map, a.image, a.out, a.points, a.to, a.step)
        return
    apply_map(a.map, a.image, a.out, a.mode, clean)


if __name__ == "__main__":
    main()
