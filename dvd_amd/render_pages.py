"""Pages at a chosen size from the saved maps of a finished run (settings.flow_outputs = 'npy'):

    python -m dvd_amd.render_pages MAP_DIR IMAGE_DIR OUT --size SPEC [--format png|jpeg] [--quality Q] [--batch N] [--max-radius R]

Every MAP_DIR/flow_<stem>.npy is a coarse map [2,G,G]; its photograph is the image file of IMAGE_DIR whose stem is <stem>, or
the stem's leading integer (evaluation.gt_candidates' rule).  SPEC is what ops.page_size reads: 'HxW', 'long:N' or 'xFACTOR'.
Documents of different sizes go --batch at a time through ops.unwarp_u8_sized_ragged - one launch filters every photograph by
its own footprint - and the pages are written by the device encoders, so only compressed bytes come back to the
host.  OUT/manifest.json records, per document, the photograph's size, the page's size and the three counts.  A map without a
photograph is logged and skipped.

    ... --clean flatten|binarize|flatten,binarize

cleans every page after the unwarp (ops.page_clean at its defaults, DESIGN.md 4.17: the illumination divided out, Sauvola's
black-and-white plane, or both); the manifest then also names the stages and, per document, the counts saturated, floored and ink."""
import argparse
import json
import os

import numpy as np

from . import evaluation
from .apply_map import load_map

IMAGE_EXTS = (".png", ".jpg", ".jpeg", ".bmp", ".tif", ".tiff", ".webp")
FORMATS = {"png": ".png", "jpeg": ".jpg"}
MAP_PREFIX, MAP_SUFFIX = "flow_", ".npy"
MANIFEST_KEYS = ("stem", "map", "image", "page", "photo_size", "page_size", "capped", "outside", "invalid")


def find_maps(map_dir):
    """[(stem, path)] of every flow_<stem>.npy of map_dir, sorted by stem."""
    names = sorted(f for f in os.listdir(map_dir) if f.startswith(MAP_PREFIX) and f.endswith(MAP_SUFFIX) and len(f) > len(MAP_PREFIX + MAP_SUFFIX))
    return [(f[len(MAP_PREFIX):-len(MAP_SUFFIX)], os.path.join(map_dir, f)) for f in names]


def list_images(image_dir):
    """lower-case file name -> file name of image_dir: read once per run."""
    return {f.lower(): f for f in sorted(os.listdir(image_dir), reverse=True)}


def find_photograph(image_dir, stem, present=None):
    """The photograph of the map flow_<stem>.npy under image_dir, or None: the stem itself, then its leading integer, each with
    the image extensions in IMAGE_EXTS' order (either letter case).  present: list_images(image_dir), where the caller has it."""
    present = list_images(image_dir) if present is None else present
    for name in evaluation.gt_candidates(stem + ".png"):
        base = os.path.splitext(name)[0]
        for ext in IMAGE_EXTS:
            if (base + ext).lower() in present:
                return os.path.join(image_dir, present[(base + ext).lower()])
    return None


class DeviceBackend:
    """The device side of render_pages: decode, the ragged sized unwarp, the encoders.  The tests replace it with the model."""

    def __init__(self):
        import torch
        from . import ops
        self.torch, self.ops = torch, ops

    def size(self, path):
        """(H, W) of the photograph as load() will give it - the EXIF orientation applied - from the file's header alone."""
        from PIL import Image
        with Image.open(path) as im:
            w, h = im.size
            turned = im.getexif().get(0x0112, 1) in (5, 6, 7, 8)
        return (w, h) if turned else (h, w)

    def load(self, path):
        """The photograph [H,W,3] uint8 on the device."""
        return self.ops.decode_image(path, png=True, log=lambda line: None)[0]

    def render(self, flows, photos, sizes, max_radius):
        """flows: n [2,G,G] float32 arrays of one G -> (n pages on the device, n count dicts)."""
        flow = self.torch.from_numpy(np.stack(flows)).cuda()
        return self.ops.unwarp_u8_sized_ragged(flow, photos, sizes, max_radius=max_radius, return_stats=True)

    def write(self, page, path, fmt, quality):
        if fmt == "jpeg":
            return self.ops.jpeg_encode_to_file(page, path, quality=quality)
        return self.ops.png_encode_to_file(page, path)

    def shape(self, photo):
        return int(photo.shape[0]), int(photo.shape[1])

    def clean(self, page, flatten, binarize):
        """(the cleaned page, again [H,W,3] - a plane is repeated into RGB; its counts)"""
        out, counts = self.ops.page_clean(page, flatten=flatten, binarize=binarize, return_stats=True)
        if binarize:
            out = out[:, :, None].expand(*out.shape, 3).contiguous()
        return out, counts


def render_pages(map_dir, image_dir, out_dir, size, fmt="png", quality=90, batch=8, max_radius=16, log=print, backend=None, clean=None):
    """Render every map of map_dir; returns the manifest (also written to out_dir/manifest.json).  clean: None, or a --clean
    request (ops.parse_clean), applied to every page after the unwarp."""
    from . import ops
    stages = None if clean is None else ops.parse_clean(clean)
    if fmt not in FORMATS:
        raise ValueError(f"--format must be one of {tuple(FORMATS)}, got {fmt!r}")
    if isinstance(quality, bool) or not isinstance(quality, int) or not 1 <= quality <= 100:
        raise ValueError(f"--quality must be an integer 1..100, got {quality!r}")
    if isinstance(batch, bool) or not isinstance(batch, int) or batch < 1:
        raise ValueError(f"--batch must be a positive integer, got {batch!r}")
    if isinstance(max_radius, bool) or not isinstance(max_radius, int) or not 1 <= max_radius <= ops.SIZED_MAX_RADIUS:
        raise ValueError(f"--max-radius must be an integer 1..{ops.SIZED_MAX_RADIUS}, got {max_radius!r}")
    ops.parse_page_size(size)                                 # no request at all: before any work
    for what, d in (("MAP_DIR", map_dir), ("IMAGE_DIR", image_dir)):
        if not os.path.isdir(d):
            raise ValueError(f"{what} must be a directory, got {d!r}")
    maps = find_maps(map_dir)
    if not maps:
        raise ValueError(f"{map_dir}: holds no {MAP_PREFIX}<stem>{MAP_SUFFIX} file")
    backend = backend or DeviceBackend()
    # every document's photograph and page size before the first launch: what cannot be rendered is skipped with one line
    present, docs, todo = list_images(image_dir), [], []
    for stem, map_path in maps:
        image = find_photograph(image_dir, stem, present)
        if image is None:
            log(f"{map_path} skipped: no photograph {stem}.* in {image_dir}")
            continue
        photo_hw = backend.size(image)
        try:
            todo.append((stem, map_path, image, ops.page_size(*photo_hw, size)))
        except ValueError as e:
            log(f"{map_path} skipped: {image} is {photo_hw[0]} x {photo_hw[1]}: {e}")
    os.makedirs(out_dir, exist_ok=True)

    def flush(group):
        # one launch per coarse-grid size among the group's maps (a run has one)
        for g in sorted({e[4].shape[-1] for e in group}):
            part = [e for e in group if e[4].shape[-1] == g]
            photos = [e[5] for e in part]
            for e in part:
                if ops.page_size(*backend.shape(e[5]), size) != e[3]:
                    raise ValueError(f"{e[2]}: decoded as {backend.shape(e[5])}, its header said otherwise")
            pages, counts = backend.render([e[4][0] for e in part], photos, [e[3] for e in part], max_radius)
            for (stem, map_path, image, page_hw, _, photo), page, cnt in zip(part, pages, counts):
                name = stem + FORMATS[fmt]
                cleaned = None
                if stages is not None:
                    page, cleaned = backend.clean(page, *stages)
                backend.write(page, os.path.join(out_dir, name), fmt, quality)
                docs.append(dict(zip(MANIFEST_KEYS, (stem, os.path.basename(map_path), os.path.basename(image), name,
                                                     list(backend.shape(photo)), list(page_hw), cnt["capped"], cnt["outside"], cnt["invalid"]))))
                log(f"{name}: {page_hw[0]} x {page_hw[1]} from {backend.shape(photo)[0]} x {backend.shape(photo)[1]}; capped {cnt['capped']}, "
                    f"outside {cnt['outside']}, invalid {cnt['invalid']}")
                if cleaned is not None:
                    docs[-1].update((s, cleaned[s]) for s in ops.CLEAN_STATS)
                    log(f"{name}: {clean}; " + ", ".join(f"{s} {cleaned[s]}" for s in ops.CLEAN_STATS))
    for k in range(0, len(todo), batch):
        flush([(*e, load_map(e[1]), backend.load(e[2])) for e in todo[k:k + batch]])
    docs.sort(key=lambda d: d["stem"])
    manifest = {"size": list(size) if isinstance(size, (tuple, list)) else size, "format": fmt, "quality": quality if fmt == "jpeg" else None,
                "max_radius": max_radius, "documents": docs}
    if stages is not None:
        manifest["clean"] = ",".join(s for s, on in zip(ops.CLEAN_STAGES, stages) if on)
    with open(os.path.join(out_dir, "manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1)
    return manifest


def main(argv=None):
    p = argparse.ArgumentParser(prog="python -m dvd_amd.render_pages", description="Pages at a chosen size from a run's saved maps.")
    p.add_argument("map_dir", help="the run's pred_flow/: flow_<stem>.npy files")
    p.add_argument("image_dir", help="the photographs, found by stem")
    p.add_argument("out", help="the directory to write the pages and manifest.json to")
    p.add_argument("--size", required=True, metavar="SPEC", help="'HxW', 'long:N' or 'xFACTOR'")
    p.add_argument("--format", default="png", choices=tuple(FORMATS))
    p.add_argument("--quality", type=int, default=90, help="JPEG quality 1..100")
    p.add_argument("--batch", type=int, default=8, help="documents per launch")
    p.add_argument("--max-radius", type=int, default=16, help="the filter's largest half-width in photograph pixels, 1..16")
    p.add_argument("--clean", default=None, metavar="STAGES", help="clean every page after the unwarp: 'flatten', 'binarize' or "
                   "'flatten,binarize'")
    a = p.parse_args(argv)
    try:
        render_pages(a.map_dir, a.image_dir, a.out, a.size, a.format, a.quality, a.batch, a.max_radius, clean=a.clean)
    except ValueError as e:
        p.error(str(e))


if __name__ == "__main__":
    main()
