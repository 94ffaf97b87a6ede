"""Scan-like pages from dewarped ones:

    python -m dvd_amd.clean_pages PAGES_DIR OUT [--no-flatten] [--binarize] [--cell S] [--close K] [--smooth B] [--keep-cast]
                                  [--white V] [--radius R] [--k K] [--format png|jpeg]

Every image file of PAGES_DIR is decoded on the device (ops.decode_image), flattened - its illumination divided out by a paper
estimate: ops.page_flatten - and, with --binarize, turned into Sauvola's black-and-white plane (ops.page_binarize), all in one
workspace (ops.page_clean).  --no-flatten binarises the page as it is; --keep-cast flattens with one gray estimate, so the
paper keeps its colour.  The result is written by the device encoders - a binarised page with its plane repeated into RGB - so
only compressed bytes come back to the host.  OUT/manifest.json records the parameters and, per page, its size and the three
counts: channel samples that saturated, samples whose paper estimate was raised to one level, and ink pixels."""
import argparse
import json
import os

from . import ops

IMAGE_SUFFIXES = (".png", ".jpg", ".jpeg")
FORMATS = {"png": ".png", "jpeg": ".jpg"}
MANIFEST_KEYS = ("stem", "image", "page", "size", "bytes", "saturated", "floored", "ink")


def find_pages(pages_dir):
    """[(stem, path)] of the image files of pages_dir, sorted by stem."""
    names = [f for f in os.listdir(pages_dir) if f.lower().endswith(IMAGE_SUFFIXES)]
    return sorted((os.path.splitext(f)[0], os.path.join(pages_dir, f)) for f in names)


def clean_pages(pages_dir, out_dir, flatten=True, binarize=False, cell=16, close=2, smooth=2, neutral=True, white=255, radius=15, k=0.2,
                fmt="png", log=print):
    """Clean every page of pages_dir; returns the manifest (also written to out_dir/manifest.json).  A bad request is a
    ValueError before anything is read or created."""
    if fmt not in FORMATS:
        raise ValueError(f"--format must be one of {tuple(FORMATS)}, got {fmt!r}")
    if not flatten and not binarize:
        raise ValueError("--no-flatten without --binarize: nothing to do")
    if cell not in ops.CLEAN_CELLS:
        raise ValueError(f"--cell must be one of {ops.CLEAN_CELLS}, got {cell!r}")
    for flag, v, lo, hi in (("--close", close, 0, 8), ("--smooth", smooth, 0, 8), ("--white", white, 1, 255), ("--radius", radius, 1, 63)):
        if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
            raise ValueError(f"{flag} must be an integer {lo}..{hi}, got {v!r}")
    kq = ops.clean_kq(k, "--k")
    if not os.path.isdir(pages_dir):
        raise ValueError(f"PAGES_DIR must be a directory, got {pages_dir!r}")
    todo = find_pages(pages_dir)
    if not todo:
        raise ValueError(f"{pages_dir}: holds no {' / '.join(IMAGE_SUFFIXES)} file")
    if len({stem for stem, _ in todo}) != len(todo):
        raise ValueError(f"{pages_dir}: two image files share a stem")
    os.makedirs(out_dir, exist_ok=True)
    pages = []
    for stem, path in todo:
        img = ops.decode_image(path, png=True, log=lambda line: None)[0]
        h, w = int(img.shape[0]), int(img.shape[1])
        out, cnt = ops.page_clean(img, flatten=flatten, binarize=binarize, cell=cell, close=close, smooth=smooth, neutral=neutral, white=white,
                                  radius=radius, k=k, return_stats=True)
        if binarize:
            out = out[:, :, None].expand(h, w, 3).contiguous()    # the encoders take RGB: no 1-bit encoder here
        name = stem + FORMATS[fmt]
        write = ops.jpeg_encode_to_file if fmt == "jpeg" else ops.png_encode_to_file
        nbytes = write(out, os.path.join(out_dir, name))
        pages.append(dict(zip(MANIFEST_KEYS, (stem, os.path.basename(path), name, [h, w], int(nbytes), *(cnt[s] for s in ops.CLEAN_STATS)))))
        log(f"{name}: {h} x {w}; " + ", ".join(f"{s} {cnt[s]}" for s in ops.CLEAN_STATS))
    manifest = {"parameters": dict(flatten=flatten, binarize=binarize, cell=cell, close=close, smooth=smooth, neutral=neutral, white=white,
                                   radius=radius, k=k, kq=kq, format=fmt),
                "pages": pages}
    with open(os.path.join(out_dir, "manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1)
    return manifest


def main(argv=None):
    p = argparse.ArgumentParser(prog="python -m dvd_amd.clean_pages", description="Scan-like pages: shading removal and Sauvola binarisation.")
    p.add_argument("pages_dir", help="the dewarped pages: .png / .jpg files")
    p.add_argument("out", help="the directory to write the cleaned pages and manifest.json to")
    p.add_argument("--no-flatten", action="store_true", help="leave the illumination as it is")
    p.add_argument("--binarize", action="store_true", help="write Sauvola's black-and-white plane")
    p.add_argument("--cell", type=int, default=16, help="pixels per cell of the paper estimate: 4, 8, 16, 32 or 64")
    p.add_argument("--close", type=int, default=2, help="half-width of the closing in cells, 0..8: ink narrower than 2 K + 1 cells is bridged")
    p.add_argument("--smooth", type=int, default=2, help="half-width of the tent in cells, 0..8")
    p.add_argument("--keep-cast", action="store_true", help="one gray paper estimate for all channels: the paper keeps its colour")
    p.add_argument("--white", type=int, default=255, help="the level the paper is taken to, 1..255")
    p.add_argument("--radius", type=int, default=15, help="half-width of Sauvola's window in pixels, 1..63")
    p.add_argument("--k", type=float, default=0.2, help="Sauvola's k, 0..1")
    p.add_argument("--format", default="png", choices=tuple(FORMATS))
    a = p.parse_args(argv)
    try:
        clean_pages(a.pages_dir, a.out, not a.no_flatten, a.binarize, a.cell, a.close, a.smooth, not a.keep_cast, a.white, a.radius, a.k,
                    a.format)
    except ValueError as e:
        p.error(str(e))


if __name__ == "__main__":
    main()
