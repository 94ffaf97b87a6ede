"""Synthetic documents with known ground truth: flat scans warped by maps drawn from a keyed family.

    python -m dvd_amd.synth_docs SCANS_DIR OUT_DIR --size HxW [--g 64] [--kinds tilt,curl,..] [--strength N] [--seed S]
           [--format jpeg|png] [--quality Q] [--step 8] [--shading L0,LGX,LGY,K] [--background FILE|R,G,B|noise] [--procedural N]

Per scan of SCANS_DIR (or per procedurally drawn page, --procedural N with SCANS_DIR given as -) it draws a backward map, turns
it round and renders the photograph on the device (ops.synth_document), and writes a dataset the document loop reads as it is:

    OUT/img/<stem>.jpg|png     the photograph (the directory Doc_benchmark lists)
    OUT/scan/<stem>.png        the flat scan                          -> env.gt_dir
    OUT/map/<stem>.npy, .flo   the map [2,g,g] and its h x w field    -> --gt_map_dir
    OUT/manifest.json          per document: key, kind, strength, attempts, the inverse's counts, the share at the filter's cap

A map is accepted only when its inverse reports no fold, no flipped, degenerate or skipped triangle; else it is redrawn with the
next attempt number, and after MAX_ATTEMPTS redraws at half the strength.  The maps and the pages are drawn on the host in
float64 from NumPy's Philox generator, keyed by ops.corruption_key(seed, path): the same seed and name, the same document."""
import argparse
import json
import os

import numpy as np

KINDS = ("tilt", "curl", "wave", "crease", "mixed")
FORMATS = ("jpeg", "png")
MAX_ATTEMPTS = 8
SCALE = 0.987
ACCEPT_ZERO = ("fold_px", "flipped_tris", "degenerate_tris", "skipped_tris")
MANIFEST_KEYS = ("stem", "key", "kind", "strength", "strength_asked", "attempts", "halvings", "stats", "cap_share", "size", "scan_size",
                 "g", "step", "image", "scan", "map", "flo")
_IMAGE_EXTS = (".jpg", ".jpeg", ".png", ".bmp", ".tif", ".tiff", ".webp")


def document_key(seed, name):
    """ops.corruption_key(seed, name) = (seed & 0xffffffff, crc32(name)): the key names the document, not its place in a run."""
    from . import ops
    return ops.corruption_key(seed, name)


def generator(key, attempt=0, stream=0):
    """NumPy's Philox generator of one document: its 128-bit key is (key[0], key[1], attempt, stream)."""
    k0, k1 = (int(v) & 0xffffffff for v in key)
    return np.random.Generator(np.random.Philox(key=np.array([k0 | k1 << 32, (int(attempt) & 0xffffffff) | (int(stream) & 0xffffffff) << 32],
                                                             dtype=np.uint64)))


def _check_map_args(g, kind, strength, margin):
    if isinstance(g, bool) or not isinstance(g, (int, np.integer)) or not 2 <= g <= 8192:
        raise ValueError(f"make_map: g must be an integer 2..8192, got {g!r}")
    if kind not in KINDS:
        raise ValueError(f"make_map: kind must be one of {', '.join(KINDS)}, got {kind!r}")
    if isinstance(strength, bool) or not isinstance(strength, (int, float, np.integer, np.floating)) or not 0 < strength <= 5:
        raise ValueError(f"make_map: strength must be a number in (0, 5], got {strength!r}")
    if isinstance(margin, bool) or not isinstance(margin, (int, float)) or not 0 <= margin < 0.5:
        raise ValueError(f"make_map: margin must be in [0, 0.5), got {margin!r}")


def _unit(rng):
    t = rng.uniform(0, 2 * np.pi)
    return np.array([np.cos(t), np.sin(t)])


def _tilt(rng, x, y, a):
    c = rng.uniform(-2 * a, 2 * a, (2, 2, 2))                       # [axis, row, column]: the four corners' displacements
    return np.stack([(c[k, 0, 0] * (1 - x) + c[k, 0, 1] * x) * (1 - y) + (c[k, 1, 0] * (1 - x) + c[k, 1, 1] * x) * y for k in (0, 1)])


def _curl(rng, x, y, s):
    """A page bent round a cylinder, seen from above: along the unit normal n of the cylinder's axis a page coordinate r lands
    at R sin(r / R).  |r| / R stays below pi / 2, so the profile is monotone."""
    n = _unit(rng)
    curv = 0.28 * s * rng.uniform(0.75, 1.25)
    r = (x - 0.5) * n[0] + (y - 0.5) * n[1] - rng.uniform(-0.1, 0.1)
    d = np.sin(r * curv) / curv - r
    return np.stack([d * n[0], d * n[1]])


def _wave(rng, x, y, a):
    count = int(rng.integers(2, 4))
    d = np.zeros((2,) + x.shape)
    for _ in range(count):
        k, m = _unit(rng), _unit(rng)
        f, phase, amp = rng.uniform(0.5, 1.5), rng.uniform(0, 2 * np.pi), a * rng.uniform(0.5, 1.0) / count * 2
        wave = amp * np.sin(2 * np.pi * f * (x * k[0] + y * k[1]) + phase)
        d += np.stack([wave * m[0], wave * m[1]])
    return d


def _crease(rng, x, y, a):
    n, m = _unit(rng), _unit(rng)
    c, width = rng.uniform(0.3, 0.7, 2), rng.uniform(0.08, 0.2)
    step = a * np.tanh(((x - c[0]) * n[0] + (y - c[1]) * n[1]) / width)
    return np.stack([step * m[0], step * m[1]])


def make_map(key, g=64, kind="mixed", strength=3, margin=0.04, attempt=0):
    """float32 [2,g,g]: a backward map of the family `kind` in the run's own convention - what flow_grid_at adds to the base
    grid k / (g - 1), so that page position t samples the photograph at ((t + flow) 2 - 1) 0.987 in [-1, 1].  strength 1..5
    scales the displacements (about 1.2 % of the side per unit).  The sampled positions are contracted about the centre until
    every one lies at least `margin` of the side inside the frame.  Drawn in float64, rounded to f32 once."""
    _check_map_args(g, kind, strength, margin)
    rng = generator(key, attempt)
    t = np.linspace(0.0, 1.0, g)
    y, x = np.meshgrid(t, t, indexing="ij")
    s = float(strength)
    a = 0.012 * s
    if kind == "tilt":
        d = _tilt(rng, x, y, a)
    elif kind == "curl":
        d = _curl(rng, x, y, s)
    elif kind == "wave":
        d = _wave(rng, x, y, a)
    elif kind == "crease":
        d = _crease(rng, x, y, a)
    else:
        d = 0.6 * _tilt(rng, x, y, a) + 0.6 * _curl(rng, x, y, s * 0.6) + 0.5 * _wave(rng, x, y, a) + 0.5 * _crease(rng, x, y, a)
    q = np.stack([x, y]) + d - 0.5                                   # the sampled position about the centre, before the scale
    reach = SCALE * np.abs(q).max()
    c = min(1.0, (0.5 - margin) * (1 - 1e-5) / reach)                # the slack covers the rounding to f32
    return (c * q + 0.5 - np.stack([x, y])).astype(np.float32)


def draw_accepted(key, accept, g=64, kind="mixed", strength=3, margin=0.04):
    """Draw maps until `accept(flow)` - a callable that returns the inverse's stats, or (stats, anything) - reports no fold and
    no flipped, degenerate or skipped triangle: at most MAX_ATTEMPTS per strength, then at half the strength.  Returns
    (flow, what accept returned, record) with record = {attempts, halvings, strength}."""
    attempt, halvings, s = 0, 0, float(strength)
    while True:
        for _ in range(MAX_ATTEMPTS):
            flow = make_map(key, g, kind, s, margin, attempt)
            got = accept(flow)
            attempt += 1
            stats = got[0] if isinstance(got, tuple) else got
            if all(stats[k] == 0 for k in ACCEPT_ZERO):
                return flow, got, {"attempts": attempt, "halvings": halvings, "strength": s}
        s, halvings = s / 2, halvings + 1
        if halvings > 16:
            raise RuntimeError(f"draw_accepted: no fold-free map of kind {kind!r} for key {key} down to strength {s}")


def procedural_page(key, h, w):
    """uint8 [h,w,3]: a text-like page - margins, lines of word boxes of keyed random width, one rule, one gray block."""
    if min(h, w) < 8:
        raise ValueError(f"procedural_page: sides of at least 8, got {h} x {w}")
    rng = generator(key, 0, stream=1)
    page = np.full((h, w, 3), 250, np.uint8)
    page[...] = (int(rng.integers(238, 256)), int(rng.integers(238, 256)), int(rng.integers(228, 256)))
    top, left = max(2, h // 12), max(2, w // 10)
    line = max(2, h // 48)                                           # the height of a line of text; as much again between lines
    block = (int(rng.integers(top, max(top + 1, h // 2))), max(line * 4, h // 6))
    rule_at = int(rng.integers(top, h - top))
    yy = top
    while yy + line <= h - top:
        if block[0] <= yy < block[0] + block[1]:
            x0, x1 = left, left + (w - 2 * left) // 2
            y1 = min(block[0] + block[1], h - top)
            page[yy:y1, x0:x1] = int(rng.integers(120, 200))
            xx = x1 + line
        else:
            xx = left + (int(rng.integers(0, 4)) == 0) * 2 * line
        end = w - left - int(rng.integers(0, max(1, (w - 2 * left) // 3)))
        ink = int(rng.integers(20, 90))
        while xx < end:
            word = int(rng.integers(1, 8)) * line
            page[yy:yy + line, xx:min(xx + word, end)] = ink
            xx += word + line
        yy += 2 * line
    page[rule_at:rule_at + max(1, line // 2), left:w - left] = 60
    return page


def noise_background(key, h, w):
    """uint8 [h,w,3]: a keyed desk texture, 4 x 4 blocks of a brownish gray."""
    rng = generator(key, 0, stream=2)
    base = rng.integers(70, 150, ((h + 3) // 4, (w + 3) // 4, 1))
    tint = np.array([12, 0, -14])
    img = np.clip(base + tint + rng.integers(-6, 7, base.shape[:2] + (3,)), 0, 255).astype(np.uint8)
    return np.ascontiguousarray(np.repeat(np.repeat(img, 4, axis=0), 4, axis=1)[:h, :w])


# ---- the command line ------------------------------------------------------------------------------------------------------------
def parse_size(text):
    try:
        h, w = (int(v) for v in str(text).lower().split("x"))
    except ValueError:
        raise ValueError(f"--size must be HxW, two integers, got {text!r}") from None
    if not 8 <= h <= 16384 or not 8 <= w <= 16384:
        raise ValueError(f"--size: sides 8..16384, got {text!r}")
    return h, w


def parse_kinds(text):
    kinds = tuple(k for k in str(text).split(",") if k)
    if not kinds or any(k not in KINDS for k in kinds):
        raise ValueError(f"--kinds must be a comma-separated list of {', '.join(KINDS)}, got {text!r}")
    return kinds


def parse_shading(text):
    """'' or None: no shading; else L0,LGX,LGY,K."""
    if text is None or text == "":
        return None
    try:
        v = [float(p) for p in str(text).split(",")]
    except ValueError:
        v = []
    if len(v) != 4 or not all(np.isfinite(v)):
        raise ValueError(f"--shading must be four finite numbers L0,LGX,LGY,K, got {text!r}")
    return dict(zip(("l0", "lgx", "lgy", "k"), v))


def parse_background(text):
    """('color', (r, g, b)) | ('noise', None) | ('file', path)."""
    text = str(text)
    if text == "noise":
        return "noise", None
    parts = text.split(",")
    if len(parts) == 3:
        try:
            rgb = tuple(int(p) for p in parts)
        except ValueError:
            rgb = (-1,)
        if all(0 <= c <= 255 for c in rgb):
            return "color", rgb
        raise ValueError(f"--background R,G,B: three integers 0..255, got {text!r}")
    if not os.path.isfile(text):
        raise ValueError(f"--background must be a file, R,G,B or noise, got {text!r}")
    return "file", text


def check_options(scans_dir, size, g=64, kinds=KINDS, strength=3, seed=0, fmt="jpeg", quality=90, step=8, procedural=0):
    """Every option that can be refused without a device or a file written; returns the list of (stem, scan path or None)."""
    h, w = size
    is_int = lambda v: isinstance(v, (int, np.integer)) and not isinstance(v, bool)           # noqa: E731
    if not is_int(g) or not 2 <= g <= 8192:
        raise ValueError(f"--g must be an integer 2..8192, got {g!r}")
    if not is_int(strength) or not 1 <= strength <= 5:
        raise ValueError(f"--strength must be an integer 1..5, got {strength!r}")
    if not is_int(seed):
        raise ValueError(f"--seed must be an integer, got {seed!r}")
    if fmt not in FORMATS:
        raise ValueError(f"--format must be one of {', '.join(FORMATS)}, got {fmt!r}")
    if not is_int(quality) or not 1 <= quality <= 100:
        raise ValueError(f"--quality must be an integer 1..100, got {quality!r}")
    if not is_int(step) or not 1 <= step <= 16384:
        raise ValueError(f"--step must be an integer 1..16384, got {step!r}")
    if not is_int(procedural) or procedural < 0:
        raise ValueError(f"--procedural must be a non-negative integer, got {procedural!r}")
    if any(k not in KINDS for k in kinds) or not kinds:
        raise ValueError(f"--kinds must name some of {', '.join(KINDS)}, got {kinds!r}")
    if procedural:
        if scans_dir not in (None, "", "-"):
            raise ValueError(f"--procedural draws its own pages: give - for SCANS_DIR, got {scans_dir!r}")
        return [(f"page_{i:05d}", None) for i in range(procedural)]
    if scans_dir in (None, "", "-") or not os.path.isdir(scans_dir):
        raise ValueError(f"SCANS_DIR must be an existing directory (or - with --procedural N), got {scans_dir!r}")
    files = sorted(f for f in os.listdir(scans_dir) if f.lower().endswith(_IMAGE_EXTS))
    stems = [os.path.splitext(f)[0] for f in files]
    if not files:
        raise ValueError(f"SCANS_DIR {scans_dir!r} holds no image file")
    if len(set(stems)) != len(stems):
        raise ValueError(f"SCANS_DIR {scans_dir!r}: two files share a stem")
    return [(s, os.path.join(scans_dir, f)) for s, f in zip(stems, files)]


class DeviceBackend:
    """What write_dataset asks of the device: ops.synth_document, the footprint's share at the cap and the device encoders."""

    def __init__(self):
        import torch
        from . import ops
        self.torch, self.ops = torch, ops

    def upload(self, array):
        return self.torch.from_numpy(np.ascontiguousarray(array)).cuda()

    def document(self, scan, flow, h, w, step, background, shading):
        """(photo, fwd, stats) of ops.synth_document; scan and a background plane come from upload()."""
        return self.ops.synth_document(scan, self.upload(flow), h, w, step=step, scale=SCALE, background=background, shading=shading)

    def at_cap(self, scan_hw, fwd):
        radii = self.ops.synth_footprint(tuple(scan_hw), fwd)
        return int((radii.max(dim=2).values == self.ops.SYNTH_MAX_RADIUS).sum())

    def write_image(self, img, path, fmt="png", quality=90):
        if fmt == "jpeg":
            return self.ops.jpeg_encode_to_file(img, path, quality=quality)
        return self.ops.png_encode_to_file(img, path)

    def write_flo(self, flow, h, w, path):
        return self.ops.flow_write_flo(self.upload(flow), h, w, path)


def write_dataset(scans_dir, out_dir, size, g=64, kinds=KINDS, strength=3, seed=0, fmt="jpeg", quality=90, step=8, shading=None,
                  background="255,255,255", procedural=0, margin=0.04, log=print, backend=None):
    """The command's work; returns the manifest (also written to OUT/manifest.json).  backend: None for the device."""
    h, w = size
    docs = check_options(scans_dir, size, g, kinds, strength, seed, fmt, quality, step, procedural)
    bg_kind, bg_value = parse_background(background)
    if isinstance(shading, str):
        shading = parse_shading(shading)
    from .ops import pil_decode_rgb8, synth_shading
    synth_shading(shading, "--shading")
    dev = DeviceBackend() if backend is None else backend
    for sub in ("img", "scan", "map"):
        os.makedirs(os.path.join(out_dir, sub), exist_ok=True)
    if bg_kind == "file":
        from PIL import Image
        bg_file = np.asarray(Image.open(bg_value).convert("RGB").resize((w, h)), dtype=np.uint8)
    ext = "jpg" if fmt == "jpeg" else "png"
    entries = []
    for i, (stem, path) in enumerate(docs):
        key = document_key(seed, stem)
        scan = procedural_page(key, h, w) if path is None else pil_decode_rgb8(path)
        dscan = dev.upload(scan)
        bg = bg_value if bg_kind == "color" else dev.upload(noise_background(key, h, w) if bg_kind == "noise" else bg_file)
        kind = kinds[i % len(kinds)]

        def accept(flow):
            photo, fwd, stats = dev.document(dscan, flow, h, w, step, bg, shading)
            return stats, (photo, fwd)
        flow, (stats, (photo, fwd)), record = draw_accepted(key, accept, g, kind, strength, margin)
        at_cap = dev.at_cap(scan.shape[:2], fwd)
        dev.write_image(photo, os.path.join(out_dir, "img", f"{stem}.{ext}"), fmt, quality)
        dev.write_image(dscan, os.path.join(out_dir, "scan", f"{stem}.png"))
        np.save(os.path.join(out_dir, "map", f"{stem}.npy"), flow)
        dev.write_flo(flow, h, w, os.path.join(out_dir, "map", f"{stem}.flo"))
        entry = {"stem": stem, "key": [int(k) for k in key], "kind": kind, "strength": record["strength"], "strength_asked": int(strength),
                 "attempts": record["attempts"], "halvings": record["halvings"], "stats": {k: int(v) for k, v in stats.items()},
                 "cap_share": at_cap / stats["covered"] if stats["covered"] else 0.0, "size": [h, w],
                 "scan_size": [int(scan.shape[0]), int(scan.shape[1])], "g": int(g), "step": int(step), "image": f"img/{stem}.{ext}",
                 "scan": f"scan/{stem}.png", "map": f"map/{stem}.npy", "flo": f"map/{stem}.flo"}
        entries.append(entry)
        log(f"{stem} {kind} strength {entry['strength']:g} attempts {entry['attempts']} covered {stats['covered']} "
            f"cap_share {entry['cap_share']:.4f}")
    manifest = {"seed": int(seed), "format": fmt, "quality": int(quality), "scale": SCALE, "margin": margin, "shading": shading,
                "background": str(background), "documents": entries}
    with open(os.path.join(out_dir, "manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1)
    return manifest


def main(argv=None):
    p = argparse.ArgumentParser(prog="python -m dvd_amd.synth_docs", description="Warp flat scans by known maps: photographs, scans and "
                                "ground-truth maps as a dataset the document loop reads.")
    p.add_argument("scans_dir", help="a directory of flat scans, or - with --procedural N")
    p.add_argument("out_dir")
    p.add_argument("--size", required=True, metavar="HxW", help="the photograph's size")
    p.add_argument("--g", type=int, default=64, help="the side of the coarse map")
    p.add_argument("--kinds", default=",".join(KINDS), help="map families, assigned to the documents in turn")
    p.add_argument("--strength", type=int, default=3, help="1..5")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--format", default="jpeg", choices=FORMATS, dest="fmt")
    p.add_argument("--quality", type=int, default=90)
    p.add_argument("--step", type=int, default=8, help="the mesh step of the inverse")
    p.add_argument("--shading", default="", metavar="L0,LGX,LGY,K")
    p.add_argument("--background", default="255,255,255", metavar="FILE|R,G,B|noise")
    p.add_argument("--procedural", type=int, default=0, metavar="N", help="draw N text-like pages instead of reading scans")
    a = p.parse_args(argv)
    try:
        size, kinds, shading = parse_size(a.size), parse_kinds(a.kinds), parse_shading(a.shading)
        parse_background(a.background)
        check_options(a.scans_dir, size, a.g, kinds, a.strength, a.seed, a.fmt, a.quality, a.step, a.procedural)
    except ValueError as e:
        p.error(str(e))
    return write_dataset(a.scans_dir, a.out_dir, size, a.g, kinds, a.strength, a.seed, a.fmt, a.quality, a.step, shading, a.background,
                         a.procedural)


if __name__ == "__main__":
    main()
