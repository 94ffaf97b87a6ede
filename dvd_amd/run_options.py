"""The engine-side switches of a sampling run (`settings.env.*` beyond the reference's attribute surface): ONE table of name,
default, accepted values and description, and `RunOptions.from_env(env)`, which reads and checks them once.  admin/local.py
takes its engine-side defaults from the table; ops.py, the loader and the page writer take the accepted-value tuples from
here.  The module imports nothing of the package, so every one of them can import it."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Any

import numpy as np

WARP_MODES = ("bilinear", "bicubic")
CODEC_ROUTES = ("pil", "hip")           # who encodes / decodes a file: PIL on the host, or the HIP codec on the device
PNG_HUFFMAN = ("fixed", "dynamic")
PAGE_FORMATS = ("png", "jpeg")
JPEG_SUBSAMPLINGS = ("420", "444")
METRIC_PRESETS = ("docunet", "wang")
GT_METRICS = ("ms_ssim", "ld")          # what env.gt_metrics may name; env.gt_ad adds 'ad'


def is_jpeg_quality(quality):
    return not isinstance(quality, bool) and isinstance(quality, (int, np.integer)) and 1 <= quality <= 100


def _jpeg_quality(quality):
    if not is_jpeg_quality(quality):
        raise ValueError(f"env.jpeg_quality must be an integer 1..100, got {quality!r}")
    return int(quality)


def either(values):
    """'a' or 'b': how a message names the accepted values."""
    return " or ".join(map(repr, values))


def _metric_preset(preset):
    if preset not in METRIC_PRESETS:
        raise ValueError(f"env.metric_preset: preset must be {either(METRIC_PRESETS)}, got {preset!r}")
    return preset


def parse_gt_metrics(value):
    """env.gt_metrics, a comma-separated list of GT_METRICS names ('ms_ssim' | 'ms_ssim,ld' | 'ld') -> the names, in the order
    of GT_METRICS.  Anything else is a ValueError."""
    names = [n.strip() for n in value.split(",")] if isinstance(value, str) else None
    if not names or any(n not in GT_METRICS for n in names) or len(set(names)) != len(names):
        raise ValueError(f"env.gt_metrics must be a comma-separated list of {GT_METRICS} without repeats, got {value!r}")
    return tuple(m for m in GT_METRICS if m in names)


def _gt_ad(value):
    if not isinstance(value, bool):
        raise ValueError(f"env.gt_ad must be True or False, got {value!r}")
    return value


@dataclass(frozen=True)
class Switch:
    name: str
    default: Any
    accepts: Any        # None: taken as it is | a tuple of the accepted strings | a checker: value -> parsed value, or ValueError
    doc: str


# In the order `RunOptions.from_env` checks them: of several bad values the first one here is reported.
TABLE = (
    Switch("grid_size", 64, None, "coordinate grid G (the reference: fixed 64)"),
    Switch("batch_docs", 1, None, "documents sampled together per GPU (the reference: 1)"),
    Switch("sampler", "ddim", None, "'ddim' | 'ddpm'"),
    Switch("unwarp_mode", "bilinear", WARP_MODES,
           "interpolation of the full-resolution unwarp tail: 'bilinear' (the reference) | 'bicubic'"),
    Switch("png_encoder", "pil", CODEC_ROUTES,
           "who writes dewarped_pred/warped_<stem>.png: 'pil' (the reference: copy the page to the host, Image.save) | 'hip' "
           "(ops.png_encode on the device, only the compressed file crosses to the host; the same pixels, other bytes - "
           "DESIGN.md 4.4)"),
    Switch("png_huffman", "fixed", PNG_HUFFMAN,
           "the deflate blocks of the 'hip' PNG encoder: 'fixed' (one fixed-Huffman block per segment) | 'dynamic' (per segment "
           "the smaller of a dynamic-Huffman and the fixed block: the same pixels in a file about a third smaller - DESIGN.md 4.4)"),
    Switch("page_format", "png", PAGE_FORMATS,
           "the container of dewarped_pred/warped_<stem>: 'png' (the reference; png_encoder chooses who writes it) | 'jpeg' "
           "(warped_<stem>.jpg: baseline JFIF encoded on the device by ops.jpeg_encode, only the file crosses to the host; "
           "png_encoder is not consulted - DESIGN.md 4.5)"),
    Switch("jpeg_quality", 90, _jpeg_quality, "1..100, PIL's `quality` scale (the Annex K tables scaled by the usual rule)"),
    Switch("jpeg_subsampling", "420", JPEG_SUBSAMPLINGS, "'420' | '444'"),
    Switch("image_decoder", "pil", CODEC_ROUTES,
           "who decodes the input photograph of the image-directory path: 'pil' (the loader decodes on the CPU, the pixels cross "
           "to the device) | 'hip' (a .jpg/.jpeg FILE crosses and ops.jpeg_decode makes the same bytes there; a file the device "
           "decoder does not cover, and every other format, is decoded by PIL with one log line naming the reason - DESIGN.md 4.6)"),
    Switch("png_decoder", "pil", CODEC_ROUTES,
           "who decodes PNG files - the .png photographs of the image-directory path and the ground-truth scans of gt_dir: 'pil' "
           "(on the CPU, the pixels cross to the device) | 'hip' (the FILE crosses and ops.png_decode inflates and unfilters it "
           "there: the same bytes; a file the device decoder hands back is decoded by PIL with one log line naming the reason - "
           "DESIGN.md 4.9)"),
    Switch("gt_metrics", "ms_ssim", parse_gt_metrics,
           "which metrics gt_dir scores: 'ms_ssim' | 'ms_ssim,ld' | 'ld'.  'ld' adds the local distortion, the mean length of a "
           "dense SIFT-flow field from the scan to the page (ops.ld_u8, DESIGN.md 4.7): logged, written to ld.txt, left in "
           "settings.ld"),
    Switch("gt_ad", False, _gt_ad,
           "True: gt_dir also scores every page with the aligned distortion (ops.ad_u8, DESIGN.md 4.8): the SIFT-flow left after "
           "a fitted translation and scale are taken out, weighted by the scan's gradient magnitude; logged, written to ad.txt, "
           "left in settings.ad.  With 'ld' in gt_metrics both come from one run of the chain."),
    Switch("gt_dir", "", None,
           "directory of ground-truth scans `<stem>.png` (matched by `evaluation.gt_candidates`): when set, every dewarped page "
           "is scored against its scan with MS-SSIM (ops.ms_ssim_u8) - logged per document and as a mean, written to ms_ssim.txt "
           "beside the pictures, left in settings.ms_ssim as [(path, value)]; \"\" = no scoring, nothing else changes"),
    Switch("metric_preset", "docunet", _metric_preset, "'docunet' | 'wang' (DESIGN.md 4.3); checked only when gt_dir is set"),
    Switch("num_synthetic_docs", 4, None, "documents of the 'synthetic' dataset"),
    Switch("full_res", (1024, 768), None, "synthetic full-resolution source size (H, W)"),
    Switch("conditioning_dir", "", None, "directory of per-document conditioning .npz files (skips ingest + pre-stage nets)"),
    Switch("num_workers", 0, None, "DataLoader workers of the image-directory path (they only decode; the reference: 8)"),
    Switch("use_prestage_nets", True, None,
           "run the pre-stage conditioning nets (GeoTr_Seg_Inf.msk, Seg, line UNet; reference evaluation.py:162-216) on the "
           "document images, as the reference does; False = synthetic documents carry random conditioning tensors"),
    Switch("synthetic_weights_if_missing", None, None,
           "None = only when eval_dataset_name == 'synthetic' (a missing checkpoint on a real dataset raises)"),
    Switch("dewarping_model_path", "", None,
           "GeoTr checkpoint (DocTr's geometry transformer, keys 'module.<...>') read when use_init_flow is True: the reference's "
           "reload_model(pretrained_dewarp_model.GeoTr, settings.env.dewarping_model_path) (train_TDiff.py:89)"),
)
SWITCHES = {s.name: s for s in TABLE}
DEFAULTS = {s.name: s.default for s in TABLE}


def read(env, name):
    """env.<name>, or the table's default when `env` lacks the attribute; unchecked."""
    return getattr(env, name, DEFAULTS[name])


def check(env, name):
    """env.<name> (or its default), checked against the table and parsed: ValueError names the setting."""
    value, accepts = read(env, name), SWITCHES[name].accepts
    if callable(accepts):
        return accepts(value)
    if accepts is not None and not (isinstance(value, str) and value in accepts):
        raise ValueError(f"env.{name} must be {either(accepts)}, got {value!r}")
    return value


@dataclass(frozen=True)
class PageOptions:
    """The switches of the page writer (`visualize_dewarping`), checked."""
    png_encoder: str
    png_huffman: str
    page_format: str
    jpeg_quality: int
    jpeg_subsampling: str

    @classmethod
    def from_env(cls, env):
        """Reads each switch of the class once and checks it, in the table's order."""
        return cls(**{s.name: check(env, s.name) for s in TABLE if s.name in cls.__dataclass_fields__})

    @property
    def page_writer(self):
        """Who writes a dewarped page: 'pil' | 'hip' (PNG, by png_encoder) | 'jpeg' (page_format 'jpeg': png_encoder is not
        consulted)."""
        return "jpeg" if self.page_format == "jpeg" else self.png_encoder


@dataclass(frozen=True)
class RunOptions(PageOptions):
    """Every switch of TABLE as one run sees it, checked.  gt_metrics is the tuple of metric names that gt_dir scores, in
    order, with 'ad' appended under gt_ad."""
    grid_size: int
    batch_docs: int
    sampler: str
    unwarp_mode: str
    image_decoder: str
    png_decoder: str
    gt_metrics: tuple
    gt_ad: bool
    gt_dir: str
    metric_preset: str
    num_synthetic_docs: int
    full_res: tuple
    conditioning_dir: str
    num_workers: int
    use_prestage_nets: bool
    synthetic_weights_if_missing: Any
    dewarping_model_path: str

    @classmethod
    def from_env(cls, env):
        """As PageOptions.from_env, but metric_preset is checked only when gt_dir is set."""
        values = {s.name: check(env, s.name) for s in TABLE if s.name != "metric_preset"}
        values["metric_preset"] = check(env, "metric_preset") if values["gt_dir"] else read(env, "metric_preset")
        if values["gt_ad"]:
            values["gt_metrics"] += ("ad",)
        return cls(**values)
