"""The engine-side switches of a sampling run (`settings.env.*` beyond the reference's attribute surface): ONE table of name,
default, accepted values and description, and `RunOptions.from_env(env)`, which reads and checks them once.  admin/local.py
takes its engine-side defaults from the table; ops.py, the loader and the page writer take the accepted-value tuples from
here.  ROUND_TABLE and `RoundOptions.from_settings(settings)` do the same for the attributes the launcher puts on `settings`
itself, and SCORES lists the per-document scores of a round: what enables each, its score sheet and its columns of the
corruption table.  A new switch or score is one row here.  The module imports nothing of the package, so every one of them can
import it."""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import Any, Optional

import numpy as np

WARP_MODES = ("bilinear", "bicubic")
CODEC_ROUTES = ("pil", "hip")           # who encodes / decodes a file: PIL on the host, or the HIP codec on the device
PNG_HUFFMAN = ("fixed", "dynamic")
PAGE_FORMATS = ("png", "jpeg")
JPEG_SUBSAMPLINGS = ("420", "444")
METRIC_PRESETS = ("docunet", "wang")
GT_METRICS = ("ms_ssim", "ld")          # what env.gt_metrics may name; env.gt_ad adds 'ad'
FLOW_OUTPUTS = ("png", "flo", "npy")    # what settings.flow_outputs may name
INVERSE_OUTPUTS = ("mesh", "flo", "mask")     # what settings.inverse_outputs may name


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


def name_list(label, accepted, empty_is_none=False):
    """The checker of `label`, a comma-separated list of `accepted` names without repeats: value -> the names, in the order of
    `accepted`.  empty_is_none: "" means none, (); otherwise "" is refused like anything else - a ValueError that names `label`."""
    def parse(value):
        if empty_is_none and isinstance(value, str) and value == "":
            return ()
        names = [n.strip() for n in value.split(",")] if isinstance(value, str) else None
        if not names or any(n not in accepted for n in names) or len(set(names)) != len(names):
            raise ValueError(f"{label} must be a comma-separated list of {accepted} without repeats, got {value!r}")
        return tuple(n for n in accepted if n in names)
    return parse


parse_gt_metrics = name_list("env.gt_metrics", GT_METRICS)     # 'ms_ssim' | 'ms_ssim,ld' | 'ld'


def _flag(label, types=(bool,)):
    def parse(value):
        if not isinstance(value, types):
            raise ValueError(f"{label} must be True or False, got {value!r}")
        return bool(value)
    return parse


def _gt_map_dir(value):
    if isinstance(value, str) and value == "":
        return None
    if not isinstance(value, str) or not os.path.isdir(value):
        raise ValueError(f"settings.gt_map_dir must be an existing directory (or \"\" for none), got {value!r}")
    return value


@dataclass(frozen=True)
class Switch:
    name: str
    default: Any
    accepts: Any        # None: taken as it is | a tuple of the accepted strings | a checker: value -> parsed value, or ValueError
    doc: str
    owner: str = "env"  # how a message names the object that carries the attribute: env.<name> | settings.<name>


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
    Switch("gt_ad", False, _flag("env.gt_ad"),
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
# What the launcher puts on `settings` itself (run_sampling.py: a flag that is not given leaves its attribute absent), in the order
# `RoundOptions.from_settings` checks them - after the env.* switches and after the corruption (evaluation.corruption_of).
ROUND_TABLE = (
    Switch("keyed_noise", False, _flag("settings.keyed_noise", (bool, np.bool_)),
           "True: the sampler's noise is keyed per document by (settings.seed, path); a clean round leaves its maps in "
           "settings.map_ref and a later round is scored against them with map_dev (DESIGN.md 4.11)", "settings"),
    Switch("flow_outputs", "", name_list("settings.flow_outputs", FLOW_OUTPUTS, empty_is_none=True),
           "what to write of every document's predicted map under pred_flow/: a comma-separated list of 'png', 'flo', 'npy' "
           "(DESIGN.md 4.12); \"\" = nothing", "settings"),
    Switch("gt_map_dir", "", _gt_map_dir,
           "directory of ground-truth maps: every document that has one there is scored with EPE, PCK, Fl and AUSE (DESIGN.md "
           "4.13); \"\" = nothing is scored (None once checked)", "settings"),
    Switch("inverse_outputs", "", name_list("settings.inverse_outputs", INVERSE_OUTPUTS, empty_is_none=True),
           "every document's predicted map is inverted on the device, and the files named are written under pred_flow/: a "
           "comma-separated list of 'mesh', 'flo', 'mask' (DESIGN.md 4.14); \"\" = nothing is inverted", "settings"),
)
SWITCHES = {s.name: s for s in TABLE + ROUND_TABLE}
DEFAULTS = {s.name: s.default for s in TABLE}           # of `env` alone: admin/local.py builds the environment from it


def read(owner, name):
    """<owner>.<name>, or the table's default when the object lacks the attribute; unchecked."""
    return getattr(owner, name, SWITCHES[name].default)


def check(owner, name):
    """<owner>.<name> (or its default), checked against the table and parsed: ValueError names the setting."""
    switch, value = SWITCHES[name], read(owner, name)
    if callable(switch.accepts):
        return switch.accepts(value)
    if switch.accepts is not None and not (isinstance(value, str) and value in switch.accepts):
        raise ValueError(f"{switch.owner}.{name} must be {either(switch.accepts)}, got {value!r}")
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


@dataclass(frozen=True)
class RoundOptions:
    """Every switch of ROUND_TABLE as one round sees it, checked: the output lists as tuples of names in their tables' order,
    gt_map_dir as None when nothing is scored."""
    keyed_noise: bool
    flow_outputs: tuple
    gt_map_dir: Optional[str]
    inverse_outputs: tuple

    @classmethod
    def from_settings(cls, settings):
        """Reads each switch once and checks it, in the table's order; an absent attribute means its default."""
        return cls(**{s.name: check(settings, s.name) for s in ROUND_TABLE})


@dataclass(frozen=True)
class ScoreKind:
    """One per-document score of a round.  `settings.<name>` holds the round's [(path, value)] and <name>.txt is its sheet."""
    name: str
    switch: Optional[str]       # the ROUND_TABLE switch that enables it; None: a metric of env.gt_dir (RunOptions.gt_metrics)
    table_columns: tuple        # what it contributes to corruption_table.txt: keys of `means`
    mean_keys: tuple            # the means logged at the end of a round, one line each ...
    mean_words: str = "mean "   # ... which opens with these words, then the key
    none: Optional[str] = None  # "mean <name>: no document of N has <none>", logged for an empty sheet; None: nothing is logged
    columns: tuple = ()         # (): the value is a float, the sheet has two columns and no header | a dict's keys: the sheet's
    integers: tuple = ()        # ... columns after `path`, under a header; these are written as integers, the others with %.6f
    logged: tuple = ()          # a dict's keys in the per-document log line
    clean_rounds: bool = True   # False: a clean round that scored nothing writes no sheet (it only left the references)

    def cell(self, value, key):
        """One value as the sheet and the log write it; a dict without `key`: a dash."""
        if self.columns and key not in value:
            return "-"
        v = value[key] if self.columns else value
        return f"{v}" if key in self.integers else f"{v:.6f}"

    def values(self, scores, key):
        """What the mean of `key` is taken over: every value of a float kind; of a dict kind the finite ones of the documents
        that have one."""
        if not self.columns:
            return [v for _, v in scores]
        return [float(s[key]) for _, s in scores if key in s and np.isfinite(s[key])]

    def means(self, scores, keys=None):
        """{key: mean} of [(path, value)] for every key of `keys` (default: the sheet's columns) that has values."""
        found = {k: self.values(scores, k) for k in ((self.columns or (self.name,)) if keys is None else keys)}
        return {k: sum(v) / len(v) for k, v in found.items() if v}


def _gt_metric(name):
    return ScoreKind(name, None, (name,), (name,), none="a ground truth in {settings.env.gt_dir}")


_MAP_SCORE_LOGGED = ("epe", "pck1", "pck5", "fl", "ause_epe")
_MAP_INVERSE_INTEGERS = ("covered", "fold_px", "flipped", "degenerate", "skipped", "tris")
# In the order corruption_table.txt lists their columns, which is also the order a round starts and summarises them in.
SCORES = (
    _gt_metric("ms_ssim"), _gt_metric("ld"), _gt_metric("ad"),
    ScoreKind("map_dev", "keyed_noise", ("map_dev",), ("map_dev",), none="a reference map from a clean round", clean_rounds=False),
    ScoreKind("map_score", "gt_map_dir", ("epe", "pck5", "ause_epe"), _MAP_SCORE_LOGGED,
              none="a ground-truth map in {settings.gt_map_dir}",
              columns=("epe", "epe_std", "pck1", "pck3", "pck5", "fl", "n_valid", "ause_epe", "ause_pck1", "ause_pck5"),
              integers=("n_valid",), logged=_MAP_SCORE_LOGGED),
    # the table's columns: fold = fold_px / covered, cycle = cycle_mean
    ScoreKind("map_inverse", "inverse_outputs", ("fold", "cycle"), ("fold", "cycle_mean", "cycle_max"), "mean map_inverse ",
              columns=_MAP_INVERSE_INTEGERS + ("cycle_mean", "cycle_max", "fold", "cycle"), integers=_MAP_INVERSE_INTEGERS,
              logged=("covered", "fold_px", "flipped", "skipped", "cycle_mean", "cycle_max")),
)
SCORE = {k.name: k for k in SCORES}
