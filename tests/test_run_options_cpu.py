"""The engine-side switches (dvd_amd/run_options.py) without a GPU: the defaults, one parse, and - for every switch and every bad
value - a refusal before the loader is read and before anything is written.  The same for the round's switches, the attributes
the launcher puts on `settings` itself."""
import dataclasses
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import admin.settings as ws
from dvd_amd import logger
from dvd_amd.run_options import ROUND_TABLE, TABLE, PageOptions, RoundOptions, RunOptions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# written out, not read from the table under test
ENGINE_DEFAULTS = {
    "grid_size": 64, "batch_docs": 1, "sampler": "ddim", "unwarp_mode": "bilinear", "gt_dir": "", "metric_preset": "docunet",
    "gt_metrics": "ms_ssim", "gt_ad": False, "png_encoder": "pil", "png_huffman": "fixed", "page_format": "png",
    "jpeg_quality": 90, "jpeg_subsampling": "420", "image_decoder": "pil", "png_decoder": "pil", "num_synthetic_docs": 4,
    "full_res": (1024, 768), "conditioning_dir": "", "num_workers": 0, "use_prestage_nets": True,
    "synthetic_weights_if_missing": None, "dewarping_model_path": ""}
REFERENCE_SURFACE = 43                      # attributes of EnvironmentSettings() that are not engine-side switches

# switch -> (what the message must hold, the bad values, other settings the case needs); in the order the values are checked
BAD = {
    "unwarp_mode": ("env.unwarp_mode must be 'bilinear' or 'bicubic'", ("nearest", "cubic", "BICUBIC", None), {}),
    "png_encoder": ("env.png_encoder must be 'pil' or 'hip'", ("zlib", "", None, "HIP"), {}),
    "png_huffman": ("env.png_huffman must be 'fixed' or 'dynamic'", ("optimal", "best", "", None, 1, "Dynamic"),
                    {"png_encoder": "hip"}),
    "page_format": ("env.page_format must be 'png' or 'jpeg'", ("tiff", "jpg", None), {}),
    "jpeg_quality": ("env.jpeg_quality must be an integer 1..100", (0, 101, -1, 90.0, "90", True, None), {"page_format": "jpeg"}),
    "jpeg_subsampling": ("env.jpeg_subsampling must be '420' or '444'", ("422", 420, None), {"page_format": "jpeg"}),
    "image_decoder": ("env.image_decoder must be 'pil' or 'hip'", ("cuda", "", None, "HIP"), {}),
    "png_decoder": ("env.png_decoder must be 'pil' or 'hip'", ("cuda", "", None, "HIP"), {}),
    "gt_metrics": ("env.gt_metrics must be a comma-separated list", ("", "ssim", "ms_ssim,ad", "ld,ld", "ms_ssim;ld", None, ("ld",)),
                   {}),
    "gt_ad": ("env.gt_ad must be True or False", ("yes", 1, 0, None, "ad", ("ad",)), {}),
    "metric_preset": ("env.metric_preset: preset must be 'docunet' or 'wang'", ("ssim", "", None), {"gt_dir": "scans"}),
}
PAGE_WRITER = ("png_encoder", "png_huffman", "page_format", "jpeg_quality", "jpeg_subsampling")
CASES = [pytest.param(key, value, id=f"{key}-{value!r}") for key, (_, values, _) in BAD.items() for value in values]


def _settings(**env):
    s = ws.Settings()
    s.name = "pytest_run_options"
    for key, value in env.items():
        setattr(s.env, key, value)
    return s


def _unread_loader():
    raise AssertionError("the loader was read")
    yield


def _refused(s, text):
    """Both entry points' checks as one harness: a ValueError that holds `text`."""
    from train_settings.dvd.evaluation import run_evaluation_docunet
    with pytest.raises(ValueError) as e:
        run_evaluation_docunet(s, logger, _unread_loader(), None, torch.nn.Linear(1, 1), None)
    assert text in str(e.value)
    return str(e.value)


@pytest.mark.parametrize("key,value", CASES)
def test_bad_value_is_refused(tmp_path, monkeypatch, key, value):
    """Before the loader is read and before anything is written: by run_evaluation_docunet for every switch, and by
    visualize_dewarping itself for the page writer's."""
    monkeypatch.chdir(tmp_path)
    text, _, needs = BAD[key]
    s = _settings(**needs, **{key: value})
    assert repr(value) in _refused(s, text)
    with pytest.raises(ValueError) as e:
        RunOptions.from_env(s.env)
    assert text in str(e.value)
    if key in PAGE_WRITER:
        from utils_flow.visualization_utils import visualize_dewarping
        with pytest.raises(ValueError) as e:
            visualize_dewarping(s, None, None, 0, None, ["a.png"], warped_u8=np.zeros((2, 2, 3), np.uint8))
        assert text in str(e.value)
        with pytest.raises(ValueError):
            PageOptions.from_env(s.env)
    assert list(tmp_path.iterdir()) == []


def test_every_checked_switch_has_bad_values():
    assert {s.name for s in TABLE if s.accepts is not None} == set(BAD)
    assert set(PAGE_WRITER) == {f.name for f in dataclasses.fields(PageOptions)}


def test_defaults_are_the_literal_ones():
    env = vars(ws.Settings().env)
    assert {k: env[k] for k in ENGINE_DEFAULTS} == ENGINE_DEFAULTS
    assert {s.name: s.default for s in TABLE} == ENGINE_DEFAULTS and all(s.doc for s in TABLE)
    assert len(env) == len(ENGINE_DEFAULTS) + REFERENCE_SURFACE
    opts = RunOptions.from_env(ws.Settings().env)
    assert dataclasses.asdict(opts) == dict(ENGINE_DEFAULTS, gt_metrics=("ms_ssim",))
    assert opts.page_writer == "pil"


@pytest.mark.parametrize("name", list(ENGINE_DEFAULTS))
def test_an_absent_attribute_means_its_default(name):
    env = ws.Settings().env
    delattr(env, name)
    assert not hasattr(env, name)
    assert RunOptions.from_env(env) == RunOptions.from_env(ws.Settings().env)
    if name in PAGE_WRITER:
        assert PageOptions.from_env(env) == PageOptions.from_env(ws.Settings().env)


def test_of_two_bad_values_the_earlier_one_is_reported(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    order = ("unwarp_mode", "png_encoder", "png_huffman", "page_format", "jpeg_quality", "jpeg_subsampling", "image_decoder",
             "png_decoder", "gt_metrics", "gt_ad", "metric_preset")
    assert set(order) == set(BAD)
    for i, first in enumerate(order):
        for second in order[i + 1:]:
            s = _settings(gt_dir="scans", **{first: BAD[first][1][0], second: BAD[second][1][0]})
            assert f"env.{second}" not in _refused(s, f"env.{first}")
    page = [k for k in order if k in PAGE_WRITER]
    for i, first in enumerate(page):
        for second in page[i + 1:]:
            with pytest.raises(ValueError, match=f"env.{first}"):
                PageOptions.from_env(_settings(**{first: BAD[first][1][0], second: BAD[second][1][0]}).env)
    assert list(tmp_path.iterdir()) == []


# ---- the round's switches: what the launcher puts on `settings` itself (ROUND_TABLE) ---------------------------------------------
ROUND_DEFAULTS = {"keyed_noise": False, "flow_outputs": "", "gt_map_dir": "", "inverse_outputs": ""}     # written out, as above
ROUND_PARSED = {"keyed_noise": False, "flow_outputs": (), "gt_map_dir": None, "inverse_outputs": ()}
# switch -> (the message, the bad values); in the order the values are checked
ROUND_BAD = {
    "keyed_noise": ("settings.keyed_noise must be True or False, got ", (1, 0, "yes", None, 1.0)),
    "flow_outputs": ("settings.flow_outputs must be a comma-separated list of ('png', 'flo', 'npy') without repeats, got ",
                     ("jpg", "png,png", "png,", ",", " ", "PNG", None, True, 3, ("png",), ["png"])),
    "gt_map_dir": ("settings.gt_map_dir must be an existing directory (or \"\" for none), got ",
                   (1, None, True, ["maps"], "missing", b"maps")),
    "inverse_outputs": ("settings.inverse_outputs must be a comma-separated list of ('mesh', 'flo', 'mask') without repeats, got ",
                        ("png", "mesh,mesh", "mesh,", ",", " ", "MESH", None, True, 3, ("mesh",), ["mesh"])),
}
ROUND_CASES = [pytest.param(key, value, id=f"{key}-{value!r}") for key, (_, values) in ROUND_BAD.items() for value in values]


def _round_settings(env=None, **attrs):
    s = _settings(**(env or {}))
    for key, value in attrs.items():
        setattr(s, key, value)
    return s


@pytest.mark.parametrize("key,value", ROUND_CASES)
def test_bad_round_value_is_refused(tmp_path, monkeypatch, key, value):
    """By run_evaluation_docunet, before the loader is read and before anything is written; the whole message."""
    monkeypatch.chdir(tmp_path)
    s = _round_settings(**{key: value})
    assert _refused(s, "settings.") == ROUND_BAD[key][0] + repr(value)
    with pytest.raises(ValueError) as e:
        RoundOptions.from_settings(s)
    assert str(e.value) == ROUND_BAD[key][0] + repr(value)
    assert list(tmp_path.iterdir()) == []


def test_every_checked_round_switch_has_bad_values():
    assert [s.name for s in ROUND_TABLE if s.accepts is not None] == list(ROUND_BAD) == list(ROUND_DEFAULTS)
    assert {f.name for f in dataclasses.fields(RoundOptions)} == set(ROUND_DEFAULTS)
    assert not {s.name for s in ROUND_TABLE} & {s.name for s in TABLE}


def test_round_defaults_are_the_literal_ones(tmp_path):
    assert {s.name: s.default for s in ROUND_TABLE} == ROUND_DEFAULTS and all(s.doc and s.owner == "settings" for s in ROUND_TABLE)
    assert all(s.owner == "env" for s in TABLE)
    assert not any(hasattr(ws.Settings(), name) for name in ROUND_DEFAULTS)              # the launcher leaves them absent
    assert dataclasses.asdict(RoundOptions.from_settings(ws.Settings())) == ROUND_PARSED
    assert RoundOptions.from_settings(_round_settings(**ROUND_DEFAULTS)) == RoundOptions.from_settings(ws.Settings())
    given = RoundOptions.from_settings(_round_settings(keyed_noise=np.True_, flow_outputs="npy, png", gt_map_dir=str(tmp_path),
                                                       inverse_outputs="mask,mesh"))
    assert dataclasses.astuple(given) == (True, ("png", "npy"), str(tmp_path), ("mesh", "mask")) and type(given.keyed_noise) is bool
    with pytest.raises(dataclasses.FrozenInstanceError):
        given.keyed_noise = False


@pytest.mark.parametrize("name", list(ROUND_DEFAULTS))
def test_an_absent_round_attribute_means_its_default(name):
    s = _round_settings(keyed_noise=True, flow_outputs="png", gt_map_dir=ROOT, inverse_outputs="mesh")
    delattr(s, name)
    assert getattr(RoundOptions.from_settings(s), name) == ROUND_PARSED[name]


def test_of_two_bad_round_values_the_earlier_one_is_reported(tmp_path, monkeypatch):
    """The env.* switches first, then the corruption, then the round's switches in ROUND_TABLE order."""
    monkeypatch.chdir(tmp_path)
    order = list(ROUND_BAD)
    for i, first in enumerate(order):
        for second in order[i + 1:]:
            s = _round_settings(**{first: ROUND_BAD[first][1][0], second: ROUND_BAD[second][1][0]})
            assert f"settings.{second}" not in _refused(s, f"settings.{first}")
    for key in order:
        s = _round_settings({"unwarp_mode": "nearest"}, **{key: ROUND_BAD[key][1][0]})
        assert "settings." not in _refused(s, "env.unwarp_mode must be 'bilinear' or 'bicubic'")
        s = _round_settings(severity=9, **{key: ROUND_BAD[key][1][0]})
        assert f"settings.{key}" not in _refused(s, "settings.severity")
    assert list(tmp_path.iterdir()) == []


def test_one_name_list_checker():
    """env.gt_metrics refuses ""; the two lists of `settings` read it as none."""
    from dvd_amd import run_options
    check = run_options.name_list("x.names", ("a", "b", "c"))
    assert check("c, a") == ("a", "c") and run_options.name_list("x.names", ("a", "b"), empty_is_none=True)("") == ()
    for bad in ("", "a,a", "a,", "d", None, ("a",)):
        with pytest.raises(ValueError) as e:
            check(bad)
        assert str(e.value) == f"x.names must be a comma-separated list of ('a', 'b', 'c') without repeats, got {bad!r}"


def test_metric_preset_is_checked_only_with_gt_dir():
    assert RunOptions.from_env(_settings(metric_preset="ssim").env).metric_preset == "ssim"
    assert RunOptions.from_env(_settings(metric_preset="wang", gt_dir="scans").env).metric_preset == "wang"


def test_run_options_are_frozen():
    opts = RunOptions.from_env(ws.Settings().env)
    for name, value in (("unwarp_mode", "bicubic"), ("gt_metrics", ()), ("page_writer", "hip")):
        with pytest.raises((dataclasses.FrozenInstanceError, AttributeError)):
            setattr(opts, name, value)
    with pytest.raises(dataclasses.FrozenInstanceError):
        del opts.gt_dir
    assert opts == RunOptions.from_env(ws.Settings().env) and hash(opts) == hash(RunOptions.from_env(ws.Settings().env))


@pytest.mark.parametrize("text,gt_ad,want", [
    ("ms_ssim", False, ("ms_ssim",)), ("ms_ssim", True, ("ms_ssim", "ad")), ("ld", False, ("ld",)), ("ld", True, ("ld", "ad")),
    ("ms_ssim,ld", False, ("ms_ssim", "ld")), ("ld, ms_ssim", True, ("ms_ssim", "ld", "ad"))])
def test_derived_metrics(text, gt_ad, want):
    opts = RunOptions.from_env(_settings(gt_metrics=text, gt_ad=gt_ad).env)
    assert opts.gt_metrics == want and opts.gt_ad is gt_ad


def test_derived_page_writer_and_parsed_quality():
    for encoder in ("pil", "hip"):
        assert RunOptions.from_env(_settings(png_encoder=encoder).env).page_writer == encoder
        assert PageOptions.from_env(_settings(png_encoder=encoder, page_format="jpeg").env).page_writer == "jpeg"
    quality = RunOptions.from_env(_settings(jpeg_quality=np.int64(75)).env).jpeg_quality
    assert quality == 75 and type(quality) is int


def test_validators_keep_their_names_and_return_values():
    from dvd_amd.evaluation import parse_gt_metrics, png_decoder_setting
    from utils_flow.visualization_utils import page_settings, png_huffman_setting
    env = _settings(jpeg_quality=np.int64(75), jpeg_subsampling="444", png_decoder="hip", png_huffman="dynamic").env
    assert page_settings(env) == ("png", 75, "444") and type(page_settings(env)[1]) is int
    assert png_huffman_setting(env) == "dynamic" and png_decoder_setting(env) == "hip"
    assert parse_gt_metrics("ld, ms_ssim") == ("ms_ssim", "ld")
    bare = type("Env", (), {})()
    assert page_settings(bare) == ("png", 90, "420") and png_huffman_setting(bare) == "fixed" and png_decoder_setting(bare) == "pil"


def test_the_loop_and_the_parse_import_neither_utils_flow_nor_datasets():
    """`import dvd_amd.evaluation` and RunOptions.from_env, in a fresh interpreter."""
    code = ("import sys\n"
            "import dvd_amd.evaluation\n"
            "from dvd_amd.run_options import RunOptions\n"
            "import admin.settings as ws\n"
            "RunOptions.from_env(ws.Settings().env)\n"
            "bad = sorted(m for m in sys.modules if m.split('.')[0] in ('utils_flow', 'datasets'))\n"
            "assert not bad, bad\n")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.environ.get("PYTHONPATH", "")]))
    res = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-3000:]
