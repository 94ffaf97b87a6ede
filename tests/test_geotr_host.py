"""CPU tests of the GeoTr init-flow prior's host side: the mirror's state_dict keys, reload_model, the option's loading
path on two gloo ranks and what the one flat weight broadcast carries."""
import json
import os
import sys

import numpy as np
import torch

from dvd_amd import prestage, synth

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLD = os.path.join(ROOT, "tests", "golden")


def test_geotr_keys_equal_the_reference():
    ref = json.load(open(os.path.join(GOLD, "geotr_keys.json")))
    assert list(prestage.GeoTr(num_attn_layers=6, num_token=1296).state_dict().keys()) == ref
    assert list(synth.geotr_spec().keys()) == ref
    # the reference's import path
    from train_settings.models.geotr.geotr_core import GeoTr_Seg_Inf, reload_model  # noqa: F401
    assert set(prestage.GeoTr_Seg_Inf().GeoTr.state_dict()) == set(ref)


def test_reload_model_module_prefixed_checkpoint(tmp_path):
    sd = synth.synth_geotr_state_dict(3)
    ckpt = {"module." + k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}
    ckpt["module.some_other_head.weight"] = torch.zeros(3)          # keys the model lacks are dropped
    ckpt["foreign.key"] = torch.ones(2)
    path = tmp_path / "doctr.pth"
    torch.save(ckpt, path)
    from train_settings.models.geotr.geotr_core import GeoTr_Seg_Inf, reload_model
    model = GeoTr_Seg_Inf()
    assert reload_model(model.GeoTr, str(path)) is model.GeoTr
    got = model.GeoTr.state_dict()
    assert all(torch.equal(got[k], torch.from_numpy(np.asarray(v))) for k, v in sd.items())
    assert model.GeoTr.bound()
    assert reload_model(model.GeoTr, "") is model.GeoTr           # empty path: unchanged, as the reference


def _settings(init_flow, path="", synthetic=False):
    import admin.settings as ws
    s = ws.Settings()
    s.env.use_init_flow, s.env.use_prestage_nets = init_flow, False
    s.env.dewarping_model_path, s.env.synthetic_weights_if_missing = path, synthetic
    s.env.seg_model_path = "missing_seg.pth"
    return s


def test_dewarping_model_path_default():
    assert _settings(False).env.dewarping_model_path == ""
    import admin.local
    assert admin.local.EnvironmentSettings().dewarping_model_path == ""


def test_broadcast_carries_geotr_once_only_with_the_flag():
    from dvd_amd import val_TDiff
    model = torch.nn.Linear(2, 2)
    off = val_TDiff.load_prestage(_settings(False).env)
    assert off is None and val_TDiff.blob_models(model, off, _settings(False).env) == [model]
    env = _settings(True, synthetic=True).env
    pre = val_TDiff.load_prestage(env)
    dewarp = pre[0]
    blobs = val_TDiff.blob_models(model, pre, env)
    assert blobs == [model, dewarp, dewarp.GeoTr]
    assert sum(m is dewarp.GeoTr for m in blobs) == 1 and dewarp.GeoTr.blob_bytes() == 4 * dewarp.GeoTr._floats


def _worker(rank, world, port, q, seg_path):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    from dvd_amd import dist_util, val_TDiff
    dist_util.setup_dist(backend="gloo")
    env = _settings(True, path="no_such_geotr.pth", synthetic=False).env
    env.seg_model_path = seg_path
    try:
        val_TDiff.load_prestage(env)
        res = (rank, "no error")
    except FileNotFoundError as e:
        res = (rank, f"FileNotFoundError {e}")
    except RuntimeError as e:
        res = (rank, f"RuntimeError {e}")
    dist_util.dist.destroy_process_group()
    q.put(res)


def test_missing_geotr_checkpoint_raises_on_every_rank(tmp_path):
    """use_init_flow with the document-mask checkpoint present and no GeoTr checkpoint: rank 0 (the only reader) fails,
    rank 1 raises with it instead of waiting in the weight broadcast."""
    from test_distributed_cpu import _spawn_ranks
    seg = tmp_path / "seg.pth"
    torch.save({"model." + k: torch.from_numpy(np.asarray(v)) for k, v in synth.synth_convnet_state_dict("u2netp", 11).items()},
               seg)
    res = _spawn_ranks(_worker, 2, (str(seg),))
    assert res[0][1].startswith("FileNotFoundError") and "no_such_geotr.pth" in res[0][1], res
    assert res[1][1].startswith("RuntimeError") and "another rank" in res[1][1], res
