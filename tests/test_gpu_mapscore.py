"""The map score on the device: the kernels of mapscore.hip against tests/mapscore_model.py under the bars of
tests/mapscore_fixtures.py - planes, order statistics and integer sums bit for bit, the two f64 sums within 1e-9 - and one run of
the document loop scored against the maps it wrote itself."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mapscore_model as M  # noqa: E402

from mapscore_fixtures import (CASES, F, ODD_SHAPES, check_against_model, check_against_reference, document, golden,  # noqa: E402
                               golden_planes, key_sets)

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t):
    return t.contiguous().view(torch.int32).cpu().numpy().view(np.uint32).ravel()


def _plane(bits):
    return _dev(bits.view(F))


@pytest.mark.parametrize("name", CASES)
def test_kernels_on_the_goldens(name):
    """The goldens' fields through the kernels: equal to the model, and under the model's bars against the real reference."""
    from dvd_amd import ops
    pred, gt, sigma, ref = golden(name)
    planes, _ = golden_planes(name)
    e, zero = ops.map_errors(_dev(pred), _dev(gt))
    assert np.array_equal(_bits(e), planes["e"]) and np.array_equal(_bits(zero), np.where(planes["valid"], np.uint32(0), M.INVALID))
    got = ops.map_metrics(_dev(pred), _dev(gt))
    got.update(ops.sparsification(e, _plane(planes["sigma"]), got["n_valid"]))
    check_against_model(got, M.score(planes))
    check_against_reference(got, ref)
    assert ops.map_valid_count(e) == got["n_valid"]
    assert ops.sparsification(e, _plane(planes["sigma"]))["AUSE"] == got["AUSE"]          # n_valid counted on the device


@pytest.mark.parametrize("h,w", ODD_SHAPES + ((1024, 768),))
def test_kernels_equal_the_model_on_odd_sizes(h, w):
    """One pixel, one row, one column, a short last group, several workgroups, and 768 block partials for the finalize."""
    from dvd_amd import ops
    flow, gt, hyps = document(h, w, n_hyp=2 if h * w > 100000 else 3)
    planes = M.errors_of_maps(flow, gt, hyps, h, w)
    e, sigma = ops.map_errors(_dev(flow), _dev(gt), _dev(hyps))
    assert tuple(e.shape) == (h, w) and np.array_equal(_bits(e), planes["e"]) and np.array_equal(_bits(sigma), planes["sigma"])
    check_against_model(ops.map_score(_dev(flow), _dev(gt), _dev(hyps)), M.score(planes))
    if h * w <= 100000:
        coarse = document(h, w, seed=5)[0]                                                # a coarse ground truth, as a .npy holds it
        check_against_model(ops.map_score(_dev(flow), _dev(coarse), _dev(hyps), size=(h, w)),
                            M.score(M.errors_of_maps(flow, coarse, hyps, h, w)))
        none = ops.map_score(_dev(flow), _dev(np.full((h, w, 2), np.nan, F)), _dev(hyps))  # no valid pixel: no curve, NaN scores
        assert none["n_valid"] == 0 and np.isnan(none["epe"]) and "AUSE" not in none


@pytest.mark.parametrize("name", sorted(key_sets()))
def test_selection_against_sort_on_hostile_keys(name):
    from dvd_amd import ops
    keys = key_sets()[name]
    valid = np.sort(keys[keys != M.INVALID])[::-1]
    n = len(valid)
    dev = _plane(keys)
    for ranks in ([0], [n - 1], [n - 1, 0, n // 2, 0], M.ranks_desc(n), list(np.linspace(0, n - 1, 50).astype(int))):
        assert np.array_equal(_bits(ops.select_kth_desc(dev, ranks)), valid[ranks]), (name, ranks[:4])
    assert ops.map_valid_count(dev) == n
    for bad in ([n], [-1], [], list(range(51)), [0.5]):
        with pytest.raises(ValueError, match="ranks"):
            ops.select_kth_desc(dev, bad, n)


def test_a_document_alone_equals_the_document_after_another():
    """Nothing of a call outlives it: the second document's score is what it scores on its own."""
    from dvd_amd import ops
    a, b = document(257, 263), document(33, 31, seed=3)
    alone = ops.map_score(*(_dev(x) for x in b))
    ops.map_score(*(_dev(x) for x in a))
    after = ops.map_score(*(_dev(x) for x in b))
    assert {k: v for k, v in alone.items() if not isinstance(v, dict)} == {k: v for k, v in after.items() if not isinstance(v, dict)}
    for m in M.METRICS:
        assert np.array_equal(alone["sparse_curve"][m], after["sparse_curve"][m]) and alone["AUSE"][m] == after["AUSE"][m]


def test_a_map_scored_against_its_own_flo_file(tmp_path):
    from dvd_amd import ops
    flow, _, hyps = document(96, 80, g=16)
    ops.flow_write_flo(_dev(flow), 96, 80, str(tmp_path / "own.flo"))
    got = ops.map_score(_dev(flow), _dev(ops.flow_read_flo(str(tmp_path / "own.flo"))), _dev(hyps))
    assert got["epe"] == 0.0 and got["epe_std"] == 0.0 and got["pck1"] == 1.0 and got["fl"] == 0.0 and got["n_valid"] == 96 * 80
    assert got["sum_e"] == 0.0 and np.all(got["opt_curve"]["EPE"] == 0.0)


def test_one_hypothesis_skips_the_sparsification():
    from dvd_amd import ops
    flow, gt, hyps = document(33, 31)
    for h in (None, _dev(hyps[:1])):
        got = ops.map_score(_dev(flow), _dev(gt), h)
        assert "AUSE" not in got and "ause_epe" not in got
        check_against_model(got, M.score(M.errors_of_maps(flow, gt, None, 33, 31), sparsify=False))
    e, sigma = ops.map_errors(_dev(flow), _dev(gt))
    assert set(np.unique(_bits(sigma)).tolist()) == {0, int(M.INVALID)}


def test_refused_shapes_launch_nothing(monkeypatch):
    from dvd_amd import lib, ops
    flow, gt, hyps = (_dev(x) for x in document(9, 11))
    real = lib.call
    calls = []
    monkeypatch.setattr(lib, "call", lambda name, *a: calls.append(name) or real(name, *a))
    for args, kw in (((flow[:, :, :7].contiguous(), gt), {}), ((flow, gt[:, :, :1].contiguous()), {}), ((flow, gt, hyps[:, :, :7].contiguous()), {}),
                     ((flow, flow), {"size": (0, 4)}), ((flow, flow), {"size": (4, 16385)}), ((flow.cpu(), gt), {}), ((flow, gt.cpu()), {}),
                     ((flow, gt, hyps.cpu()), {}), ((flow.double(), gt), {})):
        with pytest.raises(ValueError):
            ops.map_score(*args, **kw)
    assert calls == []
    raw, p = lib.raw(), lib.ptr
    ws = torch.empty(raw.dvd_mapscore_workspace_bytes(9, 11), dtype=torch.uint8, device="cuda")
    e = torch.zeros(99, device="cuda")
    for g, gt_g, n_hyp, h, w in ((1, 0, 1, 9, 11), (8, 1, 1, 9, 11), (8, 0, 65, 9, 11), (8, 0, 1, 0, 11), (8, 0, 1, 9, 16385), (0, 0, 2, 9, 11)):
        assert raw.dvd_map_errors(p(flow), g, p(gt), gt_g, p(hyps), n_hyp, h, w, p(e), p(e), p(ws), None) == lib.E_MAP_SHAPE
    assert raw.dvd_select_u32(p(e), 99, (lib.C.c_uint32 * 2)(98, 99), 2, p(e), p(ws), None) == lib.E_MAP_RANKS
    assert raw.dvd_sparsify_bins(p(e), p(e), 99, p(e), 0, p(ws), p(ws), None) == lib.E_MAP_RANKS
    torch.cuda.synchronize()
    assert float(e.abs().sum()) == 0.0                                                    # nothing was written


# ---- end to end ---------------------------------------------------------------------------------------------------------------
PATHS = ["synthetic_00000", "synthetic_00001"]
SIZE = (96, 80)


def _launcher(monkeypatch, tmp_path):
    import types
    import admin.settings as ws
    import run_sampling as R
    monkeypatch.chdir(tmp_path)
    made = []

    class Small(ws.Settings):
        def __init__(self):
            super().__init__()
            self.env.grid_size, self.env.diffusion_steps = 16, 2
            self.env.num_synthetic_docs, self.env.batch_docs, self.env.full_res = 2, 2, SIZE
            self.env.visualize, self.env.use_prestage_nets = True, True
            self.env.eval_dataset_name = "synthetic"
            made.append(self)
    monkeypatch.setattr(R, "ws_settings", types.SimpleNamespace(Settings=Small))
    monkeypatch.setattr(R, "shutil", types.SimpleNamespace(copyfile=lambda *a: None))
    return R, made


def test_a_run_scored_against_the_maps_it_wrote_itself(tmp_path, monkeypatch):
    """G = 16, 2 steps, synthetic weights, two synthetic documents, keyed noise (two runs sample the same maps).  The first pass
    writes its maps; the second pass has as ground truth document 0's own .flo file - it scores exactly 0 - and, under document
    1's name, the coarse .npy of document 0: that score is the model's."""
    import shutil
    R, made = _launcher(monkeypatch, tmp_path)
    R.run_sampling("dvd", "val_TDiff", 77, "first", keyed_noise=True, flow_outputs="flo,npy")
    wrote = tmp_path / "vis_hp" / "synthetic" / "first" / "pred_flow"
    maps = tmp_path / "maps"
    maps.mkdir()
    shutil.copy(wrote / f"flow_{PATHS[0]}.flo", maps / f"flow_{PATHS[0]}.flo")
    a, b = (np.load(wrote / f"flow_{p}.npy") for p in PATHS)
    np.save(maps / f"{PATHS[1]}.npy", a)
    R.run_sampling("dvd", "val_TDiff", 77, "second", keyed_noise=True, gt_map_dir=str(maps))
    first, second = made
    assert not hasattr(first, "gt_map_dir") and not hasattr(first, "map_score") and second.gt_map_dir == str(maps)
    assert [p for p, _ in second.map_score] == PATHS
    own, crossed = (s for _, s in second.map_score)
    assert own["epe"] == 0.0 and own["epe_std"] == 0.0 and own["pck1"] == 1.0 and own["fl"] == 0.0 and own["n_valid"] == SIZE[0] * SIZE[1]
    assert ("ause_epe" in own) == (second.env.n_batch >= 2) == ("ause_epe" in crossed)
    want = M.score(M.errors_of_maps(b, a, None, *SIZE), sparsify=False)              # the .npy is evaluated at the page's size
    assert crossed["epe"] > 0 and abs(crossed["epe"] - want["epe"]) <= 1e-9 * want["epe"]
    for k in ("n_valid", "pck1", "pck3", "pck5", "fl"):
        assert crossed[k] == want[k], k
    text = (tmp_path / "vis_hp" / "synthetic" / "second" / "map_score.txt").read_text().splitlines()
    assert len(text) == 3 and text[1].startswith(f"{PATHS[0]} 0.000000 0.000000 1.000000") and text[2].startswith(f"{PATHS[1]} {crossed['epe']:.6f}")
    assert not (tmp_path / "vis_hp" / "synthetic" / "first" / "map_score.txt").exists()
    for p in PATHS:                                                                    # the pages are what they are without the attribute
        assert (tmp_path / "vis_hp/synthetic/first/dewarped_pred" / f"warped_{p}.png").read_bytes() == \
            (tmp_path / "vis_hp/synthetic/second/dewarped_pred" / f"warped_{p}.png").read_bytes()
