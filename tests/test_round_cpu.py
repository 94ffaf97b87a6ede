"""The document loop with every round switch at once, and the table of score kinds, without a GPU: the exact log lines, files and
score sheets of a clean and then a corrupted round of run_evaluation_docunet on stand-ins (one batch of two documents, G = 9
maps, pages 40 x 30), and the launcher's corruption table against dvd_amd.run_options.SCORES for every subset of its flags."""
import itertools
import os
import types

import numpy as np
import pytest
import torch

H, W, G = 40, 30, 9
PATHS = ("dir/a_1 copy.jpg", "synthetic_00001")
ROUND = "pytest_round/c00_gaussian_noise_s5"


class _Ops:
    """dvd_amd.ops: the host-side corruption helpers as they are, every device entry recorded and answered with fixed values."""
    REAL = ("CORRUPTIONS", "CorruptionUnsupported", "PNG_SIGNATURE", "corruption_key", "corruption_number", "corruption_severity",
            "corruption_supported")

    def __init__(self, real):
        self._real, self.calls = real, []

    def __getattr__(self, name):
        if name in self.REAL:
            return getattr(self._real, name)
        raise AssertionError(f"ops.{name} was called")

    def _file(self, name, path):
        self.calls.append(f"{name} {path}")
        open(path, "wb").close()

    def map_deviation(self, ref, got):
        self.calls.append(f"map_deviation {len(ref)}")
        return [0.5 + j for j in range(len(ref))]

    def map_score(self, flow, gt, hyps=None, size=None):
        self.calls.append(f"map_score {tuple(gt.shape)} {tuple(hyps.shape)} {size}")
        return {"epe": 1.5, "epe_std": 0.5, "pck1": 0.25, "pck3": 0.5, "pck5": 0.75, "fl": 0.125, "n_valid": 1200, "ause_epe": 0.0625}

    def map_invert(self, flow, h, w):
        n = sum(c.startswith("map_invert") for c in self.calls)
        self.calls.append(f"map_invert {h} {w}")
        return torch.zeros(h, w, 2), {"covered": 1000 * (n % 2), "fold_px": 10 * (n % 2), "flipped_tris": 1, "degenerate_tris": 0,
                                      "skipped_tris": 2, "tris": 128}

    def map_cycle_error(self, flow, fwd):
        self.calls.append("map_cycle_error")
        return {"cycle_mean": 0.125, "cycle_max": 0.5, "n": 1000}

    def coverage_mask(self, fwd):
        self.calls.append("coverage_mask")
        return "MASK"

    def mesh_overlay_to_file(self, src, fwd, path, huffman="fixed"):
        self._file(f"mesh_overlay_to_file {tuple(src.shape)} {huffman}", path)

    def inverse_write_flo(self, fwd, path):
        self._file("inverse_write_flo", path)

    def png_encode_to_file(self, img, path, huffman="fixed"):
        self._file(f"png_encode_to_file {img} {huffman}", path)

    def flow_picture_to_file(self, flow, h, w, path, norm="max", huffman="fixed", return_radius=False):
        self._file(f"flow_picture_to_file {h} {w} {norm} {huffman}", path)
        return 12, 1.5

    def flow_write_flo(self, flow, h, w, path):
        self._file(f"flow_write_flo {h} {w}", path)

    def gt_metrics_u8(self, out, gt, metrics, preset="docunet"):
        self.calls.append(f"gt_metrics_u8 {tuple(gt.shape)} {metrics} {preset}")
        return {"ms_ssim": 0.75, "ld": 3.5}


def _files(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, names in os.walk(root) for f in names)


def _round(monkeypatch, evaluation, s, spy):
    """One round of run_evaluation_docunet on stand-ins for everything around the switches' own code: the log lines, and the
    keywords prepare_conditioning and sample_batch were called with."""
    batch = [{"path": PATHS[0], "src_u8": torch.zeros(H, W, 3, dtype=torch.uint8)},
             {"path": PATHS[1], "source_vis": torch.full((3, H, W), 300.0)}]
    flow = torch.arange(2 * 2 * G * G, dtype=torch.float32).reshape(2, 2, G, G) / 1000
    seen = {}

    def sample(*a, **kw):
        seen["sample_batch"] = kw
        return (flow, flow.repeat_interleave(2, 0)) if kw.get("keep_hypotheses") else flow
    monkeypatch.setattr(evaluation, "batches_of", lambda loader, n: iter([batch]))
    monkeypatch.setattr(evaluation, "adopt_reference_items", lambda *a, **k: None)
    monkeypatch.setattr(evaluation, "prepare_conditioning", lambda *a, **kw: seen.update(prepare_conditioning=kw))
    monkeypatch.setattr(evaluation, "sample_batch", sample)
    monkeypatch.setattr(evaluation, "unwarp_tail", lambda *a, **k: [torch.zeros(H, W, 3, dtype=torch.uint8)] * 2)
    monkeypatch.setattr(evaluation.th.cuda, "synchronize", lambda: None)
    lines = []
    spy.calls.clear()
    results = evaluation.run_evaluation_docunet(s, types.SimpleNamespace(info=lines.append), None, None, torch.nn.Linear(1, 1), None)
    assert [p for p, _ in results] == list(PATHS)
    return lines, seen


SHEET_HEAD = {"map_score": "path epe epe_std pck1 pck3 pck5 fl n_valid ause_epe ause_pck1 ause_pck5\n",
              "map_inverse": "path covered fold_px flipped degenerate skipped tris cycle_mean cycle_max fold cycle\n"}
MAP_SCORE_ROW = "dir/a_1 copy.jpg 1.500000 0.500000 0.250000 0.500000 0.750000 0.125000 1200 0.062500 - -\n"
PER_DOCUMENT = [
    "dir/a_1 copy.jpg map_score epe 1.500000 pck1 0.250000 pck5 0.750000 fl 0.125000 ause_epe 0.062500",
    "synthetic_00001 map_score skipped: no ground-truth map in maps",
    "dir/a_1 copy.jpg map_inverse covered 0 fold_px 0 flipped 1 skipped 2 cycle_mean 0.125000 cycle_max 0.500000",
    "synthetic_00001 map_inverse covered 1000 fold_px 10 flipped 1 skipped 2 cycle_mean 0.125000 cycle_max 0.500000",
    "dir/a_1 copy.jpg flow_rad_max 1.500000",
    "dir/a_1 copy.jpg ms_ssim 0.750000",
    "dir/a_1 copy.jpg ld 3.500000",
    "synthetic_00001 flow_rad_max 1.500000",
    "synthetic_00001 ms_ssim,ld skipped: no ground truth in scans"]
MEANS = [
    "mean ms_ssim 0.750000 over 1 of 2 documents",
    "mean ld 3.500000 over 1 of 2 documents",
    "mean epe 1.500000 over 1 of 2 documents",
    "mean pck1 0.250000 over 1 of 2 documents",
    "mean pck5 0.750000 over 1 of 2 documents",
    "mean fl 0.125000 over 1 of 2 documents",
    "mean ause_epe 0.062500 over 1 of 2 documents",
    "mean map_inverse fold 0.010000 over 1 of 2 documents",
    "mean map_inverse cycle_mean 0.125000 over 2 of 2 documents",
    "mean map_inverse cycle_max 0.500000 over 2 of 2 documents"]
MAP_DEV = ["dir/a_1 copy.jpg map_dev 0.500000", "synthetic_00001 map_dev 1.500000"]
SHEETS = {"ms_ssim.txt": "dir/a_1 copy.jpg 0.750000\n", "ld.txt": "dir/a_1 copy.jpg 3.500000\n",
          "map_score.txt": SHEET_HEAD["map_score"] + MAP_SCORE_ROW,
          "map_inverse.txt": SHEET_HEAD["map_inverse"] +
          "dir/a_1 copy.jpg 0 0 1 0 2 128 0.125000 0.500000 nan 0.125000\n"
          "synthetic_00001 1000 10 1 0 2 128 0.125000 0.500000 0.010000 0.125000\n"}
PRED_FLOW = sorted(f"pred_flow/{kind}_{stem}.{ext}" for stem in ("a_1 copy", "synthetic_00001")
                   for kind, ext in (("flow", "png"), ("flow", "flo"), ("flow", "npy"), ("mesh", "png"), ("inv", "flo"), ("mask", "png")))
OPS_CALLS = [
    "map_score (2, 9, 9) (2, 2, 9, 9) (40, 30)",
    "map_invert 40 30", "map_cycle_error", "mesh_overlay_to_file (40, 30, 3) fixed {run}/pred_flow/mesh_a_1 copy.png",
    "inverse_write_flo {run}/pred_flow/inv_a_1 copy.flo", "coverage_mask", "png_encode_to_file MASK fixed {run}/pred_flow/mask_a_1 copy.png",
    "map_invert 40 30", "map_cycle_error", "mesh_overlay_to_file (40, 30, 3) fixed {run}/pred_flow/mesh_synthetic_00001.png",
    "inverse_write_flo {run}/pred_flow/inv_synthetic_00001.flo", "coverage_mask",
    "png_encode_to_file MASK fixed {run}/pred_flow/mask_synthetic_00001.png",
    "flow_picture_to_file 40 30 max fixed {run}/pred_flow/flow_a_1 copy.png", "flow_write_flo 40 30 {run}/pred_flow/flow_a_1 copy.flo",
    "gt_metrics_u8 (4, 3, 3) ('ms_ssim', 'ld') docunet",
    "flow_picture_to_file 40 30 max fixed {run}/pred_flow/flow_synthetic_00001.png",
    "flow_write_flo 40 30 {run}/pred_flow/flow_synthetic_00001.flo"]


def test_all_switches_at_once_over_a_clean_and_a_corrupted_round(tmp_path, monkeypatch):
    """keyed_noise, flow_outputs, gt_map_dir, inverse_outputs and two env.gt_dir metrics together: what is logged, in which order,
    which files appear and what every score sheet holds."""
    import admin.settings as ws
    from PIL import Image
    from dvd_amd import evaluation
    monkeypatch.chdir(tmp_path)
    spy = _Ops(evaluation.ops)
    monkeypatch.setattr(evaluation, "ops", spy)
    os.makedirs("scans")
    os.makedirs("maps")
    Image.fromarray(np.zeros((4, 3, 3), np.uint8)).save("scans/a_1 copy.png")
    np.save("maps/flow_a_1 copy.npy", np.zeros((2, G, G), np.float32))
    s = ws.Settings()
    s.name, s.seed = "pytest_round", 5
    s.keyed_noise, s.flow_outputs, s.gt_map_dir, s.inverse_outputs = True, "npy,png,flo", "maps", "mask,mesh,flo"
    s.env.visualize, s.env.eval_dataset_name, s.env.gt_dir, s.env.gt_metrics = False, "synthetic", "scans", "ld,ms_ssim"

    lines, seen = _round(monkeypatch, evaluation, s, spy)                                  # the clean round
    for line in lines:
        print(line)
    assert seen == {"prepare_conditioning": {"decode_png": False}, "sample_batch": {"keyed_noise": True, "keep_hypotheses": True}}
    assert lines == PER_DOCUMENT + MEANS
    run = "vis_hp/synthetic/pytest_round"
    assert spy.calls == [c.format(run=run) for c in OPS_CALLS]
    assert _files(run) == sorted(PRED_FLOW + list(SHEETS))                                 # no map_dev.txt: nothing was scored
    for name, text in SHEETS.items():
        assert open(f"{run}/{name}").read() == text, name
    assert s.map_dev == [] and set(s.map_ref) == set(PATHS)
    assert [len(getattr(s, k)) for k in ("ms_ssim", "ld", "map_score", "map_inverse")] == [1, 1, 1, 2]

    s.severity, s.corruption_number, s.name = 5, 0, ROUND                                  # the corrupted round, as the launcher sets it
    lines, seen = _round(monkeypatch, evaluation, s, spy)
    for line in lines:
        print(line)
    assert seen == {"prepare_conditioning": {"decode_png": False, "corrupt": (0, 5, 5)},
                    "sample_batch": {"keyed_noise": True, "keep_hypotheses": True}}
    assert lines == ["corruption 0 (gaussian_noise) severity 5"] + MAP_DEV + PER_DOCUMENT + MEANS[:2] + [
        "mean map_dev 1.000000 over 2 of 2 documents"] + MEANS[2:]
    run = f"vis_hp/synthetic/{ROUND}"
    assert spy.calls == ["map_deviation 2"] + [c.format(run=run) for c in OPS_CALLS]
    assert _files(run) == sorted(PRED_FLOW + list(SHEETS) + ["map_dev.txt"])
    for name, text in dict(SHEETS, **{"map_dev.txt": "dir/a_1 copy.jpg 0.500000\nsynthetic_00001 1.500000\n"}).items():
        assert open(f"{run}/{name}").read() == text, name
    assert s.map_dev == [(PATHS[0], 0.5), (PATHS[1], 1.5)] and set(s.map_ref) == set(PATHS)    # a round's scores are its own
    assert [len(getattr(s, k)) for k in ("ms_ssim", "ld", "map_score", "map_inverse")] == [1, 1, 1, 2]
    assert _files("vis_hp/synthetic/pytest_round") == sorted(PRED_FLOW + list(SHEETS) + [f"c00_gaussian_noise_s5/{f}" for f in _files(run)])


# ---- the table of score kinds ---------------------------------------------------------------------------------------------------
def test_every_table_column_is_a_key_its_sheet_can_hold():
    from dvd_amd import evaluation, ops
    from dvd_amd.run_options import GT_METRICS, ROUND_TABLE, SCORE, SCORES
    assert [k.name for k in SCORES] == ["ms_ssim", "ld", "ad", "map_dev", "map_score", "map_inverse"] == list(SCORE)
    assert [k.switch for k in SCORES] == [None, None, None, "keyed_noise", "gt_map_dir", "inverse_outputs"]
    assert {k.switch for k in SCORES} - {None} <= {s.name for s in ROUND_TABLE}
    assert ops.GT_METRIC_NAMES == ("ms_ssim", "ld", "ad") == GT_METRICS + ("ad",)
    for kind in SCORES:
        assert kind.table_columns and kind.mean_keys
        if kind.columns:                                             # a dict per document: every key named is a column of the sheet
            for keys in (kind.table_columns, kind.mean_keys, kind.logged, kind.integers):
                assert set(keys) <= set(kind.columns) and len(set(keys)) == len(keys), (kind.name, keys)
        else:                                                        # a float per document, under the kind's own name
            assert kind.table_columns == kind.mean_keys == (kind.name,) and not kind.integers and not kind.logged
        assert set(kind.means([("a", {c: 1 for c in kind.columns} if kind.columns else 1.0)], kind.table_columns)) == set(kind.table_columns)
    assert SCORE["map_score"].table_columns == ("epe", "pck5", "ause_epe") and SCORE["map_inverse"].table_columns == ("fold", "cycle")
    assert evaluation.MAP_SCORE_COLUMNS is SCORE["map_score"].columns and evaluation.MAP_SCORE_LOGGED is SCORE["map_score"].logged
    assert evaluation.MAP_INVERSE_COLUMNS is SCORE["map_inverse"].columns and evaluation.MAP_INVERSE_LOGGED is SCORE["map_inverse"].logged
    assert evaluation.MAP_SCORE_LOGGED == ("epe", "pck1", "pck5", "fl", "ause_epe")
    assert evaluation.MAP_INVERSE_LOGGED == ("covered", "fold_px", "flipped", "skipped", "cycle_mean", "cycle_max")


def test_means_of_floats_and_of_dicts():
    from dvd_amd.run_options import SCORE
    nan = float("nan")
    assert SCORE["ld"].means([]) == {} and SCORE["ld"].means([("a", 1.0), ("b", 2.5)]) == {"ld": 1.75}
    scores = [("a", {"epe": 1.0, "pck5": 0.5}), ("b", {"epe": 2.0, "pck5": nan}), ("c", {"epe": nan})]
    assert SCORE["map_score"].means(scores, ("epe", "pck5", "fl")) == {"epe": 1.5, "pck5": 0.5}
    assert set(SCORE["map_score"].means(scores)) == {"epe", "pck5"} and SCORE["map_score"].values(scores, "epe") == [1.0, 2.0]
    assert SCORE["map_score"].cell(scores[0][1], "fl") == "-" and SCORE["map_score"].cell({"n_valid": 7}, "n_valid") == "7"
    assert SCORE["map_dev"].cell(0.5, "map_dev") == "0.500000"


FLAGS = {"keyed_noise": True, "flow_outputs": "npy", "gt_map_dir": "maps", "inverse_outputs": "mesh"}
TABLE_COLUMNS = {"keyed_noise": ["map_dev"], "flow_outputs": [], "gt_map_dir": ["epe", "pck5", "ause_epe"], "inverse_outputs": ["fold", "cycle"]}
TABLE_VALUES = {"keyed_noise": ["1.750000"], "flow_outputs": [], "gt_map_dir": ["1.500000", "0.750000", "0.250000"],
                "inverse_outputs": ["0.250000", "0.125000"]}


def _fake_launch(monkeypatch, R):
    def run(settings):
        settings.ms_ssim, settings.ld = [("a", 0.5), ("b", 0.75)], [("a", 2.0)]
        if settings.corruption_number == 1:                                # a round in which nothing else is scored
            return
        if getattr(settings, "keyed_noise", False) and settings.severity:
            settings.map_dev = [("a", 1.5), ("b", 2.0)]
        if getattr(settings, "gt_map_dir", None):
            settings.map_score = [("a", {"epe": 1.0, "pck5": 0.5, "ause_epe": 0.25}), ("b", {"epe": 2.0, "pck5": 1.0})]
        if getattr(settings, "inverse_outputs", None):
            settings.map_inverse = [("a", {"fold": 0.0, "cycle": 0.125}), ("b", {"fold": 0.5, "cycle": float("nan")})]
    monkeypatch.setattr(R, "importlib", types.SimpleNamespace(import_module=lambda name: types.SimpleNamespace(run=run)))
    monkeypatch.setattr(R, "shutil", types.SimpleNamespace(copyfile=lambda *a: None))


@pytest.mark.parametrize("given", [c for n in range(5) for c in itertools.combinations(FLAGS, n)], ids=lambda c: "+".join(c) or "none")
def test_the_launchers_header_is_the_enabled_kinds_columns(tmp_path, monkeypatch, given):
    import run_sampling as R
    from dvd_amd.run_options import SCORES
    monkeypatch.chdir(tmp_path)
    _fake_launch(monkeypatch, R)
    R.run_sampling("dvd", "val_TDiff", 3, "exp", corruption=True, **{k: FLAGS[k] for k in given})
    table = (tmp_path / "vis_hp" / "synthetic" / "exp" / "corruption_table.txt").read_text().splitlines()
    by_table = [c for kind in SCORES if kind.switch in given for c in kind.table_columns]
    assert by_table == [c for k in FLAGS if k in given for c in TABLE_COLUMNS[k]]
    assert table[0].split() == ["no", "kind", "severity", "ms_ssim", "ld"] + by_table                     # 'ad': no row has it
    assert table[1].split() == ["0", "gaussian_noise", "5", "0.625000", "2.000000"] + [v for k in FLAGS if k in given for v in TABLE_VALUES[k]]
    assert table[2].split() == ["1", "shot_noise", "5", "0.625000", "2.000000"] + ["-"] * len(by_table)   # a missing value: a dash
