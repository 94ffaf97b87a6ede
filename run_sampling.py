#!/usr/bin/env python3
"""Launcher with the reference's command line (reference run_sampling.py:66-87):

    python run_sampling.py --train_module dvd --train_name val_TDiff --name <run>

dispatches to train_settings/<module>/<name>.run(settings).

--corruption runs the reference's fifteen rounds (severity 5, corruption numbers 0..14 of the common-corruptions benchmark); here
each round corrupts the network input on the device, writes under <name>/cNN_<kind>_s<severity> and the run
ends with one table: kind -> mean of every metric of env.gt_dir.  --severity N and --corruption_number K choose one round.

--keyed_noise keys the sampler's noise per document (settings.keyed_noise).  With corrupted rounds it runs the
clean round first, under <name>, and the table gains the column map_dev: the mean distance, in pixels of the network input,
between the map predicted from the corrupted input and the one predicted from the clean input - a number that needs no scan.

--flow_outputs png,flo,npy writes the predicted map of every document under <name>/pred_flow (settings.flow_outputs; DESIGN.md
4.12): its colour-wheel picture, its full-resolution .flo field and / or the coarse map itself.  Every round writes its own.

--gt_map_dir DIR scores every document's predicted map against the ground-truth map DIR holds for it (settings.gt_map_dir;
DESIGN.md 4.13: <stem>.flo, flow_<stem>.flo, <stem>.npy or flow_<stem>.npy - the files --flow_outputs flo,npy writes): EPE, PCK,
Fl and the sparsification error AUSE, in map_score.txt; under --corruption the table gains the columns epe, pck5, ause_epe.

--inverse_outputs mesh,flo,mask inverts every document's predicted map on the device (settings.inverse_outputs)
and writes under <name>/pred_flow the predicted page mesh drawn on the photograph, the forward displacement field and / or the
coverage mask; map_inverse.txt holds the coverage, the fold count and the cycle error, which need neither a scan nor a
ground-truth map; under --corruption the table gains the columns fold and cycle."""
import argparse
import importlib
import os
import random
import shutil
from datetime import date

import numpy as np
import torch

import admin.settings as ws_settings


def corruption_rounds(corruption=False, severity=None, corruption_number=None, *, baseline=False):
    """[(severity, number)] of the rounds to run: the reference's fifteen under --corruption, one chosen round when --severity
    or --corruption_number is given (5 and 0 where only the other one is), else the one clean round.  baseline: the clean round
    (0, 0) comes first wherever a round corrupts."""
    if severity is None and corruption_number is None:
        rounds = [(5, c) for c in range(15)] if corruption else [(0, 0)]
    else:
        rounds = [(5 if severity is None else severity, 0 if corruption_number is None else corruption_number)]
    return [(0, 0)] + rounds if baseline and any(sev != 0 for sev, _ in rounds) else rounds


def round_name(name, severity, number):
    """The run name of one corrupted round: its pictures and score files get a directory of their own."""
    from dvd_amd import ops
    return f"{name}/c{number:02d}_{ops.CORRUPTIONS[number]}_s{severity}"


def write_corruption_table(path, rows, metrics):
    """rows [(number, kind, severity, {metric: mean})] -> the table as text, printed and written to `path`."""
    lines = ["no kind severity " + " ".join(metrics)]
    for number, kind, severity, means in rows:
        lines.append(f"{number} {kind} {severity} " + " ".join(f"{means[m]:.6f}" if m in means else "-" for m in metrics))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write(text)
    return text


def run_sampling(train_module, train_name, seed, name, cudnn_benchmark=True, corruption=False, severity=None,
                 corruption_number=None, *, keyed_noise=False, flow_outputs="", gt_map_dir="", inverse_outputs=""):
    from dvd_amd import ops
    from dvd_amd.evaluation import run_dir
    from dvd_amd.run_options import ROUND_TABLE, SCORES
    print(f"Sampling:  {train_module}  {train_name}\nDate: {date.today().strftime('%d/%m/%Y')}")
    settings = ws_settings.Settings()
    settings.module_name, settings.script_name = train_module, train_name
    settings.project_path = f"train_settings/{train_module}/{train_name}"
    settings.seed, settings.name = seed, name
    flags = {"keyed_noise": keyed_noise, "flow_outputs": flow_outputs, "gt_map_dir": gt_map_dir, "inverse_outputs": inverse_outputs}
    for switch in ROUND_TABLE:                                # absent without the flag: the run is what it always was
        if flags[switch.name]:
            setattr(settings, switch.name, flags[switch.name])
    scores = [score for score in SCORES if score.switch is None or flags[score.switch]]   # the env.gt_dir metrics, and what the flags add
    save_dir = os.path.join(settings.env.workspace_dir, settings.project_path)
    os.makedirs(save_dir, exist_ok=True)
    shutil.copyfile(settings.project_path + ".py", os.path.join(save_dir, settings.script_name + ".py"))
    module = importlib.import_module(f"train_settings.{train_module.replace('/', '.')}.{train_name.replace('/', '.')}")
    run = getattr(module, "run")
    rows = []
    rounds = corruption_rounds(corruption, severity, corruption_number, baseline=bool(keyed_noise))
    if keyed_noise:                                           # a bad round is refused before the clean round runs for it
        for sev, number in rounds:
            if ops.corruption_severity(sev, "--severity"):
                ops.corruption_number(number, "--corruption_number")
    for sev, number in rounds:
        sev = ops.corruption_severity(sev, "--severity")
        if sev == 0:                                          # the clean round, as ever
            settings.severity, settings.corruption_number, settings.name = sev, number, name
            run(settings)
            continue
        number = ops.corruption_number(number, "--corruption_number")
        kind = ops.CORRUPTIONS[number]
        if not ops.corruption_supported(number):
            print(f"corruption {number} ({kind}): no device kernel, round skipped")
            continue
        settings.severity, settings.corruption_number, settings.name = sev, number, round_name(name, sev, number)
        for score in SCORES:                                  # a round's scores are its own
            if hasattr(settings, score.name):
                delattr(settings, score.name)
        run(settings)
        means = {}
        for score in scores:
            means.update(score.means(getattr(settings, score.name, None) or [], score.table_columns))
        rows.append((number, kind, sev, means))
    settings.name = name
    if rows:
        # the ground-truth metrics that some row has, then every column of the kinds the flags enable, valued or not
        metrics = [c for score in scores for c in score.table_columns if score.switch or any(c in means for *_, means in rows)]
        write_corruption_table(os.path.join(run_dir(settings), "corruption_table.txt"), rows, metrics)


def main():
    p = argparse.ArgumentParser(description="Run a sampling script in train_settings.")
    p.add_argument("--train_module", type=str, required=True)
    p.add_argument("--train_name", type=str, required=True)
    p.add_argument("--cudnn_benchmark", type=bool, default=True)
    p.add_argument("--seed", type=int, default=1992)
    p.add_argument("--name", type=str, default="Default")
    p.add_argument("--corruption", action="store_true")
    p.add_argument("--severity", type=int, default=None, help="one chosen round: its severity 0..5 (5 if only --corruption_number is given)")
    p.add_argument("--corruption_number", type=int, default=None, help="one chosen round: its corruption 0..18 (0 if only --severity is given)")
    p.add_argument("--keyed_noise", action="store_true", help="key the sampler's noise per document; with corrupted rounds: the clean "
                   "round first, then the column map_dev in the table")
    p.add_argument("--flow_outputs", type=str, default="", help="comma-separated list of png, flo, npy: what to write of every "
                   "document's predicted map under pred_flow/ (nothing by default)")
    p.add_argument("--gt_map_dir", type=str, default="", help="directory of ground-truth maps (<stem>.flo, flow_<stem>.flo, <stem>.npy, "
                   "flow_<stem>.npy): score every document's predicted map against its own (EPE, PCK, Fl, AUSE)")
    p.add_argument("--inverse_outputs", type=str, default="", help="comma-separated list of mesh, flo, mask: invert every document's "
                   "predicted map and write the page mesh on the photograph, the forward field and / or the coverage mask under pred_flow/")
    a = p.parse_args()
    a.seed = torch.initial_seed() & (2 ** 32 - 1)      # as the reference: the CLI value is overwritten (:77-78)
    print(f"Seed is {a.seed}")
    random.seed(int(a.seed))
    np.random.seed(a.seed)
    run_sampling(a.train_module, a.train_name, seed=a.seed, name=a.name, cudnn_benchmark=a.cudnn_benchmark,
                 corruption=a.corruption, severity=a.severity, corruption_number=a.corruption_number, keyed_noise=a.keyed_noise,
                 flow_outputs=a.flow_outputs, gt_map_dir=a.gt_map_dir, inverse_outputs=a.inverse_outputs)


if __name__ == "__main__":
    main()
