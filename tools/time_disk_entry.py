#!/usr/bin/env python
"""Clips/s of the training entry on a dataset ON DISK (--synthetic 0) next to the synthetic iid input (--synthetic 1).

Builds a seeded dataset of --clips clips of (2048, 8) float64 clouds (the layout generate_NTU.py writes) in the
reference's folder layout under a temporary folder, then runs the motion training entry at --B per mode, alternating
the modes for --rounds rounds in one process.  Every run trains --epochs epochs of --steps steps; epoch 0 is the warm-up
(graph capture), the clips/s of the last epoch is reported.  Prints one JSON line (and writes it to --out).

    python tools/time_disk_entry.py [--B 32] [--clips 512] [--steps 12] [--rounds 2] [--out profiles/disk_entry.json]
"""
import argparse
import contextlib
import io
import json
import os
import re
import shutil
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODES = {"synthetic1": ["--synthetic", "1"],
         "disk_numpy": ["--synthetic", "0", "--view_rng", "numpy"],
         "disk_philox": ["--synthetic", "0", "--view_rng", "philox"]}


def make_dataset(root, n, P=2048):
    from facl_amd.dataset import clip_paths
    r = np.random.RandomState(0)
    for i in range(n):
        name = "S%03dC%03dP%03dR%03dA%03d" % (1 + i % 32, 2 + i % 2, 1 + (i // 32) % 106, 1 + i % 2, 1 + i % 60)
        pts = r.rand(P, 8) - 0.5
        pts[r.rand(P) < 0.5, 4] = 0
        pts[r.rand(P) < 0.5, 7] = 0
        arrs = (pts, r.rand(P, 8) - 0.5, r.rand(P, 8) - 0.5, r.rand(P, 8) - 0.5)
        for p, a in zip(clip_paths(root, name, "0"), arrs):
            os.makedirs(os.path.dirname(p), exist_ok=True)
            np.save(p, a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--clips", type=int, default=512)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--epochs", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--modes", type=str, default=",".join(MODES))
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()
    from facl_amd import cn3d_train_motion_GL as train
    tmp = tempfile.mkdtemp(prefix="facl_disk_")
    try:
        make_dataset(tmp, a.clips)
        res = {m: [] for m in a.modes.split(",")}
        for _ in range(a.rounds):
            for m in res:
                args = MODES[m] + ["--data_root", tmp, "--dataset", "ntu120", "--batchSize", str(a.B), "--nepoch",
                                   str(a.epochs), "--num_crop", "10", "--SAMPLE_NUM", "512", "--INPUT_FEATURE_NUM", "4",
                                   "--steps_per_epoch", str(a.steps), "--max_steps_per_epoch", str(a.steps),
                                   "--save_root_dir", os.path.join(tmp, "ck")]
                buf = io.StringIO()
                with contextlib.redirect_stdout(buf):
                    train.main(args)
                rates = [float(x) for x in re.findall(r"clips/s: ([0-9.]+)", buf.getvalue())]
                res[m].append(rates[-1])
        out = {"B": a.B, "clips": a.clips, "steps_timed": a.steps, "rounds": a.rounds,
               "clips_per_s": {m: v for m, v in res.items()},
               "median_clips_per_s": {m: float(np.median(v)) for m, v in res.items()}}
        if "synthetic1" in res:
            out["ratio_to_synthetic1"] = {m: out["median_clips_per_s"][m] / out["median_clips_per_s"]["synthetic1"]
                                          for m in res}
        line = json.dumps(out)
        print(line)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(line + "\n")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
