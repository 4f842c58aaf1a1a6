#!/usr/bin/env python
"""Clips/s of the training entry with the split RESIDENT in device memory (--resident 1) next to batches from disk
(--resident 0, --view_rng philox) and the synthetic iid input (--synthetic 1).

Same dataset as tools/time_disk_entry.py: --clips clips of four (2048, 8) float64 clouds in the reference's folder layout
under a temporary folder, the motion training entry at --B.  Every (round, mode) runs in a FRESH process, the modes
alternating within a round, so that no mode inherits another's allocator, graph or page-cache warm-up by position alone.
A run trains --epochs epochs of --steps steps; epoch 0 is the warm-up (graph capture), the clips/s of the last epoch is
reported.  The ingest of the resident mode is reported on its own (seconds, GB, GB/s) and is not part of clips/s.  Also
recorded per mode: torch.cuda.max_memory_allocated() of the run (the step's peak feeds facl_amd.resident.STEP_PEAK_BYTES).
A child that fails ends the measurement at once.  Prints one JSON line (and writes it to --out).

    python tools/time_resident_entry.py [--B 32] [--clips 512] [--steps 12] [--rounds 3] [--out profiles/resident_entry.json]
    python tools/time_resident_entry.py --worker resident --data DIR      # one run (e.g. under a kernel trace)
"""
import argparse
import contextlib
import io
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODES = {"synthetic1": ["--synthetic", "1"],
         "disk_philox": ["--synthetic", "0", "--view_rng", "philox"],
         "resident": ["--synthetic", "0", "--view_rng", "philox", "--resident", "1"]}


def worker(a):
    """One training run of mode a.worker on the dataset at a.data; prints one JSON line."""
    import torch
    from facl_amd import cn3d_train_motion_GL as train
    args = MODES[a.worker] + ["--data_root", a.data, "--dataset", "ntu120", "--batchSize", str(a.B), "--nepoch",
                              str(a.epochs), "--num_crop", "10", "--SAMPLE_NUM", "512", "--INPUT_FEATURE_NUM", "4",
                              "--steps_per_epoch", str(a.steps), "--max_steps_per_epoch", str(a.steps),
                              "--save_root_dir", os.path.join(a.data, "ck")]
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        train.main(args)
    text = buf.getvalue()
    out = {"mode": a.worker, "clips_per_s": [float(x) for x in re.findall(r"clips/s: ([0-9.]+)", text)],
           "max_memory_allocated": int(torch.cuda.max_memory_allocated())}
    m = re.search(r"resident: (\d+) clips, ([0-9.]+) GB, ([0-9.]+) s", text)
    if m:
        out["ingest"] = {"clips": int(m.group(1)), "GB": float(m.group(2)), "s": float(m.group(3))}
    print("RESULT " + json.dumps(out))


def spread(v):
    return float(max(v) - min(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--clips", type=int, default=512)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--modes", type=str, default=",".join(MODES))
    ap.add_argument("--out", type=str, default="")
    ap.add_argument("--data", type=str, default="", help="dataset folder: built there if missing, and kept")
    ap.add_argument("--worker", type=str, default="", choices=[""] + list(MODES))
    ap.add_argument("--child_timeout", type=int, default=240)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    from tools.time_disk_entry import make_dataset
    tmp = a.data or tempfile.mkdtemp(prefix="facl_resident_")
    try:
        if not os.path.isdir(os.path.join(tmp, "reslution")):
            make_dataset(tmp, a.clips)
        modes = a.modes.split(",")
        runs = {m: [] for m in modes}
        for _ in range(a.rounds):
            for m in modes:
                cmd = [sys.executable, os.path.abspath(__file__), "--worker", m, "--data", tmp, "--B", str(a.B), "--steps",
                       str(a.steps), "--epochs", str(a.epochs)]
                r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=a.child_timeout, text=True)
                res = re.search(r"^RESULT (.*)$", r.stdout, flags=re.M)
                if r.returncode != 0 or res is None:
                    raise SystemExit("mode %s failed (exit %d); nothing more is started:\n%s" % (m, r.returncode, r.stdout[-4000:]))
                runs[m].append(json.loads(res.group(1)))
                print("%s: %.1f clips/s" % (m, runs[m][-1]["clips_per_s"][-1]), file=sys.stderr, flush=True)
        rate = {m: [x["clips_per_s"][-1] for x in v] for m, v in runs.items()}
        med = {m: float(np.median(v)) for m, v in rate.items()}
        out = {"B": a.B, "clips": a.clips, "steps_timed": a.steps, "epochs": a.epochs, "rounds": a.rounds,
               "process_per_run": True, "clips_per_s": rate, "median_clips_per_s": med,
               "spread_clips_per_s": {m: spread(v) for m, v in rate.items()},
               "max_memory_allocated": {m: [x["max_memory_allocated"] for x in v] for m, v in runs.items()}}
        if "synthetic1" in med:
            out["ratio_to_synthetic1"] = {m: med[m] / med["synthetic1"] for m in med}
        if "resident" in runs:
            ing = [x["ingest"] for x in runs["resident"]]
            out["ingest"] = {"clips": ing[0]["clips"], "GB": ing[0]["GB"], "s": [x["s"] for x in ing],
                             "GB_per_s": [x["GB"] / x["s"] if x["s"] else None for x in ing]}
            if "disk_philox" in med:
                gap = med["resident"] - med["disk_philox"]
                out["resident_minus_disk_philox"] = gap
                out["spreads_combined"] = out["spread_clips_per_s"]["resident"] + out["spread_clips_per_s"]["disk_philox"]
                # seconds saved per epoch of this dataset against batches from disk, and the epochs that repay the ingest
                per_epoch = a.clips / med["disk_philox"] - a.clips / med["resident"]
                out["break_even_epochs"] = float(np.median(out["ingest"]["s"])) / per_epoch if per_epoch > 0 else None
        line = json.dumps(out)
        print(line)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(line + "\n")
    finally:
        if not a.data:
            shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
