#!/usr/bin/env python
"""Seconds and clips/s of the prediction entry (facl_amd.predict --draws 1) next to motion-feature extraction
(facl_amd.extract_motion_feature) on the same clips: the same loader and encoder, prediction adds the head and the two
kernels of csrc/predict.hip per batch.

Same dataset as tools/time_resident_entry.py: --clips clips of four (2048, 8) float64 clouds in the reference's folder
layout under a temporary folder, listed under <root>/raw as the extraction entries expect.  Its cameras are 2 and 3, so the
cross-view train split is all of it: prediction runs with --subset all, extraction over its train and (empty) test split,
--clips clips each.  The encoder and the 60-class head are freshly initialised (timing does not depend on the weights).
Every (round, entry) runs in a FRESH process, the two entries alternating within a round; a run is timed around the
entry's main(), checkpoint loading and the first launches included, no file written.  A child that fails ends the
measurement at once.  Prints one JSON line (and writes it to --out): the expectation is that prediction is no slower than
extraction by more than extraction's own spread (max - min) over its rounds.

    python tools/time_predict.py [--B 32] [--clips 512] [--rounds 3] [--out profiles/predict.json]
    python tools/time_predict.py --worker predict --data DIR      # one run (e.g. under a kernel trace)
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
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ENTRIES = ("predict", "extract")
VIEWS = ["--num_crop", "10", "--SAMPLE_NUM", "512", "--INPUT_FEATURE_NUM", "4"]


def make_checkpoints(root):
    """A freshly initialised encoder and 60-class head under <root>/ck (host only)."""
    import torch
    from facl_amd import predict
    from facl_amd.cls_head import ClipClassifier
    from facl_amd.cn3d_model_conbag import PointNet_Plus
    os.makedirs(os.path.join(root, "ck"), exist_ok=True)
    torch.manual_seed(1)
    opt = predict.predict_parser().parse_args(VIEWS)
    torch.save(PointNet_Plus(opt, gost=10).state_dict(), os.path.join(root, "ck", "enc.pth"))
    torch.save(ClipClassifier(10, 60).state_dict(), os.path.join(root, "ck", "fc.pth"))


def list_clips(root):
    """<root>/raw/<name>.npy for every clip of the tree: the folder the extraction entries list."""
    os.makedirs(os.path.join(root, "raw"), exist_ok=True)
    for n in os.listdir(os.path.join(root, "reslution", "Resolution60", "raw")):
        np.save(os.path.join(root, "raw", n), np.zeros((1, 8)))


def worker(a):
    """One run of entry a.worker on the dataset at a.data; prints one JSON line."""
    import torch
    common = ["--data_root", a.data, "--dataset", "ntu120", "--batchSize", str(a.B), "--view_rng", a.view_rng] + VIEWS
    enc, fc = os.path.join(a.data, "ck", "enc.pth"), os.path.join(a.data, "ck", "fc.pth")
    buf = io.StringIO()
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(buf):
        if a.worker == "predict":
            from facl_amd import predict
            res = predict.main(common + ["--encoder", enc, "--head", fc, "--subset", "all", "--draws", "1", "--topk", "5"])
            clips = res["clips"]
        else:
            from facl_amd import extract_motion_feature
            clips = extract_motion_feature.main(common + ["--synthetic", "0", "--checkpoint", enc]).shape[0]
    torch.cuda.synchronize()
    s = time.perf_counter() - t0
    print("RESULT " + json.dumps({"entry": a.worker, "clips": int(clips), "s": s, "clips_per_s": clips / s,
                                  "max_memory_allocated": int(torch.cuda.max_memory_allocated())}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--clips", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--view_rng", type=str, default="philox", choices=("numpy", "philox"))
    ap.add_argument("--out", type=str, default="")
    ap.add_argument("--data", type=str, default="", help="dataset folder: built there if missing, and kept")
    ap.add_argument("--worker", type=str, default="", choices=("",) + ENTRIES)
    ap.add_argument("--child_timeout", type=int, default=240)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    from tools.time_disk_entry import make_dataset
    tmp = a.data or tempfile.mkdtemp(prefix="facl_predict_")
    try:
        if not os.path.isdir(os.path.join(tmp, "reslution")):
            make_dataset(tmp, a.clips)
        list_clips(tmp)
        make_checkpoints(tmp)
        runs = {e: [] for e in ENTRIES}
        for _ in range(a.rounds):
            for e in ENTRIES:
                cmd = [sys.executable, os.path.abspath(__file__), "--worker", e, "--data", tmp, "--B", str(a.B), "--view_rng", a.view_rng]
                r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=a.child_timeout, text=True)
                res = re.search(r"^RESULT (.*)$", r.stdout, flags=re.M)
                if r.returncode != 0 or res is None:
                    raise SystemExit("entry %s failed (exit %d); nothing more is started:\n%s" % (e, r.returncode, r.stdout[-4000:]))
                runs[e].append(json.loads(res.group(1)))
                print("%s: %.2f s, %.1f clips/s" % (e, runs[e][-1]["s"], runs[e][-1]["clips_per_s"]), file=sys.stderr, flush=True)
        secs = {e: [x["s"] for x in v] for e, v in runs.items()}
        med = {e: float(np.median(v)) for e, v in secs.items()}
        spread = {e: float(max(v) - min(v)) for e, v in secs.items()}
        out = {"B": a.B, "clips": {e: runs[e][0]["clips"] for e in ENTRIES}, "rounds": a.rounds, "view_rng": a.view_rng,
               "process_per_run": True, "seconds": secs, "median_seconds": med, "spread_seconds": spread,
               "clips_per_s": {e: [x["clips_per_s"] for x in v] for e, v in runs.items()},
               "max_memory_allocated": {e: [x["max_memory_allocated"] for x in v] for e, v in runs.items()},
               "predict_minus_extract_seconds": med["predict"] - med["extract"],
               "no_slower_within_extract_spread": bool(med["predict"] - med["extract"] <= spread["extract"])}
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
