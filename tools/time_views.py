#!/usr/bin/env python
"""clips/s of the GPU view construction (facl_amd.views.build_views: host draws in the reference's NumPy order +
one HIP launch per batch) next to the NumPy restatement of the dataset class's per-sample pipeline (oracle/views.py =
cn3D_data_set.py:285-350, what the reference runs in its 16 DataLoader workers) on the host cores.  Prints one JSON line.

With --baseline_lib (a libfacl_hip.so built from the parent commit) it compares the NumPy-mode kernel of two builds instead, as
tools/time_views_sizes.py does: every run is a fresh process (FACL_LIB picks the library), the two libraries alternate, and per
library the --rounds values of build_views_clips_per_s, their median and their spread (max - min) are reported.  This build's
median may fall below the baseline's by no more than the baseline's own spread.  The figure INCLUDES the host draws and the
copies, which are most of it.  A child that fails ends the measurement at once.  --out: also write the line to that file (into
its "numpy_mode" key when the file already holds a JSON object).

    python tools/time_views.py [--B 32] [--iters 20] [--baseline_lib PATH [--rounds 5] [--out profiles/views_fold.json]]
"""
import argparse
import json
import os
import re
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(vals):
    return {"values": vals, "median": float(np.median(vals)), "spread": float(max(vals) - min(vals))}


def compare(a):
    """This build against a.baseline_lib: alternating fresh processes, medians and spread per library; one JSON line."""
    from facl_amd import _lib
    libs = {"baseline": os.path.abspath(a.baseline_lib), "this": _lib.lib_path()}
    runs, dev_runs = {k: [] for k in libs}, {k: [] for k in libs}
    for i in range(a.rounds):
        for k in sorted(libs):                                      # baseline, this, baseline, this, ...
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--B", str(a.B), "--iters", str(a.iters), "--oracle", "0"],
                               stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=a.child_timeout, text=True,
                               env=dict(os.environ, FACL_LIB=libs[k]))
            res = re.search(r"^(\{.*\})$", r.stdout, flags=re.M)
            if r.returncode != 0 or res is None:
                raise SystemExit("%s round %d failed (exit %d); nothing more is started:\n%s" % (k, i, r.returncode, r.stdout[-4000:]))
            got = json.loads(res.group(1))
            runs[k].append(got["build_views_clips_per_s"])
            dev_runs[k].append(got["build_views_device_rng_clips_per_s"])
            print("%s round %d: %.1f clips/s (device draws: %.1f)" % (k, i, runs[k][-1], dev_runs[k][-1]), file=sys.stderr, flush=True)
    out = {"what": "facl_build_views_f32 through build_views: clips/s INCLUDING the host draws and the copies", "B": a.B,
           "iters_per_run": a.iters, "rounds": a.rounds, "process_per_run": True,
           "clips_per_s": {k: spread(v) for k, v in runs.items()},
           "device_draws_clips_per_s": {k: spread(v) for k, v in dev_runs.items()}}        # no host draws: nearer the kernel
    c = out["clips_per_s"]
    out["no_regression"] = {"baseline_minus_this_clips_per_s": c["baseline"]["median"] - c["this"]["median"],
                            "baseline_spread_clips_per_s": c["baseline"]["spread"],
                            "holds": c["baseline"]["median"] - c["this"]["median"] <= c["baseline"]["spread"]}
    print(json.dumps(out))
    if a.out:
        whole = out
        if os.path.exists(a.out):
            with open(a.out) as f:
                whole = dict(json.load(f), numpy_mode=out)
        with open(a.out, "w") as f:
            f.write(json.dumps(whole) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--oracle", type=int, default=1, help="0 = skip the NumPy restatement on the host cores")
    ap.add_argument("--baseline_lib", type=str, default="", help="libfacl_hip.so of the parent commit")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--child_timeout", type=int, default=300)
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()
    if a.baseline_lib:
        return compare(a)
    from facl_amd.views import build_views, synthetic_raw_clip
    from oracle import views as OV
    clips = [synthetic_raw_clip(b, np.float32, P=4000, Kp=1500, R1=2000, R2=1000) for b in range(a.B)]
    rng = np.random.RandomState(0)
    for _ in range(3):
        build_views(clips, rng)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.iters):
        out = build_views(clips, rng)
    torch.cuda.synchronize()
    t_gpu = (time.perf_counter() - t0) / a.iters
    gen = torch.Generator(device="cuda")
    gen.manual_seed(0)
    for _ in range(3):
        build_views(clips, device_rng=gen)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.iters):
        out = build_views(clips, device_rng=gen)
    torch.cuda.synchronize()
    t_dev = (time.perf_counter() - t0) / a.iters
    res = {"what": "view construction, 10 views x 512 points x 4 channels per clip (SURVEY 8 f-3)", "B": a.B,
           "build_views_ms_per_batch": round(1e3 * t_gpu, 3), "build_views_clips_per_s": round(a.B / t_gpu, 1),
           "build_views_device_rng_ms_per_batch": round(1e3 * t_dev, 3), "build_views_device_rng_clips_per_s": round(a.B / t_dev, 1)}
    if a.oracle:
        t0 = time.perf_counter()
        for _ in range(3):
            want = OV.collate_view_major([OV.get_item(rng, *c) for c in clips])
        t_cpu = (time.perf_counter() - t0) / 3
        res.update({"oracle_numpy_ms_per_batch_1_core": round(1e3 * t_cpu, 3), "oracle_numpy_clips_per_s_1_core": round(a.B / t_cpu, 1)})
    print(json.dumps({**res, "host_cores": len(os.sched_getaffinity(0)),
                      "note": "build_views = host draws (reference NumPy order, one core) + H2D of sources / indices / noise + one "
                              "HIP launch; the reference spreads the NumPy pipeline over 16 DataLoader workers"}))


if __name__ == "__main__":
    main()
