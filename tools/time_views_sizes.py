#!/usr/bin/env python
"""The philox views at any view count G and cloud size P (csrc/views_philox.hip, csrc/views_resident.hip), measured.

1. No regression at the old size: device time per launch of the EXISTING entries facl_build_views_philox_f64 and
   facl_build_views_resident_f64 at --B, on this build and -- with --baseline_lib, a libfacl_hip.so built from the parent
   commit -- on that one.  Every run is a fresh process; the two libraries alternate; each run reports the median of
   --reps windows of --launches launches between two device events.  Reported per library: the --rounds medians, their
   median and their spread (max - min).  The new median may exceed the baseline's by no more than the baseline's own spread.
2. New sizes: us per launch and points/s of the _gp entries at (10,512), (10,2048), (24,512), (24,2048), disk and resident,
   and the kernel's share of the step of the training entry at that size (--synthetic 1 --graph 1: B / clips per second).
3. End to end: clips/s of the training entry at --num_crop 24 --SAMPLE_NUM 2048 --resident 1 --graph 1 on a synthetic tree
   (tools/time_disk_entry.make_dataset), from disk (--resident 0), and on the synthetic iid input of the same size.
With --sizes_every_round 1 the _gp sizes are timed in EVERY round and library (medians and spread per library), and, where
   the library has the recipe entries, a non-default view recipe (scale,tilt_neg,tilt_pos,jitter,rot,mirror,t7) next to them,
   per library as well; with a baseline, rule 1 is then applied to every cell at 10 x 512 and 24 x 2048 (no_regression_sizes).
A child that fails ends the measurement at once.  Prints one JSON line (and writes it to --out).

    python tools/time_views_sizes.py [--baseline_lib PATH] [--out profiles/views_sizes.json]
"""
import argparse
import contextlib
import ctypes
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
SIZES = [(10, 512), (10, 2048), (24, 512), (24, 2048)]
ENTRY = {"synthetic1": ["--synthetic", "1"],
         "disk_philox": ["--synthetic", "0", "--view_rng", "philox"],
         "resident": ["--synthetic", "0", "--view_rng", "philox", "--resident", "1"]}


def kernel_worker(a):
    """Times the view entries of the library at a.lib on B clips of four (2048, 8) float64 clouds; one JSON line."""
    import torch
    from facl_amd.resident import build_table
    lib = ctypes.CDLL(a.lib)                               # bound by hand: a baseline library lacks the _gp entries
    P_, I_, L_ = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    sig = {"facl_views_temporal_rows_f64": [P_, L_, I_, P_, I_, P_, P_, P_, P_],
           "facl_build_views_philox_f64": [P_, L_, I_, P_, P_, P_, L_, I_, I_, P_, P_, P_],
           "facl_resident_temporal_rows_f64": [P_, P_, P_, I_, I_, P_, P_],
           "facl_build_views_resident_f64": [P_, P_, P_, I_, P_, I_, L_, I_, P_, P_, P_, P_],
           "facl_build_views_philox_gp_f64": [P_, L_, I_, P_, P_, P_, L_, I_, I_, I_, I_, P_, P_, P_],
           "facl_build_views_resident_gp_f64": [P_, P_, P_, I_, P_, I_, I_, I_, L_, I_, P_, P_, P_, P_]}
    has_gp = hasattr(lib, "facl_build_views_philox_gp_f64")
    has_recipe = hasattr(lib, "facl_build_views_philox_recipe_f64")       # a baseline library lacks the recipe entries
    if has_recipe:
        sig["facl_build_views_philox_recipe_f64"] = sig["facl_build_views_philox_gp_f64"][:-1] + [P_, I_, P_, P_]
        sig["facl_build_views_resident_recipe_f64"] = sig["facl_build_views_resident_gp_f64"][:-1] + [P_, I_, P_, P_]
    for name, args in sig.items():
        if has_gp or "_gp_" not in name:
            getattr(lib, name).argtypes = args
            getattr(lib, name).restype = I_
    dev, B = torch.device("cuda", 0), a.B
    r = np.random.RandomState(0)
    rows = np.full((B, 4), 2048, dtype=np.int64)
    src = r.rand(int(rows.sum()), 8) - 0.5
    for b in range(B):
        pts = src[b * 4 * 2048:b * 4 * 2048 + 2048]
        pts[r.rand(2048) < 0.5, 4] = 0
        pts[r.rand(2048) < 0.5, 7] = 0
    table, total, total0 = build_table(rows, np.arange(B))
    meta = np.concatenate((table[:, 0:8], table[:, 8:9]), 1).astype(np.int32)
    s = torch.cuda.current_stream().cuda_stream
    src = torch.from_numpy(src).to(dev)
    meta, tab = torch.from_numpy(meta).to(dev), torch.from_numpy(table).to(dev)
    list_d = torch.empty((2, total), dtype=torch.int32, device=dev)
    counts = torch.empty((B, 2), dtype=torch.int32, device=dev)
    err1 = torch.zeros((1,), dtype=torch.int32, device=dev)
    list_r = torch.empty((2 * total0,), dtype=torch.int32, device=dev)
    err2 = torch.tensor([0, 2 ** 31 - 1], dtype=torch.int32, device=dev)
    sel = torch.from_numpy(r.permutation(B).astype(np.int32)).to(dev)

    def ok(rc):
        if rc != 0:
            raise SystemExit("entry returned %d" % rc)
    ok(lib.facl_views_temporal_rows_f64(src.data_ptr(), total, 8, meta.data_ptr(), B, list_d.data_ptr(), counts.data_ptr(),
                                        err1.data_ptr(), s))
    ok(lib.facl_resident_temporal_rows_f64(src.data_ptr(), tab.data_ptr(), list_r.data_ptr(), 0, B, err2.data_ptr(), s))
    out = torch.empty((24 * B * 2048 * 4,), dtype=torch.float32, device=dev)

    def disk(G=None, P=None):
        head = (src.data_ptr(), total, 8, meta.data_ptr(), list_d.data_ptr(), counts.data_ptr(), 2000, 1, B)
        if G is None:
            return lambda: lib.facl_build_views_philox_f64(*head, out.data_ptr(), None, s)
        return lambda: lib.facl_build_views_philox_gp_f64(*head, G, P, out.data_ptr(), None, s)

    def resident(G=None, P=None):
        head = (src.data_ptr(), tab.data_ptr(), list_r.data_ptr(), B, sel.data_ptr(), B)
        if G is None:
            return lambda: lib.facl_build_views_resident_f64(*head, 2000, 1, out.data_ptr(), None, err2.data_ptr(), s)
        return lambda: lib.facl_build_views_resident_gp_f64(*head, G, P, 2000, 1, out.data_ptr(), None, err2.data_ptr(), s)

    # a non-default recipe: every new kind, a mirrored one and a temporal one (seven jitter draws, as the default list has)
    kinds = np.array([10, 11, 12, 9, 4, 1, 6], dtype=np.int32)             # scale,tilt_neg,tilt_pos,jitter,rot,mirror,t7
    strengths = np.array([0.01, 0.05, 0.8, 0.5, 1.5, 0.25])
    tail = (kinds.ctypes.data, len(kinds), strengths.ctypes.data)

    def disk_recipe(G, P):
        head = (src.data_ptr(), total, 8, meta.data_ptr(), list_d.data_ptr(), counts.data_ptr(), 2000, 1, B)
        return lambda: lib.facl_build_views_philox_recipe_f64(*head, G, P, out.data_ptr(), None, *tail, s)

    def resident_recipe(G, P):
        head = (src.data_ptr(), tab.data_ptr(), list_r.data_ptr(), B, sel.data_ptr(), B)
        return lambda: lib.facl_build_views_resident_recipe_f64(*head, G, P, 2000, 1, out.data_ptr(), None, err2.data_ptr(),
                                                                *tail, s)

    def time_us(fn):
        for _ in range(a.launches):
            ok(fn())
        torch.cuda.synchronize()
        ws = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.launches):
                fn()
            e1.record()
            e1.synchronize()
            ws.append(1e3 * e0.elapsed_time(e1) / a.launches)
        return float(np.median(ws))

    res = {"old_entries_us": {"disk": time_us(disk()), "resident": time_us(resident())}}
    if has_gp and a.sizes:
        res["sizes_us"] = {"%dx%d" % gp: {"disk": time_us(disk(*gp)), "resident": time_us(resident(*gp))} for gp in SIZES}
    if has_recipe and a.sizes:
        res["recipe_us"] = {"%dx%d" % gp: {"disk": time_us(disk_recipe(*gp)), "resident": time_us(resident_recipe(*gp))}
                            for gp in ((10, 512), (24, 2048))}
    assert int(err1.item()) == 0 and err2.cpu().tolist()[0] == 0
    print("RESULT " + json.dumps(res))


def entry_worker(a):
    """One run of the motion training entry in mode a.worker at a.G views of a.P points; one JSON line."""
    import torch
    from facl_amd import cn3d_train_motion_GL as train
    args = ENTRY[a.worker] + ["--data_root", a.data, "--dataset", "ntu120", "--batchSize", str(a.B), "--nepoch", str(a.epochs),
                              "--num_crop", str(a.G), "--SAMPLE_NUM", str(a.P), "--INPUT_FEATURE_NUM", "4", "--graph", "1",
                              "--steps_per_epoch", str(a.steps), "--max_steps_per_epoch", str(a.steps),
                              "--save_root_dir", os.path.join(a.data, "ck")]
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        train.main(args)
    print("RESULT " + json.dumps({"clips_per_s": [float(x) for x in re.findall(r"clips/s: ([0-9.]+)", buf.getvalue())],
                                  "max_memory_allocated": int(torch.cuda.max_memory_allocated())}))


def child(cmd, timeout, env=None):
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       timeout=timeout, text=True, env=env)
    res = re.search(r"^RESULT (.*)$", r.stdout, flags=re.M)
    if r.returncode != 0 or res is None:
        raise SystemExit("%s failed (exit %d); nothing more is started:\n%s" % (cmd, r.returncode, r.stdout[-4000:]))
    return json.loads(res.group(1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--baseline_lib", type=str, default="", help="libfacl_hip.so of the parent commit")
    ap.add_argument("--clips", type=int, default=256)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--entries", type=int, default=1, help="0 = kernels only")
    ap.add_argument("--out", type=str, default="")
    ap.add_argument("--child_timeout", type=int, default=300)
    ap.add_argument("--worker", type=str, default="", choices=["", "kernel"] + list(ENTRY))
    ap.add_argument("--lib", type=str, default="")
    ap.add_argument("--sizes", type=int, default=0)
    ap.add_argument("--sizes_every_round", type=int, default=0,
                    help="1 = time the _gp sizes (and, where the library has them, the recipe entries) in every round and library")
    ap.add_argument("--data", type=str, default="")
    ap.add_argument("--G", type=int, default=24)
    ap.add_argument("--P", type=int, default=2048)
    a = ap.parse_args()
    if a.worker == "kernel":
        return kernel_worker(a)
    if a.worker:
        return entry_worker(a)
    from facl_amd import _lib
    libs = {"this": _lib.lib_path()}
    if a.baseline_lib:
        libs["baseline"] = os.path.abspath(a.baseline_lib)
    common = ["--B", str(a.B), "--reps", str(a.reps), "--launches", str(a.launches)]
    runs = {k: [] for k in libs}
    size_runs, recipe_runs = {k: [] for k in libs}, {k: [] for k in libs}
    sizes = None
    for i in range(a.rounds):
        for k in sorted(libs):                                      # baseline, this, baseline, this, ...
            every = bool(a.sizes_every_round)
            last = k == "this" and i == a.rounds - 1
            res = child(["--worker", "kernel", "--lib", libs[k], "--sizes", str(int(last or every))] + common, a.child_timeout)
            runs[k].append(res["old_entries_us"])
            if k == "this":
                sizes = res.get("sizes_us", sizes)
            if "sizes_us" in res:
                size_runs[k].append(res["sizes_us"])
            if "recipe_us" in res:
                recipe_runs[k].append(res["recipe_us"])
            print("%s round %d: %s %s" % (k, i, res["old_entries_us"], res.get("sizes_us", {}).get("24x2048", "")),
                  file=sys.stderr, flush=True)
    out = {"B": a.B, "launches_per_window": a.launches, "windows_per_run": a.reps, "rounds": a.rounds, "process_per_run": True,
           "source": "four (2048, 8) float64 clouds per clip", "old_entries_us": {}}
    for k, v in runs.items():
        out["old_entries_us"][k] = {p: {"medians": [x[p] for x in v], "median": float(np.median([x[p] for x in v])),
                                        "spread": float(max(x[p] for x in v) - min(x[p] for x in v))}
                                    for p in ("disk", "resident")}
    if "baseline" in runs:
        o = out["old_entries_us"]
        out["no_regression"] = {p: {"this_minus_baseline_us": o["this"][p]["median"] - o["baseline"][p]["median"],
                                    "baseline_spread_us": o["baseline"][p]["spread"],
                                    "holds": o["this"][p]["median"] - o["baseline"][p]["median"] <= o["baseline"][p]["spread"]}
                                for p in ("disk", "resident")}
    def spread(vals):
        return {"medians": vals, "median": float(np.median(vals)), "spread": float(max(vals) - min(vals))}
    if a.sizes_every_round:                                          # the _gp entries per library and round, and a recipe's time
        out["sizes_us_by_library"] = {k: {gp: {p: spread([r[gp][p] for r in v]) for p in ("disk", "resident")} for gp in v[0]}
                                      for k, v in size_runs.items() if v}
        if any(recipe_runs.values()):
            out["recipe_us"] = {"kinds": "scale,tilt_neg,tilt_pos,jitter,rot,mirror,t7",
                                **{k: {gp: {p: spread([r[gp][p] for r in v]) for p in ("disk", "resident")} for gp in v[0]}
                                   for k, v in recipe_runs.items() if v}}
        if "baseline" in out["sizes_us_by_library"]:                 # the rule of 1., for every cell both libraries have
            cells = {"default " + gp: (out["sizes_us_by_library"]["this"][gp], out["sizes_us_by_library"]["baseline"][gp])
                     for gp in ("10x512", "24x2048")}
            if "baseline" in out.get("recipe_us", {}):
                cells.update({"recipe " + gp: (out["recipe_us"]["this"][gp], out["recipe_us"]["baseline"][gp])
                              for gp in out["recipe_us"]["this"]})
            out["no_regression_sizes"] = {c: {p: {"this_minus_baseline_us": t[p]["median"] - b[p]["median"],
                                                  "baseline_spread_us": b[p]["spread"],
                                                  "holds": t[p]["median"] - b[p]["median"] <= b[p]["spread"]}
                                              for p in ("disk", "resident")} for c, (t, b) in cells.items()}
    out["sizes"] = {k: {p: {"us_per_launch": us, "points_per_s": a.B * int(k.split("x")[0]) * int(k.split("x")[1]) / (us * 1e-6)}
                        for p, us in v.items()} for k, v in (sizes or {}).items()}
    if a.entries:
        from tools.time_disk_entry import make_dataset
        tmp = tempfile.mkdtemp(prefix="facl_views_sizes_")
        try:
            make_dataset(tmp, a.clips)
            ecommon = ["--data", tmp, "--B", str(a.B), "--steps", str(a.steps), "--epochs", str(a.epochs)]
            out["step"] = {}
            for G, P in SIZES:
                res = child(["--worker", "synthetic1", "--G", str(G), "--P", str(P)] + ecommon, a.child_timeout)
                k = "%dx%d" % (G, P)
                ms = 1e3 * a.B / res["clips_per_s"][-1]
                out["step"][k] = {"entry_synthetic1_clips_per_s": res["clips_per_s"][-1], "entry_step_ms": ms,
                                  "max_memory_allocated": res["max_memory_allocated"],
                                  "views_share_of_step": {p: v["us_per_launch"] * 1e-3 / ms for p, v in out["sizes"][k].items()}}
                print("step %s: %.3f ms" % (k, ms), file=sys.stderr, flush=True)
            out["end_to_end_24x2048"] = {"clips": a.clips, "steps_timed": a.steps, "epochs": a.epochs,
                                         "synthetic1_clips_per_s": out["step"]["24x2048"]["entry_synthetic1_clips_per_s"]}
            for m in ("resident", "disk_philox"):
                res = child(["--worker", m, "--G", "24", "--P", "2048"] + ecommon, a.child_timeout)
                out["end_to_end_24x2048"][m + "_clips_per_s"] = res["clips_per_s"][-1]
                out["end_to_end_24x2048"][m + "_max_memory_allocated"] = res["max_memory_allocated"]
                print("%s: %.1f clips/s" % (m, res["clips_per_s"][-1]), file=sys.stderr, flush=True)
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
