#!/usr/bin/env python
"""Clips per second of the 3DV generation (facl_amd/gen3dv.py) on 60-frame 424x512 synthetic depth clips at a few batch
sizes, split into decode/upload, kernels and write-out, beside the NumPy restatement (tests/ref3dv.py) on one core of the same
box in the same run.  Writes profiles/gen3dv.json.

    python tools/time_generate_3dv.py [--clips 8] [--batches 1,4,8] [--out profiles/gen3dv.json]
"""
import argparse
import json
import os
import random
import socket
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ref3dv as T                                          # noqa: E402
from facl_amd import _lib, gen3dv, generate_3dv            # noqa: E402


def clip(i):
    return T.make_clip(dict(n=60, hw=(424, 512), parts=[(250, 250 + 3 * i, 125, 90, 2600, 0, 1, 0, 90),
                                                         (190, 150 + 5 * i, 34, 28, 2300, 1, 2, 12, 0)]))


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--clips", type=int, default=8)
    ap.add_argument("--batches", default="1,4,8")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gen3dv.json"))
    opt = ap.parse_args()
    torch.set_num_threads(1)
    names = ["S001C001P%03dR001A001" % (i + 1) for i in range(opt.clips)]
    clips = [clip(i) for i in range(opt.clips)]
    res = {"box": socket.gethostname(), "gpu": torch.cuda.get_device_name(0), "clips": opt.clips,
           "frames": 60, "image": [424, 512], "upload_MB_per_clip": round(61 * 424 * 512 * 2 / 1e6, 1)}
    with tempfile.TemporaryDirectory() as tmp:
        for n, c in zip(names, clips):
            np.save(os.path.join(tmp, n + ".npy"), c)
        t0 = time.perf_counter()
        loaded = [generate_3dv.load_clip(n, os.path.join(tmp, n + ".npy")) for n in names]
        res["decode_npy_s_per_clip"] = (time.perf_counter() - t0) / opt.clips
        # NumPy restatement, one core
        t0 = time.perf_counter()
        nref = min(2, opt.clips)
        for c in clips[:nref]:
            T.generate_clip(c, np.random.RandomState(0), random.Random(0))
        res["numpy_restatement_s_per_clip"] = (time.perf_counter() - t0) / nref
        gen3dv.generate_clips(loaded[:1], names[:1], mode="philox", seed=1)                   # warm-up: library, allocator
        res["device"] = {}
        for bs in [int(b) for b in opt.batches.split(",")]:
            _lib.TIMING = {}
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            outs = []
            for i in range(0, opt.clips, bs):
                outs += gen3dv.generate_clips(loaded[i:i + bs], names[i:i + bs], mode="philox", seed=1)
            torch.cuda.synchronize()
            total = time.perf_counter() - t0
            tab = _lib.timing_table()
            _lib.TIMING = None
            t0 = time.perf_counter()
            for n, arrays in zip(names, outs):
                for p, a in zip(generate_3dv.out_paths(os.path.join(tmp, "o%d" % bs), 60, n), arrays):
                    generate_3dv.write_atomic(p, a)
            wr = time.perf_counter() - t0
            res["device"]["batch_%d" % bs] = {
                "clips_per_s": opt.clips / total, "total_s_per_clip": total / opt.clips,
                "upload_ms_per_clip": tab["gen3dv_upload"][0] * tab["gen3dv_upload"][1] / opt.clips,
                "kernels_ms_per_clip": sum(v[0] * v[1] for k, v in tab.items() if k != "gen3dv_upload") / opt.clips,
                "kernel_ms_per_batch": {k: v[0] for k, v in tab.items() if k != "gen3dv_upload"},
                "write_s_per_clip": wr / opt.clips}
    os.makedirs(os.path.dirname(opt.out), exist_ok=True)
    with open(opt.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps(res, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
