#!/usr/bin/env python
"""Fenced median ms/step of the training step (grouping, encoder, both losses, backward, FusedAdam; graph-replayed like
bench.py) at B = 32, T = 24, N = 2048 for several INPUT_FEATURE_NUM in ONE process, one JSON line per width.

    python tools/time_feature_dims.py                          # D = 3, 4, 8
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/time_feature_dims.py --steps 10
                                                               # per-kernel times (a run of its own: tracing moves the step)
"""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--dims", default="3,4,8")
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--T", type=int, default=24)
    ap.add_argument("--N", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    import numpy as np
    import torch
    from facl_amd.cn3d_model_conbag import PointNet_Plus
    from facl_amd.optim import FusedAdam
    from facl_amd.train_common import ContrastiveStep, GraphedStep, synthetic_batch
    dev = torch.device("cuda:0")
    for D in (int(v) for v in a.dims.split(",")):
        torch.manual_seed(1)
        opt = SimpleNamespace(temperal_num=3, knn_K=64, ball_radius=0.16, ball_radius2=0.25, sample_num_level1=64,
                              sample_num_level2=64, INPUT_FEATURE_NUM=D, Num_Class=512, batchSize=a.B,
                              pooling="concatenation", SAMPLE_NUM=a.N)
        net = PointNet_Plus(opt, gost=a.T).to(dev).train()
        optim = FusedAdam(net.parameters(), lr=0.0003, betas=(0.5, 0.999), eps=1e-06)
        gen = torch.Generator(device=dev)
        gen.manual_seed(0)
        batches = [synthetic_batch(a.B, a.T, a.N, D, dev, gen) for _ in range(2)]
        step = GraphedStep(ContrastiveStep(net, optim, opt, a.T), batches[0], a.T)
        for i in range(a.warmup):
            step(batches[i % 2], epoch=0)
        fenced = []
        for i in range(a.steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            step(batches[i % 2], epoch=0)
            torch.cuda.synchronize()
            fenced.append(time.perf_counter() - t0)
        print(json.dumps({"D": D, "B": a.B, "T": a.T, "N": a.N, "steps": a.steps,
                          "ms_per_step_median_fenced": round(1e3 * float(np.median(fenced)), 3),
                          "ms_min": round(1e3 * min(fenced), 3)}), flush=True)
        del step, net, optim, batches
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
