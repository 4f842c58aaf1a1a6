"""Step time of the contrastive step under the loss modes, in one process on the MI355X.

    python tools/time_loss_modes.py [--out profiles/loss_modes.json]

B=32, G=24, N=2048, D=3, synthetic clouds.  Median fenced milliseconds per graph-replayed step (a device synchronisation
around every timed step) of the default loss, of (normalize, tau 0.1, mask zero) and of (normalize, tau 0.1, mask exclude):
same model class, same FusedAdam, GraphedStep.  The non-default modes add two small launches (the row pass, forward and
backward) to the default step.  Writes the times and their differences to the default as JSON."""
import argparse
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

MODES = (("default", dict(loss_normalize=0, loss_temperature=1.0, loss_mask="zero")),
         ("cos_t0.1_zero", dict(loss_normalize=1, loss_temperature=0.1, loss_mask="zero")),
         ("cos_t0.1_exclude", dict(loss_normalize=1, loss_temperature=0.1, loss_mask="exclude")))


def fenced_ms(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "loss_modes.json"))
    p.add_argument("--steps", type=int, default=50)
    p.add_argument("--warmup", type=int, default=10)
    a = p.parse_args(argv)
    from facl_amd.cn3d_model_conbag import PointNet_Plus
    from facl_amd.optim import FusedAdam
    from facl_amd.train_common import ContrastiveStep, GraphedStep, synthetic_batch
    B, G, N, D = 32, 24, 2048, 3
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev)
    gen.manual_seed(1000)
    pts = synthetic_batch(B, G, N, D, dev, gen)
    res = {"config": {"B": B, "G": G, "N": N, "D": D, "steps": a.steps, "warmup": a.warmup,
                      "device": torch.cuda.get_device_name(0)}}
    for name, flags in MODES:
        opt = SimpleNamespace(temperal_num=3, knn_K=64, ball_radius=0.16, ball_radius2=0.25, sample_num_level1=64,
                              sample_num_level2=64, INPUT_FEATURE_NUM=D, Num_Class=512, batchSize=B, pooling="concatenation",
                              SAMPLE_NUM=N, **flags)
        torch.manual_seed(1)
        net = PointNet_Plus(opt, gost=G).to(dev).train()
        optim = FusedAdam(net.parameters(), lr=3e-4, betas=(0.5, 0.999), eps=1e-6)
        step = ContrastiveStep(net, optim, opt, G)
        g = GraphedStep(step, pts, G, restore=True)
        res[name + "_graph_ms"] = fenced_ms(lambda: g(pts), a.steps, a.warmup)
        res[name + "_loss"] = float(g.out[0].detach())
        del g, step, optim, net
    for name, _ in MODES[1:]:
        res[name + "_minus_default_us"] = 1e3 * (res[name + "_graph_ms"] - res["default_graph_ms"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))
    return res


if __name__ == "__main__":
    main()
