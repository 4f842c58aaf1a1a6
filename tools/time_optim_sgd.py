"""Step time under the three optimizers of --optim (FusedAdam, FusedSGD plain and LARS) on the MI355X.

    python tools/time_optim_sgd.py [--out profiles/optim_sgd.json]

B=32, G=24, N=2048, D=3, synthetic clouds, the default loss: the headline step.  Median fenced milliseconds per graph-replayed
step (a device synchronisation around every timed step) with adam, sgd and lars in ONE process: same model class, same
GraphedStep, the three measured in turn and then once more in reverse order, so that a drift of the box shows as a difference
between the two passes instead of as a difference between optimizers.  Also the optimizer launches alone on the same tensors with
random gradients, fenced per step.  Writes JSON."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from time_optim_recipe import B, D, G, N, _net, _opt, fenced_ms  # noqa: E402

KINDS = ("adam", "sgd", "lars")


def make(kind, params):
    from facl_amd.optim import FusedAdam, FusedSGD
    if kind == "adam":
        return FusedAdam(params, lr=3e-4, betas=(0.5, 0.999), eps=1e-6)
    # plain SGD at Adam's 3e-4 diverges on this step within the warm-up (gradient norm ~170): a rate at which the values stay
    # finite, so that no timed step runs on NaN; the rate is a device scalar and does not enter the time
    return FusedSGD(params, lr=3e-4 if kind == "lars" else 1e-6, momentum=0.9, weight_decay=1e-4, lars=kind == "lars", lars_eta=1e-3)


def traffic(net):
    """Bytes per step by the kernels' own reads and writes: Adam reads p, g, m, v and writes p, m, v; SGD reads p, g, buf and writes
    p, buf; LARS reads p and g once more for the norms."""
    n = sum(p.numel() for p in net.parameters())
    return {"parameters": n, "tensors": len(list(net.parameters())), "adam_bytes": 7 * 4 * n, "sgd_bytes": 5 * 4 * n,
            "lars_bytes": 7 * 4 * n}


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_sgd.json"))
    p.add_argument("--steps", type=int, default=50)
    p.add_argument("--warmup", type=int, default=10)
    a = p.parse_args(argv)
    from facl_amd.train_common import ContrastiveStep, GraphedStep, synthetic_batch
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev)
    gen.manual_seed(1000)
    pts = synthetic_batch(B, G, N, D, dev, gen)
    res = {"config": {"B": B, "G": G, "N": N, "D": D, "steps": a.steps, "warmup": a.warmup,
                      "device": torch.cuda.get_device_name(0)}, "graph_ms_passes": {k: [] for k in KINDS}}
    for kind in KINDS + KINDS[::-1]:
        net = _net(dev)
        optim = make(kind, net.parameters())
        step = ContrastiveStep(net, optim, _opt(), G)
        g = GraphedStep(step, pts, G, restore=True)
        res["graph_ms_passes"][kind].append(fenced_ms(lambda: g(pts), a.steps, a.warmup))
        res[kind + "_loss"] = float(g.out[0].detach())
        res["traffic"] = traffic(net)
        del g, step, optim, net
    for kind in KINDS:
        res[kind + "_graph_ms"] = sum(res["graph_ms_passes"][kind]) / 2.0       # both passes are in the file
        if res[kind + "_loss"] != res[kind + "_loss"] or abs(res[kind + "_loss"]) == float("inf"):
            raise FloatingPointError("%s: the timed steps ran on a non-finite loss" % kind)
    for kind in KINDS:                                        # the optimizer launches alone
        net = _net(dev)
        g2 = torch.Generator(device=dev)
        g2.manual_seed(2)
        for q in net.parameters():
            q.grad = 1e-3 * torch.randn(q.shape, device=dev, generator=g2)
        optim = make(kind, net.parameters())
        res[kind + "_optimizer_only_ms"] = fenced_ms(optim.step, a.steps, a.warmup)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))
    return res


if __name__ == "__main__":
    main()
