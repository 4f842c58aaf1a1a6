"""Cost of the optimizer recipe (FusedAdam's max_grad_norm / weight_decay / cosine schedule) on the MI355X.

    python tools/time_optim_recipe.py [--out profiles/optim_recipe.json]
    python tools/time_optim_recipe.py --kernel_only 1

Default: B=32, G=24, N=2048, D=3, synthetic clouds, the default loss.  Median fenced milliseconds per graph-replayed step (a
device synchronisation around every timed step) with the recipe off -- FusedAdam's defaults, bench.py's step -- and with
clipping + decoupled decay + warm-up / cosine on, in one process: same model class, same GraphedStep.  Writes JSON: its own keys
are replaced in --out, keys it does not produce (recorded bench.py lines `bench_ab`) are kept.

--kernel_only 1: the optimizer launches alone on the headline model's tensors and random gradients, fenced per step:
facl_grad_sqnorm + facl_adam_prep_ex + facl_adamw_apply against facl_adam_prep + facl_adam_apply."""
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

B, G, N, D = 32, 24, 2048, 3
RECIPE = dict(max_grad_norm=1.0, weight_decay=0.05, schedule="cosine", warmup_steps=100, decay_steps=100000, lr_min=1e-6)


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


def _opt(**flags):
    return SimpleNamespace(temperal_num=3, knn_K=64, ball_radius=0.16, ball_radius2=0.25, sample_num_level1=64,
                           sample_num_level2=64, INPUT_FEATURE_NUM=D, Num_Class=512, batchSize=B, pooling="concatenation",
                           SAMPLE_NUM=N, **flags)


def traffic(net):
    """Bytes per step by the kernels' own reads and writes: Adam reads p, g, m, v and writes p, m, v; the norm reads g once more."""
    n = sum(p.numel() for p in net.parameters())
    return {"parameters": n, "tensors": len(list(net.parameters())), "adam_bytes": 7 * 4 * n, "sqnorm_bytes": 4 * n,
            "sqnorm_partials": sum((p.numel() + 2047) // 2048 for p in net.parameters())}


def _net(dev):
    from facl_amd.cn3d_model_conbag import PointNet_Plus
    torch.manual_seed(1)
    return PointNet_Plus(_opt(), gost=G).to(dev).train()


def kernel_only(a):
    from facl_amd.optim import FusedAdam
    dev = torch.device("cuda:0")
    res = {"kernel_only": 1, "config": {"steps": a.steps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0)}}
    for name, recipe in (("off", {}), ("on", RECIPE)):
        net = _net(dev)
        gen = torch.Generator(device=dev)
        gen.manual_seed(2)
        for p in net.parameters():
            p.grad = 1e-3 * torch.randn(p.shape, device=dev, generator=gen)
        optim = FusedAdam(net.parameters(), lr=3e-4, betas=(0.5, 0.999), eps=1e-6, **recipe)
        res["optimizer_%s_ms" % name] = fenced_ms(optim.step, a.steps, a.warmup)
        if recipe:
            res["grad_norm"], res["clip_coef"], res["traffic"] = float(optim.grad_norm()), float(optim.clip_coef()), traffic(net)
    res["on_minus_off_us"] = 1e3 * (res["optimizer_on_ms"] - res["optimizer_off_ms"])
    print(json.dumps(res, sort_keys=True))
    return res


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_recipe.json"))
    p.add_argument("--steps", type=int, default=50)
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--kernel_only", type=int, default=0)
    a = p.parse_args(argv)
    if a.kernel_only:
        res = kernel_only(a)
        write_results(a.out, {"kernel_only": res})
        return res
    from facl_amd.optim import FusedAdam
    from facl_amd.train_common import ContrastiveStep, GraphedStep, synthetic_batch
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev)
    gen.manual_seed(1000)
    pts = synthetic_batch(B, G, N, D, dev, gen)
    res = {"config": {"B": B, "G": G, "N": N, "D": D, "recipe": RECIPE, "steps": a.steps, "warmup": a.warmup,
                      "device": torch.cuda.get_device_name(0)}}
    for name, recipe in (("off", {}), ("on", RECIPE)):
        net = _net(dev)
        optim = FusedAdam(net.parameters(), lr=3e-4, betas=(0.5, 0.999), eps=1e-6, **recipe)
        step = ContrastiveStep(net, optim, _opt(), G)
        g = GraphedStep(step, pts, G, restore=True)
        res[name + "_graph_ms"] = fenced_ms(lambda: g(pts), a.steps, a.warmup)
        res[name + "_loss"] = float(g.out[0].detach())
        if recipe:
            res["grad_norm"], res["clip_coef"], res["lr"] = float(optim.grad_norm()), float(optim.clip_coef()), float(optim.current_lr())
            res["traffic"] = traffic(net)
        del g, step, optim, net
    res["on_minus_off_us"] = 1e3 * (res["on_graph_ms"] - res["off_graph_ms"])
    write_results(a.out, res)
    print(json.dumps(res, sort_keys=True))
    return res


def write_results(path, res):
    """`res` into the JSON file at `path`; blocks recorded there by other means (bench_ab, kernel_only) stay."""
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    kept = {}
    if os.path.exists(path):
        with open(path) as f:
            kept = json.load(f)
    with open(path, "w") as f:
        json.dump({**kept, **res}, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
