"""Cost of the momentum key encoder (--key_encoder 1) on the MI355X.

    python tools/time_key_encoder.py [--out profiles/key_encoder.json]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/time_key_encoder.py --kernel_only 1

Default: B=32, G=24, N=2048, D=3, synthetic clouds.  Median fenced milliseconds per graph-replayed step (a device
synchronisation around every timed step) for --neg_queue 4096 alone and with --key_encoder 1 in one process: same model class,
same FusedAdam, GraphedStep; the queue is FULL before the timed window (L / B extra warm-up steps).  Writes JSON: its own keys
are replaced in --out, keys it does not produce (the recorded bench.py lines `bench_ab`, the profiler's `kernel_trace`) are kept.

--kernel_only 1: facl_ema_apply alone over the parameter tensors of the headline model and a copy of them, a few dozen launches
for a kernel trace taken by the profiler in a run of its own (kernel times never come from this script)."""
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

B, G, N, D, L = 32, 24, 2048, 3, 4096
MOMENTUM = 0.999


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


def ema_traffic(net):
    """Bytes facl_ema_apply moves per launch: the copy read and written, the model read."""
    n = sum(p.numel() for p in net.parameters())
    return {"parameters": n, "tensors": len(list(net.parameters())), "hbm_floor_bytes": 3 * 4 * n}


def kernel_only(launches):
    from facl_amd.cn3d_model_conbag import PointNet_Plus
    from facl_amd.key_encoder import KeyEncoder
    dev = torch.device("cuda:0")
    torch.manual_seed(1)
    net = PointNet_Plus(_opt(), gost=G).to(dev).train()
    key = KeyEncoder(net, MOMENTUM)
    for _ in range(launches):
        key.update()
    torch.cuda.synchronize()
    print(json.dumps({"kernel_only": 1, "launches": launches, **ema_traffic(net)}, sort_keys=True))


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "key_encoder.json"))
    p.add_argument("--steps", type=int, default=50)
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--kernel_only", type=int, default=0)
    p.add_argument("--launches", type=int, default=40)
    a = p.parse_args(argv)
    if a.kernel_only:
        return kernel_only(a.launches)
    from facl_amd.cn3d_model_conbag import PointNet_Plus
    from facl_amd.optim import FusedAdam
    from facl_amd.train_common import ContrastiveStep, GraphedStep, synthetic_batch
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev)
    gen.manual_seed(1000)
    pts = synthetic_batch(B, G, N, D, dev, gen)
    res = {"config": {"B": B, "G": G, "N": N, "D": D, "neg_queue": L, "key_momentum": MOMENTUM, "steps": a.steps,
                      "warmup": a.warmup, "device": torch.cuda.get_device_name(0)}}
    for name, flags in (("queue", {}), ("queue_key", dict(key_encoder=1, key_momentum=MOMENTUM))):
        torch.manual_seed(1)
        net = PointNet_Plus(_opt(neg_queue=L, **flags), gost=G).to(dev).train()
        optim = FusedAdam(net.parameters(), lr=3e-4, betas=(0.5, 0.999), eps=1e-6)
        step = ContrastiveStep(net, optim, _opt(neg_queue=L, **flags), G)
        g = GraphedStep(step, pts, G, restore=True)
        res[name + "_graph_ms"] = fenced_ms(lambda: g(pts), a.steps, a.warmup + L // B)
        res[name + "_loss"] = float(g.out[0].detach())
        res[name + "_head_valid"] = list(step.queue.head_valid())
        if flags:
            res["ema_traffic"] = ema_traffic(net)
        del g, step, optim, net
    res["key_minus_queue_us"] = 1e3 * (res["queue_key_graph_ms"] - res["queue_graph_ms"])
    write_results(a.out, res)
    print(json.dumps(res, sort_keys=True))
    return res


def write_results(path, res):
    """`res` into the JSON file at `path`; blocks recorded there by other means (bench_ab, kernel_trace) stay."""
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
