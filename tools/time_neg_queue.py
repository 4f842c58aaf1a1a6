"""Cost of the cross-batch queue of negative keys (--neg_queue) on the MI355X.

    python tools/time_neg_queue.py [--out profiles/neg_queue.json]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/time_neg_queue.py --kernel_only 4096

Default: B=32, G=24, N=2048, D=3, synthetic clouds.  Median fenced milliseconds per graph-replayed step (a device
synchronisation around every timed step) for --neg_queue 0, 1024 and 4096 in one process: same model class, same FusedAdam,
GraphedStep; every queue is FULL before the timed window (L / B extra warm-up steps), the state it stays in during training.
Beside the differences to 0: the work the queue adds, computed from the shapes.  Writes JSON: its own keys are replaced in
--out, keys it does not produce (the recorded bench.py lines `bench_ab`, the profiler's `kernel_trace_L4096`) are kept.

--kernel_only L: no model; facl_contrast_pair_queue alone on random similarities of that shape (full queue, mask zero), a few
dozen launches for a kernel trace taken by the profiler in a run of its own (kernel times never come from this script)."""
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

B, G, N, D, C = 32, 24, 2048, 3, 512
LENGTHS = (0, 1024, 4096)


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


def added_work(L):
    """What a step with a queue of L rows adds, from the shapes: two R x L x C GEMMs (sim_q forward, its dgrad), and sim_q /
    dsim_q written and read once each by the GEMMs and the loss, plus the scaled copy of dsim_q the backward makes."""
    R = (G + 1) * B
    return {"rows": R, "gemm_flop_each": 2 * R * L * C, "gemms": 2, "sim_q_bytes": 4 * R * L, "dsim_q_bytes": 4 * R * L,
            "loss_hbm_floor_bytes": 4 * R * (G * B + L) * 2}


def kernel_only(L, launches):
    from facl_amd import _lib
    from facl_amd.sa_mlp import _Workspace
    lib = _lib.load_library()
    dev = torch.device("cuda:0")
    R, J = (G + 1) * B, G * B
    torch.manual_seed(1)
    sim, sim_q = torch.randn(R, J, device=dev) * 2.0, torch.randn(R, L, device=dev) * 2.0
    dsim, dsim_q = torch.empty_like(sim), torch.empty_like(sim_q)
    order = torch.randperm(G, device=dev)
    state = torch.tensor([0, L], dtype=torch.int32, device=dev)
    l64, l32 = torch.empty(2, dtype=torch.float64, device=dev), torch.empty(3, device=dev)
    ws = _Workspace.get(dev)
    for _ in range(launches):
        _lib.check(lib.facl_contrast_pair_queue(_lib.ptr(sim), _lib.ptr(sim_q), G, B, B, J, L, _lib.ptr(order), 0, 0, _lib.ptr(state),
                                                _lib.ptr(dsim), _lib.ptr(dsim_q), _lib.ptr(l64), _lib.ptr(l32), _lib.ptr(ws),
                                                _lib.stream()), "facl_contrast_pair_queue")
    torch.cuda.synchronize()
    print(json.dumps({"kernel_only": L, "launches": launches, "losses": l32.tolist(), **added_work(L)}, sort_keys=True))


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "neg_queue.json"))
    p.add_argument("--steps", type=int, default=50)
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--kernel_only", type=int, default=0)
    p.add_argument("--launches", type=int, default=40)
    a = p.parse_args(argv)
    if a.kernel_only:
        return kernel_only(a.kernel_only, a.launches)
    from facl_amd.cn3d_model_conbag import PointNet_Plus
    from facl_amd.optim import FusedAdam
    from facl_amd.train_common import ContrastiveStep, GraphedStep, synthetic_batch
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev)
    gen.manual_seed(1000)
    pts = synthetic_batch(B, G, N, D, dev, gen)
    res = {"config": {"B": B, "G": G, "N": N, "D": D, "steps": a.steps, "warmup": a.warmup,
                      "device": torch.cuda.get_device_name(0)}}
    for L in LENGTHS:
        opt = SimpleNamespace(temperal_num=3, knn_K=64, ball_radius=0.16, ball_radius2=0.25, sample_num_level1=64,
                              sample_num_level2=64, INPUT_FEATURE_NUM=D, Num_Class=512, batchSize=B, pooling="concatenation",
                              SAMPLE_NUM=N, neg_queue=L)
        torch.manual_seed(1)
        net = PointNet_Plus(opt, gost=G).to(dev).train()
        optim = FusedAdam(net.parameters(), lr=3e-4, betas=(0.5, 0.999), eps=1e-6)
        step = ContrastiveStep(net, optim, opt, G)
        g = GraphedStep(step, pts, G, restore=True)
        name = "queue_%d" % L
        res[name + "_graph_ms"] = fenced_ms(lambda: g(pts), a.steps, a.warmup + L // B)
        res[name + "_loss"] = float(g.out[0].detach())
        if L:
            res[name + "_head_valid"] = list(step.queue.head_valid())
            res[name + "_added_work"] = added_work(L)
        del g, step, optim, net
    for L in LENGTHS[1:]:
        res["queue_%d_minus_0_us" % L] = 1e3 * (res["queue_%d_graph_ms" % L] - res["queue_0_graph_ms"])
    write_results(a.out, res)
    print(json.dumps(res, sort_keys=True))
    return res


def write_results(path, res):
    """`res` into the JSON file at `path`; blocks recorded there by other means (bench_ab, kernel_trace_*) stay."""
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
