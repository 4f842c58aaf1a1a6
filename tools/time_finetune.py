"""Step time of supervised fine-tuning beside the contrastive step, in one process on the MI355X.

    python tools/time_finetune.py [--out profiles/finetune.json]

B=32, G=24, N=2048, D=3, synthetic clouds.  Median fenced milliseconds per step (a device synchronisation around every
timed step) of: the fine-tune step graph-replayed and eager, and the contrastive step built the same way (same model
class, same FusedAdam, GraphedStep), graph-replayed and eager.  Writes the times and their ratios as JSON.

    python tools/time_finetune.py --freeze_bn 1

measures instead the EAGER fine-tune step with frozen BatchNorm (model in eval()) beside the eager train-mode
step -- nothing is captured -- and adds `finetune_frozen_eager_ms`, `finetune_train_eager_ms` and their ratio to the JSON file."""
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
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "finetune.json"))
    p.add_argument("--steps", type=int, default=50)
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--num_class", type=int, default=60)
    p.add_argument("--freeze_bn", type=int, default=0, choices=(0, 1))
    a = p.parse_args(argv)
    from facl_amd.finetune import FineTuneNet, FineTuneStep
    from facl_amd.optim import FusedAdam
    from facl_amd.train_common import ContrastiveStep, GraphedStep, synthetic_batch
    B, G, N, D = 32, 24, 2048, 3
    dev = torch.device("cuda:0")
    opt = SimpleNamespace(temperal_num=3, knn_K=64, ball_radius=0.16, ball_radius2=0.25, sample_num_level1=64,
                          sample_num_level2=64, INPUT_FEATURE_NUM=D, Num_Class=512, batchSize=B, pooling="concatenation",
                          SAMPLE_NUM=N)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1000)
    pts = synthetic_batch(B, G, N, D, dev, gen)
    res = {"config": {"B": B, "G": G, "N": N, "D": D, "num_class": a.num_class, "steps": a.steps, "warmup": a.warmup,
                      "device": torch.cuda.get_device_name(0)}}
    def make(step_cls, **kw):
        torch.manual_seed(1)
        net = FineTuneNet(opt, a.num_class, gost=G).to(dev).train()
        optim = FusedAdam(net.parameters(), lr=3e-4, betas=(0.5, 0.999), eps=1e-6)
        step = step_cls(net, optim, opt, G, **kw)
        if step_cls is FineTuneStep:
            step.labels.copy_(torch.randint(0, a.num_class, (B,), device=dev, generator=gen).to(torch.int32))
        return step

    if a.freeze_bn:
        if os.path.exists(a.out):                        # keep the figures of the default run beside the new ones
            with open(a.out) as f:
                res = {**json.load(f), "config_frozen": res["config"]}
        step = make(FineTuneStep)
        res["finetune_train_eager_ms"] = fenced_ms(lambda: step(pts), a.steps, a.warmup)
        step.freeze_bn = True                            # the running statistics are those of the train-mode steps above
        res["finetune_frozen_eager_ms"] = fenced_ms(lambda: step(pts), a.steps, a.warmup)
        res["finetune_frozen_over_train_eager"] = res["finetune_frozen_eager_ms"] / res["finetune_train_eager_ms"]
    else:
        for name, cls in (("finetune", FineTuneStep), ("contrastive", ContrastiveStep)):
            step = make(cls)
            g = GraphedStep(step, pts, G, restore=True)
            res[name + "_graph_ms"] = fenced_ms(lambda: g(pts), a.steps, a.warmup)
            res[name + "_eager_ms"] = fenced_ms(lambda: step(pts), a.steps, a.warmup)
            del g, step
        res["finetune_over_contrastive_graph"] = res["finetune_graph_ms"] / res["contrastive_graph_ms"]
        res["finetune_over_contrastive_eager"] = res["finetune_eager_ms"] / res["contrastive_eager_ms"]
        res["finetune_eager_over_graph"] = res["finetune_eager_ms"] / res["finetune_graph_ms"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))
    return res


if __name__ == "__main__":
    main()
