"""Step time of the contrastive step with class-mates as extra positives, in one process on the MI355X.

    python tools/time_loss_sup.py [--out profiles/loss_sup.json]

B=32, G=24, N=2048, D=3, synthetic clouds, the size of tools/time_loss_class.py.  Median fenced milliseconds per graph-replayed
step (a device synchronisation around every timed step) of (normalize, tau 0.1, mask class) and of the same with
--class_positives 1.0, ids drawn from 60 classes and changed before every step, each without a queue and with --neg_queue 4096:
same model class, same FusedAdam, GraphedStep.  The positives add a slot_term evaluation per class cell and, with a queue, one
short launch (the cells' terms against lse).  Also records the min-max spread of the class steps, the yardstick the difference
is read against.  Writes the times as JSON."""
import argparse
import json
import os
import sys
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in (os.path.dirname(os.path.abspath(__file__)), ROOT):
    if d not in sys.path:
        sys.path.insert(0, d)

from time_loss_class import CLASSES, fenced_ms  # noqa: E402


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "loss_sup.json"))
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
    res = {"config": {"B": B, "G": G, "N": N, "D": D, "classes": CLASSES, "steps": a.steps, "warmup": a.warmup,
                      "device": torch.cuda.get_device_name(0)}}
    for L in (0, 4096):
        for name, weight in (("class", 0.0), ("sup", 1.0)):
            name = "%s_queue_%d" % (name, L)
            opt = SimpleNamespace(temperal_num=3, knn_K=64, ball_radius=0.16, ball_radius2=0.25, sample_num_level1=64,
                                  sample_num_level2=64, INPUT_FEATURE_NUM=D, Num_Class=512, batchSize=B, pooling="concatenation",
                                  SAMPLE_NUM=N, loss_normalize=1, loss_temperature=0.1, loss_mask="class", class_positives=weight,
                                  neg_queue=L)
            torch.manual_seed(1)
            net = PointNet_Plus(opt, gost=G).to(dev).train()
            optim = FusedAdam(net.parameters(), lr=3e-4, betas=(0.5, 0.999), eps=1e-6)
            step = ContrastiveStep(net, optim, opt, G)
            g = GraphedStep(step, pts, G, restore=True)
            pool = [torch.randint(0, CLASSES, (B,), device=dev, generator=gen).to(torch.int32) for _ in range(8)]
            calls = [0]

            def run():                                      # as the training entry does before every step: another batch's ids
                step.clip_classes.copy_(pool[calls[0] % len(pool)])
                calls[0] += 1
                g(pts)

            med, lo, hi = fenced_ms(run, a.steps, a.warmup)
            res[name + "_graph_ms"] = med
            res[name + "_min_max_ms"] = [lo, hi]
            res[name + "_loss"] = float(g.out[0].detach())
            del g, step, optim, net
        res["sup_minus_class_queue_%d_us" % L] = 1e3 * (res["sup_queue_%d_graph_ms" % L] - res["class_queue_%d_graph_ms" % L])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))
    return res


if __name__ == "__main__":
    main()
