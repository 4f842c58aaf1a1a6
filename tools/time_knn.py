"""Time the weighted-kNN evaluation (facl_amd.knn_eval.knn_predict: fused similarity GEMM + top-k, then the vote) on
synthetic features of the linear probe's size, next to a torch baseline on the same device that produces the same result:
chunked torch.mm on normalised fp32 rows + topk, the chunk sized so that it never holds more than 1 GB of similarities.

    python tools/time_knn.py [--out profiles/knn_eval.json] [--nq 18960 --nb 37920 --widths 5632 11264 --k 20]

Every timing is fenced (device synchronised before the clock starts and before it stops) and follows warm-up calls; the
figure kept is the median of --reps calls."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FP16_MFMA_PEAK = 2.5e15          # dense fp16 matrix flop/s of an MI355X (public specification), for the fraction reported


def baseline_predict(q, x, labels, k, T, num_class, max_sim_bytes=1 << 30):
    """torch: F.normalize, chunked mm + topk, exp-weighted scatter vote."""
    qn, xn = torch.nn.functional.normalize(q, dim=1), torch.nn.functional.normalize(x, dim=1)
    chunk = max(1, max_sim_bytes // (4 * x.shape[0]))
    preds = []
    for i in range(0, q.shape[0], chunk):
        s = torch.mm(qn[i:i + chunk], xn.t())
        v, ix = s.topk(k, dim=1)
        sc = torch.zeros(v.shape[0], num_class, device=q.device)
        sc.scatter_add_(1, labels[ix], torch.exp(v / T))
        preds.append(sc.argmax(dim=1))
    return torch.cat(preds)


def fenced(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts)


def main(args=None):
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_eval.json"))
    p.add_argument("--nq", type=int, default=18960)
    p.add_argument("--nb", type=int, default=37920)
    p.add_argument("--widths", type=int, nargs="+", default=[5632, 11264])
    p.add_argument("--k", type=int, default=20)
    p.add_argument("--T", type=float, default=0.1)
    p.add_argument("--num_class", type=int, default=60)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--reps", type=int, default=5)
    opt = p.parse_args(args)
    from facl_amd.knn_eval import knn_predict, knn_topk
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    rows = []
    for C in opt.widths:
        g = torch.Generator(device=dev).manual_seed(C)
        # class centres + noise, so that neighbours carry a signal and the two paths can be compared on their predictions
        centres = torch.randn(opt.num_class, C, device=dev, generator=g)
        yb = torch.arange(opt.nb, device=dev) % opt.num_class
        yq = torch.arange(opt.nq, device=dev) % opt.num_class
        x = centres[yb] + 4.0 * torch.randn(opt.nb, C, device=dev, generator=g)
        q = centres[yq] + 4.0 * torch.randn(opt.nq, C, device=dev, generator=g)
        fused = lambda: knn_predict(q, x, yb, k=opt.k, T=opt.T, num_class=opt.num_class)
        base = lambda: baseline_predict(q, x, yb, opt.k, opt.T, opt.num_class)
        topk = lambda: knn_topk(q, x, opt.k)
        agree = float((fused()[0].long() == base()).float().mean())
        t_f, t_fmin = fenced(fused, opt.warmup, opt.reps)
        t_k, _ = fenced(topk, 1, opt.reps)
        t_b, t_bmin = fenced(base, opt.warmup, opt.reps)
        flop = 2.0 * opt.nq * opt.nb * C
        rows.append({"nq": opt.nq, "nb": opt.nb, "C": C, "k": opt.k, "fused_ms": round(t_f, 3), "fused_min_ms": round(t_fmin, 3),
                     "fused_topk_only_ms": round(t_k, 3), "torch_ms": round(t_b, 3), "torch_min_ms": round(t_bmin, 3),
                     "torch_over_fused": round(t_b / t_f, 3), "predictions_agree": round(agree, 5),
                     "useful_tflops_fused": round(flop / t_k / 1e9, 1),
                     "fp16_mfma_fraction": round(3.0 * flop / (t_k * 1e-3) / FP16_MFMA_PEAK, 4)})
        print(json.dumps(rows[-1]), flush=True)
        del x, q, centres
        torch.cuda.empty_cache()
    result = {"device": torch.cuda.get_device_name(dev), "torch": torch.__version__, "warmup": opt.warmup, "reps": opt.reps,
              "timing": "host clock between device synchronisations, median of reps", "fp16_mfma_peak_flops": FP16_MFMA_PEAK,
              "note": "fp16_mfma_fraction counts the three fp16 products of the exact split per multiply-add",
              "shapes": rows}
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    with open(opt.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    return result


if __name__ == "__main__":
    main()
