"""Time one Lloyd iteration of the device k-means (facl_amd.cluster) at the linear probe's size, next to the same
iteration in plain torch on the same device (normalised copy, mm + argmax, index_add_):

    python tools/time_cluster.py [--out profiles/cluster.json] [--n 37920 --K 60 --ld 5632 --widths 5632 512]

Every shape is a column slice (the LAST C columns) of one (n, ld) matrix.  Recorded per shape: the median fenced milliseconds
of facl_cluster_row_inv, of facl_cluster_sums and of the assignment call (facl_knn_topk, k = 1), and the sums pass's bytes
(n C 4, what the algorithm has to read) over its time as a fraction of the HBM peak.  Every timing is fenced (device
synchronised before the clock starts and before it stops) and follows warm-up calls; the figure kept is the median of --reps."""
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

HBM_PEAK = 8.0e12                # bytes/s of an MI355X (public specification), for the fraction reported


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


def torch_iteration(x, cent):
    """The same iteration in plain torch: a normalised copy of both operands, mm + argmax, index_add_ of the unit rows."""
    xn = torch.nn.functional.normalize(x, dim=1)
    lab = torch.mm(xn, torch.nn.functional.normalize(cent, dim=1).t()).argmax(dim=1)
    new = torch.zeros_like(cent)
    new.index_add_(0, lab, xn)
    return lab, new


def main(args=None):
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "cluster.json"))
    p.add_argument("--n", type=int, default=37920)
    p.add_argument("--K", type=int, default=60)
    p.add_argument("--ld", type=int, default=5632)
    p.add_argument("--widths", type=int, nargs="+", default=[5632, 512])
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--reps", type=int, default=20)
    opt = p.parse_args(args)
    from facl_amd import _lib
    from facl_amd import cluster as fcl
    from facl_amd.knn_eval import knn_topk
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    g = torch.Generator(device=dev).manual_seed(opt.ld)
    centres = torch.randn(opt.K, opt.ld, device=dev, generator=g)
    full = centres[torch.arange(opt.n, device=dev) % opt.K] + 4.0 * torch.randn(opt.n, opt.ld, device=dev, generator=g)
    lib = _lib.load_library()
    rows = []
    for C in opt.widths:
        x = full[:, opt.ld - C:]
        n, K = opt.n, opt.K
        cent = x[torch.arange(K, device=dev) * (n // K)].contiguous()
        inv = fcl.row_inv(x)
        labels = knn_topk(x, cent, 1)[1][:, 0].contiguous()
        order, offs = fcl.label_order(labels, K)
        ws = torch.empty(((lib.facl_cluster_ws_bytes(n, K, C) + 7) // 8,), dtype=torch.float64, device=dev)
        err = torch.zeros((1,), dtype=torch.int32, device=dev)
        out = torch.zeros_like(cent)
        # the bare entry: no allocation and no read-back inside the timed window
        sums = lambda: _lib.check(lib.facl_cluster_sums(_lib.ptr(x), n, x.stride(0), C, _lib.ptr(inv), _lib.ptr(order), _lib.ptr(offs),
                                                        K, _lib.ptr(out), _lib.ptr(err), _lib.ptr(ws), _lib.stream()), "facl_cluster_sums")
        rinv = lambda: _lib.check(lib.facl_cluster_row_inv(_lib.ptr(x), n, x.stride(0), C, _lib.ptr(inv), _lib.stream()),
                                  "facl_cluster_row_inv")
        t_s, t_smin = fenced(sums, opt.warmup, opt.reps)
        t_r, t_rmin = fenced(rinv, opt.warmup, opt.reps)
        t_a, t_amin = fenced(lambda: knn_topk(x, cent, 1), opt.warmup, opt.reps)
        t_o, _ = fenced(lambda: fcl.label_order(labels, K), opt.warmup, opt.reps)
        t_t, t_tmin = fenced(lambda: torch_iteration(x, cent), opt.warmup, opt.reps)
        assert int(err.item()) == 0
        # the two iterations agree: the same labels (up to near ties) and the same sums
        lab_t, new_t = torch_iteration(x, cent)
        agree = float((lab_t == labels.long()).float().mean())
        diff = float((out - new_t).abs().max() / new_t.abs().max())
        nbytes = 4.0 * n * C
        rows.append({"n": n, "K": K, "C": C, "ldx": opt.ld, "row_inv_ms": round(t_r, 4), "row_inv_min_ms": round(t_rmin, 4),
                     "sums_ms": round(t_s, 4), "sums_min_ms": round(t_smin, 4), "assign_ms": round(t_a, 4), "assign_min_ms": round(t_amin, 4),
                     "label_order_ms": round(t_o, 4), "sums_bytes": nbytes, "sums_tb_per_s": round(nbytes / (t_s * 1e-3) / 1e12, 3),
                     "sums_hbm_fraction": round(nbytes / (t_s * 1e-3) / HBM_PEAK, 4),
                     "row_inv_hbm_fraction": round(nbytes / (t_r * 1e-3) / HBM_PEAK, 4),
                     "torch_iteration_ms": round(t_t, 4), "torch_iteration_min_ms": round(t_tmin, 4),
                     "torch_over_device_iteration": round(t_t / (t_s + t_a + t_o), 3),
                     "labels_agree": round(agree, 6), "sums_max_rel_diff_vs_torch": diff})
        print(json.dumps(rows[-1]), flush=True)
    result = {"device": torch.cuda.get_device_name(dev), "torch": torch.__version__, "warmup": opt.warmup, "reps": opt.reps,
              "timing": "host clock between device synchronisations, median of reps (a launch boundary and the host call are inside)",
              "hbm_peak_bytes_per_s": HBM_PEAK,
              "note": "sums_bytes counts the feature rows only (n C 4); the fp64 partial sums written and read back are extra traffic",
              "shapes": rows}
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    with open(opt.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    return result


if __name__ == "__main__":
    main()
