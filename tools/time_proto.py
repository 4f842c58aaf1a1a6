"""Time the fused prototype contrastive term (facl_amd.proto) at the training shape, next to the torch-fp32
composition of the same forward + backward on the same device (F.normalize, mm, log_softmax, autograd):

    python tools/time_proto.py [--out profiles/proto.json] [--M 800 --B 32 --C 512 --Ks 60 1024]

Recorded per K: the median fenced milliseconds of facl_proto_nce (the bare entry: both launches, no allocation and no read-back
inside the timed window), of the autograd wrapper (the entry plus the backward's one elementwise launch) and of the torch
composition, forward + backward.  Every timing is fenced (device synchronised before the clock starts and before it stops) and
follows warm-up calls; the figure kept is the median of --reps."""
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


def torch_composition(x, classes, protos, proto_inv, scale):
    """The same term in plain torch, fp32: forward and backward -> (loss, dx)."""
    x = x.detach().requires_grad_(True)
    M, K = x.shape[0], protos.shape[0]
    z = torch.nn.functional.normalize(x, dim=1)
    l = torch.mm(z, (protos * proto_inv[:, None]).t()) * scale[None, :]
    rows = torch.arange(M, device=x.device)
    s = classes.long()[rows % classes.shape[0]]
    known = (s >= 0) & (s < K)
    loss = -(torch.log_softmax(l, dim=1)[rows, torch.where(known, s, torch.zeros_like(s))] * known).sum() / M
    loss.backward()
    return loss.detach(), x.grad


def main(args=None):
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "proto.json"))
    p.add_argument("--M", type=int, default=800)
    p.add_argument("--B", type=int, default=32)
    p.add_argument("--C", type=int, default=512)
    p.add_argument("--Ks", type=int, nargs="+", default=[60, 1024])
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--reps", type=int, default=20)
    opt = p.parse_args(args)
    from facl_amd import _lib, proto
    from facl_amd import cluster as fcl
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    g = torch.Generator(device=dev).manual_seed(opt.M)
    lib = _lib.load_library()
    M, B, C = opt.M, opt.B, opt.C
    x = torch.randn(M, C, device=dev, generator=g)
    rows = []
    for K in opt.Ks:
        protos = 20.0 * torch.randn(K, C, device=dev, generator=g)
        proto_inv = fcl.row_inv(protos)
        scale = 1.0 + 9.0 * torch.rand(K, device=dev, generator=g)
        classes = torch.randint(0, K, (B,), device=dev, generator=g).to(torch.int32)
        dstacked, loss, ws, err = proto.buffers(dev, M, C, K)
        entry = lambda: _lib.check(lib.facl_proto_nce(_lib.ptr(x), M, x.stride(0), C, B, _lib.ptr(classes), _lib.ptr(protos),
                                                      _lib.ptr(proto_inv), _lib.ptr(scale), K, _lib.ptr(loss), _lib.ptr(dstacked),
                                                      _lib.ptr(err), _lib.ptr(ws), _lib.stream()), "facl_proto_nce")

        def wrapper():
            xr = x.detach().requires_grad_(True)
            proto.proto_nce_raw(xr, classes, protos, proto_inv, scale)[0].backward()
            return xr.grad

        t_e, t_emin = fenced(entry, opt.warmup, opt.reps)
        t_w, t_wmin = fenced(wrapper, opt.warmup, opt.reps)
        t_t, t_tmin = fenced(lambda: torch_composition(x, classes, protos, proto_inv, scale), opt.warmup, opt.reps)
        assert int(err.item()) == 0
        # the two agree
        loss_t, dx_t = torch_composition(x, classes, protos, proto_inv, scale)
        entry()
        d_loss = float((loss[0] - loss_t).abs())
        d_dx = float((dstacked - dx_t).abs().max() / dx_t.abs().max())
        rows.append({"M": M, "B": B, "C": C, "K": K, "fused_entry_ms": round(t_e, 4), "fused_entry_min_ms": round(t_emin, 4),
                     "fused_autograd_ms": round(t_w, 4), "fused_autograd_min_ms": round(t_wmin, 4),
                     "torch_fp32_fwd_bwd_ms": round(t_t, 4), "torch_fp32_fwd_bwd_min_ms": round(t_tmin, 4),
                     "torch_over_fused_entry": round(t_t / t_e, 3), "torch_over_fused_autograd": round(t_t / t_w, 3),
                     "loss": float(loss[0]), "loss_abs_diff_vs_torch": d_loss, "dx_max_rel_diff_vs_torch": d_dx})
        print(json.dumps(rows[-1]), flush=True)
    result = {"device": torch.cuda.get_device_name(dev), "torch": torch.__version__, "warmup": opt.warmup, "reps": opt.reps,
              "timing": "host clock between device synchronisations, median of reps (launch boundaries and the host calls are inside)",
              "shapes": rows}
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    with open(opt.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    return result


if __name__ == "__main__":
    main()
