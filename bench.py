#!/usr/bin/env python
"""bench.py -- contrastive-step clips/sec on synthetic clouds (BASELINE.json metric).

    python bench.py [--gpus N --steps K --warmup W]            # N > 1: starts its own N ranks (torch.distributed.run)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \\
        bench.py --gpus N --steps K --warmup W                 # ... or is started as one of them
    python bench.py --full                                     # + fenced-step median, in-step rooflines, CPU baseline
    python bench.py --dump-outputs DIR                         # + what the last timed step computed, as DIR/<name>.npy

A plain run sets up, warms up, times the K steps and prints the result line; everything else it can measure
(`ms_per_step_median_fenced`, `roofline` / `roofline_more`, `cpu_baseline`) runs only under --full, after the timed steps.

One "step" = one full training iteration of the reference loop body (cn3d_train_motion_GL.py:224-335) on a
batch already resident in HBM: view-major reshape -> kNN/radius grouping -> encoder forward -> global + circle
loss -> backward -> Adam.  Workload at N=1 = BASELINE.json configs[1]: motion stream, B=32, T=24 views,
N=2048 points (`--config appearance` = configs[2], the appearance entry's step; `--config dense` = configs[4]).
Weak scaling: every rank processes its own B clips; the embeddings all-gather, SyncBN all-reduces and the gradient
all-reduce are the exchange steps (facl_amd/dist.py).  Prints ONE JSON line on rank 0.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_MFMA_F32_TFLOPS = 157.3     # /opt/skills/guides/MI355X_MICROARCH.md, "Peak FP32 (matrix)"
PEAK_MFMA_BF16_TFLOPS = 2500.0   # same guide, BF16/FP16 dense (the split-bf16 and the fp16 kernels run on this pipe)
PEAK_HBM_GBPS = 8000.0


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--config", choices=("motion", "appearance", "dense", "extract"), default="motion",
                    help="motion = BASELINE configs[1] (headline); appearance = configs[2]; dense = configs[4]; extract = the "
                         "feature-extraction path (SURVEY 8 f-1: eval-mode encoder, extract_motion_feature.py), own metric string")
    ap.add_argument("--B", type=int, default=None, help="clips per GPU (default 32; dense: 8)")
    ap.add_argument("--T", type=int, default=None, help="views per clip (reference: gost / num_crop; default 24, dense 32)")
    ap.add_argument("--N", type=int, default=None, help="points per view (default 2048, dense 4096)")
    ap.add_argument("--D", type=int, default=3, help="input channels (north_star: 3-ch; checkpoints: 4)")
    ap.add_argument("--precision", choices=("f32", "x3", "x3b"), default="f32",
                    help="f32 (default, the headline): fp32-grade bf16x6 contractions; x3: opt-in three-product variant "
                         "(~1e-5 relative per GEMM); x3b: three products in the BACKWARD GEMMs only (features / loss unchanged)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, also measure what the headline does not need: the median of K fenced steps, "
                         "the in-step kernel rooflines and the CPU baseline (off: set-up, warm-up, timed steps, result line only)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed (returned arrays; for the training configs also the model "
                         "state after it) as DIR/<name>.npy in float32 / float64")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--fps", type=int, default=0, help="1: FPS-reorder the views on the GPU inside the timed step")
    ap.add_argument("--graph", type=int, default=1, help="1: replay the step as HIP graph(s): one graph on a single GPU, graph "
                                                         "segments cut at every collective under data parallelism")
    ap.add_argument("--rehearse-dp", type=int, default=0,
                    help="1 (with --gpus 1): run the data-parallel code path on a 1-rank RCCL group -- every collective of the "
                         "N>1 step executes (as an identity) -- to time that path on a one-GPU box; never the headline")
    ap.add_argument("--cpu-clips", type=int, default=32, help="clips in the bounded CPU-baseline sample (default: the metric's own B = 32)")
    a = ap.parse_args()
    if a.steps < 1 or a.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    dflt = {"motion": (32, 24, 2048), "appearance": (32, 24, 2048), "dense": (8, 32, 4096), "extract": (32, 24, 2048)}[a.config]
    a.B = dflt[0] if a.B is None else a.B
    a.T = dflt[1] if a.T is None else a.T
    a.N = dflt[2] if a.N is None else a.N
    return a


# ---------------------------------------------------------------------------------------------------------------------
# N > 1 without an outer launcher: become the launcher.  Nothing in this branch touches the GPU (device_count() does not
# initialise HIP on this image); the ranks are fresh child processes and this process only relays their JSON line.
def spawn_ranks(a):
    import torch
    have = torch.cuda.device_count()
    rehearsal = os.environ.get("FACL_DIST_BACKEND") == "gloo"          # N ranks on fewer devices: CPU-collective rehearsal only
    if have < a.gpus and not rehearsal:
        print("bench.py: --gpus %d requested but only %d device(s) visible" % (a.gpus, have), file=sys.stderr)
        return 2

    def attempt(extra_args, extra_env):
        s = socket.socket()
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
        s.close()
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(a.gpus),
               "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:] + extra_args
        env = dict(os.environ)
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        env.setdefault("OMP_NUM_THREADS", "1")
        env.setdefault("TORCH_NCCL_ASYNC_ERROR_HANDLING", "1")   # a timed-out collective ends the rank instead of waiting on
        env.update(extra_env)
        p = subprocess.Popen(cmd, stdout=subprocess.PIPE, env=env, text=True)
        line = None
        for ln in p.stdout:
            if ln.lstrip().startswith('{"metric"'):
                line = ln.strip()
            else:
                sys.stderr.write(ln)
        return p.wait(), line

    rc, line = attempt([], {})
    if (rc != 0 or line is None) and a.graph:
        # ONE more attempt, as a fresh process tree (never a re-exec of a rank that touched the GPU), on eager launches:
        # whatever went wrong while capturing / replaying graph segments must not cost the measurement
        reason = "graph-segment run failed: exit %d, %s" % (rc, "no result line" if line is None else "result line present")
        print("bench.py: the %d-rank child run failed (exit %d); retrying once with --graph 0" % (a.gpus, rc), file=sys.stderr)
        env2 = {"FACL_BENCH_LAUNCH_NOTE": reason}
        for k in ("FACL_TEST_CAPTURE_FAIL", "FACL_TEST_CAPTURE_EXIT"):
            env2[k] = ""
        rc, line = attempt(["--graph", "0"], env2)
    if rc != 0 or line is None:
        print("bench.py: the %d-rank child run failed (exit %d)" % (a.gpus, rc), file=sys.stderr)
        return rc or 1
    print(line)
    return 0


def make_opt(a):
    from types import SimpleNamespace
    return SimpleNamespace(temperal_num=3, knn_K=64, ball_radius=0.16, ball_radius2=0.25, sample_num_level1=64,
                           sample_num_level2=64, INPUT_FEATURE_NUM=a.D, Num_Class=512, batchSize=a.B,
                           pooling="concatenation", SAMPLE_NUM=a.N)


def _baseline_metric():
    """BASELINE.json's metric string, verbatim (the file ships with the repository)."""
    try:
        return json.load(open(os.path.join(ROOT, "BASELINE.json")))["metric"]
    except Exception:
        return "contrastive-step clips/sec (B=32,T=24,N=2048) at 1/2/4/8 MI355X"


def _pmc_traffic(a, kernel):
    """HBM bytes per launch from OFFLINE PMC passes (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, profiles/pmc_traffic.json):
    reported only when the shape matches the one the counters were collected at, else null.  (label, build) tell
    which build the counters belong to."""
    try:
        pm = json.load(open(os.path.join(ROOT, "profiles", "pmc_traffic.json")))
        if pm["shape"] == {"B": a.B, "T": a.T, "N": a.N, "D": a.D}:
            return pm.get(kernel), "offline rocprofv3 --pmc, build %s" % pm.get("build", "r01")
    except Exception:
        pass
    return None, None


def _pmc_mfma(a, kernel):
    """MFMA-pipe utilisation of the launch from OFFLINE PMC passes (profiles/pmc_mfma_util.json, r02_pmc_mfma_util.md)."""
    try:
        pm = json.load(open(os.path.join(ROOT, "profiles", "pmc_mfma_util.json")))
        if pm["shape"] == {"B": a.B, "T": a.T, "N": a.N, "D": a.D} and getattr(a, "precision", "f32") == "f32":
            return pm.get(kernel)
    except Exception:
        pass
    return None


# ---------------------------------------------------------------------------------------------------------------------
# Roofline models of the heavy entry points (DESIGN.md section 3 derives every figure).  A "unit" is one group of 64
# neighbour positions; nunits = M*S.  pipe "f32": v_mfma_f32_32x32x2_f32 (157.3 TFLOP/s, algorithmic FLOPs);
# pipe "bf16x6": exact 3-way bf16 split on v_mfma_f32_32x32x16_bf16 -- 6 executed bf16 FLOPs per algorithmic one, priced
# against the 2.5 PFLOP/s dense bf16 peak.
def kernel_models(a, K=64):
    M = a.B * a.T
    S = 512 if a.config == "dense" else 64             # level-1 centroids per cloud (facl_amd/dense.py: S1)
    nunits, D = M * S, a.D
    sa_f32 = os.environ.get("FACL_SA_F32") == "1"
    bwd2_f32 = os.environ.get("FACL_BWD2_F32") == "1"
    y2 = 64 * 64 * 4                                   # one (64 pos x 64 ch) fp32 tile
    fwd_h3 = os.environ.get("FACL_FWD_H3", "1") != "0"  # forward arithmetic of facl_sa_fwd3 / the row-streamed GEMMs (sa_mlp.py)
    return {
        # FPS (when --fps 1): the cloud's xyz read once, m = S picks written; the S-1 passes over the cloud stay on chip
        "facl_fps": dict(kernel="k_fps", flops=M * S * a.N * 9.0, pipe="valu", bytes=M * (a.N * D * 4.0 + S * 4.0)),
        "facl_group": dict(kernel="k_group", flops=M * S * a.N * 8.0, pipe="valu",
                           bytes=M * (a.N * D * 4.0 + S * K * D * 4.0 + S * 12.0)),
        # eval mode, one kernel: x -> pooled; layers 2 and 3 on the MFMA (fp16x3), 64*D*4 B in and 1 KiB out per unit
        "facl_sa_eval": dict(kernel="k_sa_eval", pipe="fp16x3", flops=nunits * 2.0 * 64 * (64 + 256) * 64,
                             bytes=nunits * (64 * D * 4.0 + 1024.0)),
        "facl_sa_fwd2": dict(kernel="k_sa_fwd2" if sa_f32 else "k_sa_fwd2_sb", pipe="f32" if sa_f32 else "fp16x3" if fwd_h3 else "bf16x6",
                             flops=nunits * 2.0 * 64 * 64 * 64, bytes=nunits * (64 * D * 4.0 + y2)),
        "facl_sa_fwd3": dict(kernel="k_sa_fwd3_sb<fp16>" if a.config == "dense" else ("k_sa_fwd3" if sa_f32 else
                                    "k_sa_fwd3_sb<x3>" if getattr(a, "precision", "f32") == "x3" else "k_sa_fwd3_sb"),
                             pipe="f16" if a.config == "dense" else ("f32" if sa_f32 else "bf16x3" if getattr(a, "precision", "f32") == "x3"
                                                                     else "fp16x3" if fwd_h3 else "bf16x6"),
                             flops=nunits * 2.0 * 64 * 64 * 256, bytes=nunits * (y2 + 1024.0 + 256.0)),
        "facl_sa_bwd1": dict(kernel="k_sa_bwd1", pipe="fp16x3", flops=nunits * (2.0 * 64 * 64 * 64 + 2.0 * 256 * 64),
                             bytes=nunits * (2.0 * y2 + 1024 + 256)),
        "facl_sa_bwd_w3": dict(kernel="k_sa_bwd_w3p" if os.environ.get("FACL_BWD_W3_PAIR", "1") != "0" else "k_sa_bwd_w3", pipe="fp16x3", flops=nunits * (2.0 * 64 * 64 * 64 + 2.0 * 256 * 64),
                               bytes=nunits * (y2 + 1024.0 + 256.0)),
        # da1 = dy2 W2 (2*64*64) + dW2 += dy2^T a1 (2*64*64) + R1 += [x|1]^T dz1 (2*64*4) per position
        "facl_sa_bwd2": dict(kernel="k_sa_bwd2" if bwd2_f32 else "k_sa_bwd2_sb",
                             pipe="f32" if bwd2_f32 else "fp16x3" if os.environ.get("FACL_BWD_H3", "1") != "0" else "bf16x6",
                             flops=nunits * 64.0 * (2 * 64 * 64 + 2 * 64 * 64 + 2 * 64 * 4),
                             bytes=nunits * (2.0 * y2 + 64 * D * 4.0)),
    }


def _gemm_model(label):
    parts = label.split()
    kind, dims = parts[0], parts[1]
    m, k, n = (int(v) for v in dims.split("x"))
    tag = parts[2] if len(parts) > 2 else ""
    pipe = "f16" if tag == "f16" else "bf16x3" if tag == "x3" else "fp16x3" if tag == "h3" else \
        ("f32" if os.environ.get("FACL_GEMM_F32") == "1" else "bf16x6")
    name = {"facl_gemm_fwd": "k_gemm_sb fwd", "facl_gemm_dgrad": "k_gemm_sb dgrad", "facl_gemm_wgrad": "k_gemm_sb wgrad",
            "facl_gemm_rs_fwd": "k_gemm_rs fwd", "facl_gemm_rs_dgrad": "k_gemm_rs dgrad", "facl_gemm_rs_wgrad": "k_wgrad_rs wgrad"}[kind]
    return dict(kernel="%s %s%s" % (name, dims, " (fp16 inputs)" if pipe == "f16" else " (bf16x3)" if pipe == "bf16x3" else ""),
                pipe=pipe, flops=2.0 * m * k * n,
                bytes=4.0 * (m * k + k * n + m * n))


def price(model, ms):
    """One roofline record: both roofs are evaluated, `bound` is the one that allows the LONGER time at its peak."""
    sec = ms * 1e-3
    ex = model["flops"] * {"bf16x6": 6.0, "bf16x3": 3.0, "fp16x3": 3.0}.get(model["pipe"], 1.0)
    peak_tf = PEAK_MFMA_BF16_TFLOPS if model["pipe"] in ("bf16x6", "bf16x3", "fp16x3", "f16") else PEAK_MFMA_F32_TFLOPS
    t_mfma = ex / (peak_tf * 1e12) if model["pipe"] != "valu" else 0.0
    t_hbm = model["bytes"] / (PEAK_HBM_GBPS * 1e9)
    rec = {"kernel": model["kernel"], "ms_per_launch": round(ms, 4)}
    if t_mfma >= t_hbm:
        ach = ex / sec / 1e12
        rec.update(bound="mfma", achieved=round(ach, 1), peak=peak_tf, unit="TFLOP/s", frac=round(ach / peak_tf, 4))
    else:
        ach = model["bytes"] / sec / 1e9
        rec.update(bound="hbm", achieved=round(ach, 1), peak=PEAK_HBM_GBPS, unit="GB/s", frac=round(ach / PEAK_HBM_GBPS, 4))
    rec.update(pipe=model["pipe"], algorithmic_flops_per_launch=model["flops"], algorithmic_bytes_per_launch=model["bytes"],
               algorithmic_tflops=round(model["flops"] / sec / 1e12, 1), hbm_frac=round(model["bytes"] / sec / 1e9 / PEAK_HBM_GBPS, 4))
    if model["pipe"] == "bf16x6":
        rec["executed_bf16_flops_per_launch"] = ex
    if model["pipe"] == "fp16x3":
        rec["executed_fp16_flops_per_launch"] = ex
    return rec


def step_rooflines(a, eager_step, batches, nsteps=8):
    """Every heavy entry point of the step timed INSIDE the training step: `nsteps` extra eager steps (after the timed
    region) with HIP events recorded on the launch stream around each entry (facl_amd/_lib.py: timed; a stand-alone
    loop of one kernel sits elsewhere on the clock/power curve and would not match the rocprof average of the real
    run).  The brackets include the one or two ~5 us partial-sum reduction launches an entry issues after its kernel.
    Returns (roofline of the LONGEST kernel, the others sorted by time)."""
    from facl_amd import _lib
    _lib.TIMING = {}
    try:
        for i in range(nsteps):
            eager_step(batches[i % 2], epoch=0)
        table = _lib.timing_table()
    finally:
        _lib.TIMING = None
    models = kernel_models(a)
    recs = []
    for label, (ms, n) in table.items():
        m = models.get(label) or (_gemm_model(label) if label.startswith("facl_gemm_") else None)
        if m is None:
            continue
        r = price(m, ms)
        r["launches_per_step"] = round(n / nsteps, 2)
        r["measured"] = "in-step HIP events, %d eager steps" % nsteps
        r["traffic"], src = _pmc_traffic(a, m["kernel"])
        if src:
            r["traffic_source"] = src
        mu = _pmc_mfma(a, m["kernel"])
        if mu:
            r["mfma_util_pmc"] = mu            # {"busy_frac", "MfmaUtil" (rocprofv3, %), "clock_ghz"}: offline counters, same build
        recs.append(r)
    recs.sort(key=lambda r: -r["ms_per_launch"])
    # sub-20-us launches are glue, not roofline material (kept only when nothing else was measured: toy shapes)
    big = [r for r in recs if r["ms_per_launch"] >= 0.02 or not r["kernel"].startswith("k_gemm")] or recs
    return big[0], big[1:]


def host_cores():
    """CPU threads this process may really use: affinity mask capped by the cgroup CPU quota."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        q, p = open("/sys/fs/cgroup/cpu.max").read().split()
        if q != "max":
            n = max(1, min(n, int(float(q) / float(p) + 0.5)))
    except Exception:
        pass
    return n


def cpu_baseline(a):
    """The oracle's training step (a port of the reference's op sequence onto torch-CPU; timed against the imported
    reference in the build container: x1.04-1.08) on the host cores, on a bounded sample:
    `cpu_clips` clips of the same (T, N, D) shape, 1 warm-up + 3 timed steps."""
    import numpy as np
    import torch
    from oracle import step as OS
    from oracle import encoder as E
    from oracle.weights import formula_state_dict
    cores = host_cores()
    torch.set_num_threads(cores)
    Bc, G = a.cpu_clips, a.T
    sd = E.clone_state(formula_state_dict(a.D))
    opt = OS.AdamState(sd)
    g = torch.Generator().manual_seed(0)
    order = np.arange(G)
    times = []
    for it in range(4):
        pts = OS.view_major(torch.rand(Bc, G, a.N, a.D, generator=g) - 0.5)
        t0 = time.time()
        OS.train_step(sd, opt, pts, Bc, G, 64, 64, 0.16 if a.N != 512 else 0.06, order)
        times.append(time.time() - t0)
    t = float(np.median(times[1:]))
    return {"value": round(Bc / t, 3), "unit": "clips/s", "cores": cores, "kind": "port",
            "sample": f"B={Bc} clips x T={G} views x N={a.N} pts, D={a.D}: 1 warm-up + 3 timed steps "
                      f"(median {t:.2f} s/step, first {times[0]:.2f} s) of oracle.step.train_step"}


def cpu_baseline_extract(a):
    """Extraction configuration: oracle.step.extract_step (grouping + the encoder under eval() + the feature layout, torch-CPU
    ops) on a bounded sample: `cpu_clips` clips of the same (T, N, D) shape, 1 warm-up + 3 timed passes."""
    import numpy as np
    import torch
    from oracle import step as OS
    from oracle import encoder as E
    from oracle.weights import formula_state_dict
    cores = host_cores()
    torch.set_num_threads(cores)
    Bc, G = a.cpu_clips, a.T
    sd = E.clone_state(formula_state_dict(a.D))
    g = torch.Generator().manual_seed(0)
    times = []
    for it in range(4):
        pts = OS.view_major(torch.rand(Bc, G, a.N, a.D, generator=g) - 0.5)
        t0 = time.time()
        OS.extract_step(sd, pts, Bc, G, 64, 64, 0.16 if a.N != 512 else 0.06)
        times.append(time.time() - t0)
    t = float(np.median(times[1:]))
    return {"value": round(Bc / t, 3), "unit": "clips/s", "cores": cores, "kind": "port",
            "sample": f"B={Bc} clips x T={G} views x N={a.N} pts, D={a.D}: 1 warm-up + 3 timed passes "
                      f"(median {t:.2f} s, first {times[0]:.2f} s) of oracle.step.extract_step"}


def make_extract_step(a, dev, rank):
    """bench.py --config extract: (step, eager step, batches, launch mode, workload, dtype, note).  One "step" = the per-batch
    body of extract_motion_feature.py:171-182 on a batch resident in HBM: grouping -> encoder under eval() -> feature layout."""
    import torch
    from facl_amd.cn3d_model_conbag import PointNet_Plus
    from facl_amd.extract_common import extract_batch
    from facl_amd.train_common import synthetic_batch
    opt = make_opt(a)
    net = PointNet_Plus(opt, gost=a.T).to(dev).eval()
    gen = torch.Generator(device=dev)
    gen.manual_seed(rank)
    batches = [synthetic_batch(a.B, a.T, a.N, a.D, dev, gen) for _ in range(2)]

    def eager(batch, epoch=0):
        with torch.no_grad():
            f = extract_batch(net, batch, opt)
        return f.sum(), f, None                          # (the bench reads a scalar back at the end, as for the loss; f: --dump-outputs)
    mode, step = "eager", eager
    if a.graph:
        try:
            static = batches[0].clone()
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                for _ in range(2):
                    eager(static)
            torch.cuda.current_stream().wait_stream(s)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                out = eager(static)

            def step(batch, epoch=0):
                static.copy_(batch, non_blocking=True)
                g.replay()
                return out
            mode = "hipgraph"
        except Exception as e:                            # never lose the measurement to a capture problem
            print("graph capture failed (%s: %s); running eager" % (type(e).__name__, e), file=sys.stderr)
            step = eager
    workload = (f"feature extraction (extract_motion_feature.py:171-182), B={a.B}/GPU T={a.T} N={a.N} D={a.D}, S=64 K=64: kNN/radius "
                f"grouping, cn3d_model_conbag encoder under eval() (net3DV_1 as ONE kernel, csrc/sa_eval.hip), (T+1)*512 features per clip")
    note = ("fp32 storage and accumulation; the dense contractions on the 16-bit MFMAs with every fp32 operand split exactly into two "
            "fp16 pieces of the operand times a power of two taken from its own maximum (fp16x3, DESIGN 3.0)")
    return step, eager, batches, mode, workload, "f32", note


def cpu_baseline_dense(a):
    """Dense configuration: oracle/dense.py (the 3-level encoder restated on torch-CPU ops, fp32) forward + losses +
    backward on a 2-clip sample of the same (T, N, D) shape, 1 warm-up + 1 timed pass.  No optimiser step (the oracle
    of this configuration has none): the CPU figure is therefore slightly favourable to the CPU."""
    import numpy as np
    import torch
    from oracle import dense as OD
    cores = host_cores()
    torch.set_num_threads(cores)
    Bc = 2
    times = OD.time_step(Bc, a.T, a.N, a.D, repeats=2)
    t = float(times[1])
    return {"value": round(Bc / t, 3), "unit": "clips/s", "cores": cores, "kind": "port",
            "sample": f"B={Bc} clips x T={a.T} views x N={a.N} pts, D={a.D}: 1 warm-up + 1 timed pass ({t:.2f} s) of "
                      f"oracle.dense forward + losses + backward (no optimiser step)"}


DUMP_BYTES = 64 << 20            # --dump-outputs: at most this much in all (every config's outputs are < 20 MB at its defaults)


def dump_outputs(path, named, state=None):
    """--dump-outputs: `named` {name: tensor} = what the caller of the timed step receives, `state` = the module state
    the step leaves behind (training configs).  float64 stays float64, everything else is written as float32; integer
    state (num_batches_tracked) as float64."""
    import numpy as np
    import torch
    arrays = {name: t for name, t in named.items() if t is not None}
    arrays.update(("state." + k, v) for k, v in (state or {}).items())
    out, total = {}, 0
    for name, t in arrays.items():
        x = t.detach().cpu()
        x = (x.double() if x.dtype == torch.float64 or not x.is_floating_point() else x.float()).numpy()
        total += x.nbytes
        out[name] = x
    if total > DUMP_BYTES:
        raise RuntimeError("--dump-outputs: %d bytes exceed the %d-byte budget" % (total, DUMP_BYTES))
    os.makedirs(path, exist_ok=True)
    for name, x in out.items():
        np.save(os.path.join(path, name + ".npy"), x)
    print("bench.py: %d arrays (%.1f MB) written to %s" % (len(out), total / 1e6, path), file=sys.stderr)


def main():
    a = parse()
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(spawn_ranks(a))
    import numpy as np
    import torch
    from facl_amd import dist as fdist
    ndev = torch.cuda.device_count()
    # one rank per GPU, bound BEFORE the process group exists (RCCL creates its communicator on the current device);
    # `% device_count` only matters for the gloo rehearsal of N>1 on a single-GPU box
    local = int(os.environ.get("LOCAL_RANK", "0")) % max(ndev, 1)
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    rank, world = fdist.init_from_env()
    if a.rehearse_dp and world == 1:
        import torch.distributed as tdist
        import socket
        with socket.socket() as sk:                          # a port nobody holds (a fixed one can sit in TIME_WAIT after a torchrun)
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        fdist.full_graph_env()
        tdist.init_process_group("nccl", rank=0, world_size=1)
        fdist.is_distributed = lambda: True                 # is_distributed() is world_size > 1: force the hooks on
        import facl_amd.train_common as _tc
        _tc.fdist.is_distributed = fdist.is_distributed
    if world != a.gpus:
        print("bench.py: --gpus %d but WORLD_SIZE=%d" % (a.gpus, world), file=sys.stderr)
        sys.exit(2)
    if world > ndev and os.environ.get("FACL_DIST_BACKEND") != "gloo":
        print("bench.py: %d ranks but only %d device(s) visible" % (world, ndev), file=sys.stderr)
        sys.exit(2)

    torch.manual_seed(1)                       # opt.manualSeed = 1 (cn3d_train_motion_GL.py:142-144)
    np.random.seed(1)
    if a.config == "dense":
        from facl_amd import dense as fdense
        step, eager_step, batches, mode, workload, dtype, dtype_note = fdense.make_bench_step(a, dev, rank, world)
    elif a.config == "extract":
        step, eager_step, batches, mode, workload, dtype, dtype_note = make_extract_step(a, dev, rank)
    else:
        from facl_amd.cn3d_model_conbag import PointNet_Plus
        from facl_amd.train_common import ContrastiveStep, GraphedStep, GraphCaptureFailed, synthetic_batch, appearance_batch
        opt = make_opt(a)
        net = PointNet_Plus(opt, gost=a.T).to(dev).train()
        net.precision = a.precision
        net.bn_reduce_fn = fdist.make_bn_reduce_fn()
        use_graph = bool(a.graph)              # world > 1: the capture is cut at every collective (facl_amd/dist.py: GraphSegments)
        from facl_amd.optim import FusedAdam
        optim = FusedAdam(net.parameters(), lr=0.0003, betas=(0.5, 0.999), eps=1e-06)     # cn3d_train_motion_GL.py:180, one launch
        step = ContrastiveStep(net, optim, opt, a.T, fps_reorder=bool(a.fps))
        eager_step = step
        gen = torch.Generator(device=dev)
        gen.manual_seed(rank)
        make = appearance_batch if a.config == "appearance" else synthetic_batch
        batches = [make(a.B, a.T, a.N, a.D, dev, gen) for _ in range(2)]   # resident in HBM
        mode = "eager"
        if os.environ.get("FACL_BENCH_LAUNCH_NOTE"):        # set by spawn_ranks' second attempt
            mode = "eager (%s)" % os.environ["FACL_BENCH_LAUNCH_NOTE"]
        if use_graph:
            try:
                step = GraphedStep(step, batches[0], a.T)
                mode = ("hipgraph (OPT-IN FACL_DP_GRAPH=full: collectives captured inside the graph; replay validated against one eager step)"
                        if getattr(step, "full_dp_graph", False) else "hipgraph") if step.segments is None else \
                    "hipgraph segments (%d graphs, %d eager collectives between them; replay validated against one eager step)" % (
                        step.segments.n_graphs, len(step.segments.items) - step.segments.n_graphs)
            except GraphCaptureFailed as e:
                # never lose the measurement to a capture problem.  The training state is restored and, under data parallelism,
                # every rank raises this at the same collective (facl_amd/dist.py: GraphSegments votes), so all ranks go eager
                # together; any OTHER exception under world > 1 propagates: the rank exits non-zero and the launcher stops the rest
                print("graph capture failed (%s); running eager" % e, file=sys.stderr)
                mode = "eager (graph capture failed: %s)" % str(e)[:200]
        stream = "motion" if a.config == "motion" else "appearance"
        workload = (f"{stream} stream, B={a.B}/GPU T={a.T} N={a.N} D={a.D}, S=64 K=64, "
                    f"fps-reorder {'on' if a.fps else 'off (the reference loop never calls it: cn3D_data_set.py:285-350)'}, "
                    f"kNN/radius grouping, full cn3d_model_conbag encoder, global+circle loss, backward, Adam")
        dtype = {"f32": "f32", "x3": "bf16x3", "x3b": "f32 (backward GEMMs bf16x3)"}[a.precision]
        dtype_note = ("fp32 storage and accumulation; dense contractions on the 16-bit MFMAs with every fp32 operand split "
                      "exactly: fp16x3 (two fp16 pieces of the operand times a power of two taken from the operand's own maximum / "
                      "bound -- no fixed scale, no range contract since round 4 --, 3 products per multiply-add) in the set-abstraction "
                      "passes and the row-streamed tail GEMMs (forward, dgrad, wgrad), bf16x6 (three bf16 pieces, 6 products) in the "
                      "~800-row FC-head / loss GEMMs; both measure at or below torch's fp32 matmul error against fp64 (DESIGN.md 3.0).  "
                      "Measured parity at this size (tests/test_gpu_headline.py, one full step vs a torch-fp64 evaluation): features "
                      "4.5e-6 / 4.8e-6 (x / x_global, worst row), losses 1e-7, BN running statistics < 1e-5, every parameter gradient "
                      "<= 1.1e-5 of fp64 with the discrete decisions (max-pool argmax, ReLU signs) pinned; the reference's own fp32 run "
                      "sits 4e-5..1.5e-3 from the same fp64 truth (DESIGN.md section 2).  FACL_FWD_H3=0 FACL_BWD_H3=0 select bf16x6 everywhere")
        if a.precision == "x3":
            dtype_note = ("OPT-IN --precision x3 (not the headline): fp32 storage and accumulation; the tail / loss GEMMs and the "
                          "64->256 set-abstraction layer keep two bf16 pieces per operand, three products per multiply-add "
                          "(~1e-5 relative; tests/test_gpu_headline.py holds features and loss to the north_star's 1e-4)")
        elif a.precision == "x3b":
            dtype_note = ("OPT-IN --precision x3b (not the headline): forward, features and loss exactly as the default; the "
                          "dgrad / wgrad GEMMs of the tail and the loss use three bf16 products per multiply-add (~1e-5 relative "
                          "on the gradients)")

    def barrier():
        if world > 1:
            torch.distributed.barrier()
        torch.cuda.synchronize()

    for i in range(a.warmup):
        step(batches[i % 2], epoch=0)
    barrier()
    t0 = time.perf_counter()
    for i in range(a.steps):
        res = step(batches[i % 2], epoch=0)
    barrier()
    dt = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([dt], dtype=torch.float64, device=dev)
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        dt = float(t.item())
    loss = res[0]
    final_loss = float(loss.item())
    if a.dump_outputs and rank == 0:
        # before anything under --full steps the model again: these are the last TIMED step's results
        names = ("feature_sum", "features", None) if a.config == "extract" else ("loss", "loss_c", "loss_circle")
        net = None if a.config == "extract" else eager_step.netR
        dump_outputs(a.dump_outputs, {n: t for n, t in zip(names, res) if n is not None},
                     None if net is None else net.state_dict())

    ms_median_fenced = rl_main = rl_more = None
    if a.full:
        # SURVEY 8(d) asks for the median of fenced steps: the same K steps again, each bracketed by a device synchronise
        # (the value above stays the contract's one-sync-per-K mean; at ~4 ms/step the per-step fence costs ~1 %)
        fenced = []
        for i in range(a.steps):
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            step(batches[i % 2], epoch=0)
            torch.cuda.synchronize()
            fenced.append(time.perf_counter() - t1)
        fenced.sort()
        ms_median_fenced = 1e3 * fenced[len(fenced) // 2]
        # in-step kernel timing: extra eager steps on EVERY rank (they contain the collectives), reported by rank 0
        rl_main, rl_more = step_rooflines(a, eager_step, batches)
    out = None
    if rank == 0:
        clips = a.B * world * a.steps / dt
        out = {"metric": _baseline_metric(), "value": round(clips, 2), "unit": "clips/s",
               "n_gpus": world, "steps": a.steps, "warmup": a.warmup, "ms_per_step": round(dt / a.steps * 1e3, 3)}
        if a.full:
            out["ms_per_step_median_fenced"] = round(ms_median_fenced, 3)
        out.update({
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": dtype, "data": "synthetic",
            "dtype_note": dtype_note,
            "config": {"workload": workload, "global_batch": a.B * world,
                       "parallelism": f"dp{world}" + (" (REHEARSAL: data-parallel code path on a 1-rank RCCL group)" if a.rehearse_dp else ""),
                       "launch": mode,
                       "precision": getattr(a, "precision", "f32")},
            "final_loss": final_loss})
        if a.full:
            out["roofline"], out["roofline_more"] = rl_main, rl_more
        if a.config == "dense":
            out["metric"] = ("dense-config contrastive-step clips/sec (BASELINE configs[4]: N=4096 T=32, 3-level set "
                             "abstraction, fp16 MFMA point-MLP)")
        if a.config == "extract":
            out["metric"] = "feature-extraction clips/sec (B=32,T=24,N=2048), eval-mode encoder (SURVEY 8 f-1: extract_motion_feature.py)"
            out.pop("final_loss", None)
        if a.full and world == 1 and not a.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline_dense(a) if a.config == "dense" else cpu_baseline_extract(a) if a.config == "extract" \
                else cpu_baseline(a)
    if world > 1:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()
    elif a.rehearse_dp:
        torch.distributed.destroy_process_group()
    if rank == 0:
        print(json.dumps(out))


if __name__ == "__main__":
    main()
