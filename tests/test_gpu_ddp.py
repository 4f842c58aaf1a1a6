"""world_size-2 rehearsal of the data-parallel step on ONE GPU (gloo collectives, both ranks on cuda:0):
the sharded step (SyncBN hooks inside the HIP passes, embeddings all-gather, flat gradient all-reduce) must
equal the single-process step at the global batch."""
import os
import sys

import numpy as np
import pytest
import torch

from ranks import ROOT, rank_env, run_ranks
from step_factory import dp_step, make_net, step_opt

pytestmark = pytest.mark.gpu


def _worker(rank, world, port, q, extra_env=None):
    rank_env(rank, world, port, FACL_DIST_BACKEND="gloo", **(extra_env or {}))
    import torch.distributed as dist
    from facl_amd import dist as fdist
    torch.cuda.set_device(0)
    fdist.init_from_env()
    torch.manual_seed(3)
    G, Bl, N, D = 4, 2, 512, 4
    full = torch.rand(Bl * world, G, N, D) - 0.5
    loss, grads, bufs = dp_step(full[rank * Bl:(rank + 1) * Bl], G, rank, world)
    q.put((rank, loss, {k: v.numpy() for k, v in grads.items()}, {k: v.numpy() for k, v in bufs.items()}))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("oneshot", [False, True])
def test_two_ranks_equal_single_process_global_batch(oneshot):
    """oneshot: the SyncBN reductions go through the OPT-IN peer-mailbox kernel (FACL_ONESHOT_SYNCBN=1, csrc/mailbox.hip: both
    ranks open each other's IPC handle on the one GPU) instead of the process group's all-reduce; same bounds."""
    port = 29600 + (os.getpid() % 2000) + (7 if oneshot else 0)
    env = {"FACL_ONESHOT_SYNCBN": "1"} if oneshot else {"FACL_ONESHOT_SYNCBN": "0"}
    res = run_ranks(_worker, 2, port, args=(env,), timeout=300)
    # single process, global batch
    torch.manual_seed(3)
    G, Bl, N, D = 4, 2, 512, 4
    full = torch.rand(Bl * 2, G, N, D) - 0.5
    loss1, grads1, bufs1 = dp_step(full, G, 0, 1)
    loss2 = 0.5 * (res[0][1] + res[1][1])                         # mean of the per-rank (local-mean) losses
    print("loss 1-rank %.6f  2-rank %.6f" % (loss1, loss2))
    assert abs(loss1 - loss2) <= 1e-5 * abs(loss1)
    gmax = max(float(np.linalg.norm(v.numpy())) for v in grads1.values())
    for k, g1 in grads1.items():
        g1 = g1.numpy()
        for r in (0, 1):
            assert k in res[r][2], k                                          # after the averaged all-reduce both ranks agree
            g2 = res[r][2][k]
            assert np.linalg.norm(g2 - g1) <= 2e-4 * max(np.linalg.norm(g1), 1e-2 * gmax) + 1e-6, (k, r)
    for k, b1 in bufs1.items():                                   # SyncBN: running statistics of the GLOBAL batch
        assert np.allclose(res[0][3][k], b1.numpy(), rtol=2e-5, atol=1e-7), k


def _worker_nccl1(rank, world, port, q):
    """Real RCCL backend with a 1-rank group: every collective of facl_amd/dist.py executes (fp64 all-reduce of the BN
    buffers, all-gather + reduce-scatter of the embeddings, flat gradient all-reduce) and must be the identity."""
    rank_env(rank, world, port)
    import torch.distributed as dist
    from facl_amd import dist as fdist
    import facl_amd.train_common as TC
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1)
    fdist.is_distributed = lambda: True                          # is_distributed() is world_size > 1: force the hooks on
    TC.fdist.is_distributed = fdist.is_distributed
    torch.manual_seed(3)
    full = torch.rand(4, 4, 512, 4) - 0.5
    loss, grads, bufs = dp_step(full, 4, 0, 1)
    q.put((loss, {k: v.numpy() for k, v in grads.items()}))
    dist.destroy_process_group()


def test_rccl_backend_one_rank_group_is_identity():
    (loss_d, grads_d), = run_ranks(_worker_nccl1, 1, 29700 + (os.getpid() % 2000), timeout=300)
    torch.manual_seed(3)
    full = torch.rand(4, 4, 512, 4) - 0.5
    loss1, grads1, _ = dp_step(full, 4, 0, 1)
    assert abs(loss1 - loss_d) <= 1e-6 * abs(loss1)
    for k, g1 in grads1.items():
        g1 = g1.numpy()
        assert np.linalg.norm(grads_d[k] - g1) <= 1e-5 * max(np.linalg.norm(g1), 1e-6), k


def _worker_nccl2(rank, world, port, q):
    """One rank per DEVICE on the real RCCL backend: reduce-scatter backward of the embeddings all-gather (rank-major
    (R,G,B_l,C) chunks), fp64 SyncBN all-reduces, asynchronous tail-bucket gradient all-reduce."""
    rank_env(rank, world, port, LOCAL_RANK=str(rank), HSA_ENABLE_IPC_MODE_LEGACY="0")
    os.environ.pop("FACL_DIST_BACKEND", None)
    import torch.distributed as dist
    from facl_amd import dist as fdist
    torch.cuda.set_device(rank)
    fdist.init_from_env()
    assert dist.get_backend() == "nccl" and fdist._use_reduce_scatter(None)
    torch.manual_seed(3)
    G, Bl, N, D = 4, 2, 512, 4
    full = torch.rand(Bl * world, G, N, D) - 0.5
    loss, grads, bufs = dp_step(full[rank * Bl:(rank + 1) * Bl], G, rank, world)
    q.put((rank, loss, {k: v.numpy() for k, v in grads.items()}, {k: v.numpy() for k, v in bufs.items()}))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_on_rccl_equal_single_process_global_batch():
    """The N>1 path on the backend the scaling runs use.  Needs two devices: self-skips on the one-GPU test box (the
    gloo rehearsal above covers the math there)."""
    if torch.cuda.device_count() < 2:
        pytest.skip("needs >= 2 GPUs (RCCL refuses two ranks on one device)")
    port = 29800 + (os.getpid() % 2000)
    res = run_ranks(_worker_nccl2, 2, port, timeout=600)
    torch.manual_seed(3)
    G, Bl, N, D = 4, 2, 512, 4
    full = torch.rand(Bl * 2, G, N, D) - 0.5
    loss1, grads1, bufs1 = dp_step(full, G, 0, 1)
    loss2 = 0.5 * (res[0][1] + res[1][1])
    assert abs(loss1 - loss2) <= 1e-5 * abs(loss1)
    gmax = max(float(np.linalg.norm(v.numpy())) for v in grads1.values())
    for k, g1 in grads1.items():
        g1 = g1.numpy()
        for r in (0, 1):
            g2 = res[r][2][k]
            assert np.linalg.norm(g2 - g1) <= 2e-4 * max(np.linalg.norm(g1), 1e-2 * gmax) + 1e-6, (k, r)
    for k, b1 in bufs1.items():
        assert np.allclose(res[0][3][k], b1.numpy(), rtol=2e-5, atol=1e-7), k


def test_bench_gpus_flag_launches_ranks_or_fails_loudly():
    """`python bench.py --gpus 2` must start two ranks by itself (torch.distributed.run child); with fewer devices than
    ranks it must exit non-zero instead of silently reporting n_gpus = 1 (round-1 defect).  On a one-GPU box the
    2-rank path is then rehearsed on gloo collectives through the same self-launch."""
    import json
    import subprocess
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    env.pop("FACL_DIST_BACKEND", None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--B", "2", "--T", "4",
           "--N", "512", "--full", "--no-cpu-baseline"]
    if torch.cuda.device_count() < 2:
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode != 0 and "device" in r.stderr
        env["FACL_DIST_BACKEND"] = "gloo"
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('{"metric"')][-1])
    assert line["n_gpus"] == 2 and line["config"]["global_batch"] == 4 and line["config"]["parallelism"] == "dp2"
    assert line["value"] > 0 and line["roofline"]["ms_per_launch"] > 0


def _bench_2rank_gloo(extra_env, timeout=600):
    import json
    import subprocess
    import time
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    env.update(FACL_DIST_BACKEND="gloo", FACL_DIST_TIMEOUT_S="60")
    env.update(extra_env)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--B", "2", "--T", "4",
           "--N", "512", "--no-cpu-baseline"]
    t0 = time.time()
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=timeout)
    dt = time.time() - t0
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{"metric"')]
    return r, (json.loads(lines[-1]) if lines else None), dt


def test_capture_failure_on_one_rank_all_ranks_go_eager_together():
    """rank 1's graph-segment capture raises after the 3rd collective.  The ranks must agree on the
    failure (facl_amd/dist.py: GraphSegments votes), restore their training state and finish the measurement TOGETHER on
    eager launches -- inside the first child run, no hang, no mismatched collective."""
    r, line, dt = _bench_2rank_gloo({"FACL_TEST_CAPTURE_FAIL": "1:3"})
    print("returned after %.1f s" % dt)
    assert r.returncode == 0, r.stderr[-3000:]
    assert line["n_gpus"] == 2 and line["value"] > 0
    assert line["config"]["launch"].startswith("eager (graph capture failed"), line["config"]["launch"]
    assert "retrying once" not in r.stderr                        # agreed in-process, the launcher's second attempt was not needed
    assert dt < 90, dt


def test_rank_death_during_capture_launcher_retries_once_on_eager_launches():
    """rank 1 DIES in the middle of the capture (no vote possible).  torch.distributed.run stops the other
    rank (or its 60 s process-group timeout does), `bench.py --gpus 2` starts ONE fresh child tree with --graph 0 and reports
    that line, marked as such."""
    r, line, dt = _bench_2rank_gloo({"FACL_TEST_CAPTURE_EXIT": "1:3"})
    print("returned after %.1f s" % dt)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "retrying once with --graph 0" in r.stderr
    assert line["n_gpus"] == 2 and line["value"] > 0
    assert line["config"]["launch"].startswith("eager (graph-segment run failed"), line["config"]["launch"]
    assert dt < 150, dt


def _run_graphed_vs_eager(clip, G):
    """Two identical models: one stepped eagerly, one through GraphedStep (segmented capture under data parallelism); three
    optimizer steps each on the same clips; returns (eager losses, graph losses, max relative parameter difference,
    number of graph segments, number of eager collectives between them)."""
    from facl_amd import dist as fdist
    from facl_amd.optim import FusedAdam
    from facl_amd.train_common import ContrastiveStep, GraphedStep
    B, _, N, D = clip.shape
    opt = step_opt(D, B, N)
    order = np.array([2, 0, 3, 1])
    clips = [clip.cuda(), (clip * 0.9).cuda(), (clip * 1.1).cuda()]
    nets, losses = [], []
    for graphed in (False, True):
        net = make_net(D, G, opt=opt, device="cuda").train()
        net.bn_reduce_fn = fdist.make_bn_reduce_fn()
        step = ContrastiveStep(net, FusedAdam(net.parameters(), lr=3e-4, betas=(0.5, 0.999), eps=1e-6), opt, G)
        seg = None
        if graphed:
            sd = {k: v.clone() for k, v in net.state_dict().items()}
            step = GraphedStep(step, clips[0], G)        # 3 warm-up optimizer steps inside: restore the start state
            seg = step.segments
            net.load_state_dict(sd)
            o = step.step.optimizer
            o._step.zero_()
            for st in o.state.values():
                st["exp_avg"].zero_()
                st["exp_avg_sq"].zero_()
        ls = []
        for c in clips:
            loss, _, _ = step(c, epoch=0, order=order)
            ls.append(float(loss.item()))
        nets.append(net)
        losses.append(ls)
    worst = 0.0
    for (k, a), (_, b) in zip(nets[0].named_parameters(), nets[1].named_parameters()):
        worst = max(worst, float((a - b).norm() / a.norm().clamp_min(1e-12)))
    return losses[0], losses[1], worst, seg.n_graphs, len(seg.items) - seg.n_graphs


def _worker_graph(rank, world, port, q, backend):
    rank_env(rank, world, port)
    import torch.distributed as dist
    from facl_amd import dist as fdist
    import facl_amd.train_common as TC
    torch.cuda.set_device(0)
    if backend == "gloo":
        os.environ["FACL_DIST_BACKEND"] = "gloo"
        fdist.init_from_env()
    else:
        dist.init_process_group("nccl", rank=0, world_size=1)
        fdist.is_distributed = lambda: True                      # force every collective on with a 1-rank RCCL group
        TC.fdist.is_distributed = fdist.is_distributed
    torch.manual_seed(3)
    G, Bl, N, D = 4, 2, 512, 4
    full = torch.rand(Bl * world, G, N, D) - 0.5
    try:
        res = _run_graphed_vs_eager(full[rank * Bl:(rank + 1) * Bl], G)
    except BaseException:                                        # fail fast in the parent instead of a queue timeout
        import traceback
        q.put((rank, "error", traceback.format_exc()))
        os._exit(1)
    q.put((rank,) + res)
    if world > 1:
        dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("backend,world", [("gloo", 2), ("nccl", 1)])
def test_segmented_graph_step_equals_eager_step_under_data_parallelism(backend, world):
    """GraphedStep under data parallelism: the capture is cut at every collective (SyncBN all-reduces, embeddings all-gather
    and its backward, the asynchronous tail bucket and the late bucket of the gradient average); kernel segments replay as
    HIP graphs, the collectives run eagerly between them.  Three optimizer steps (FusedAdam) must give the eager step's
    losses and parameters -- on 2 gloo ranks sharing the GPU, and on the real RCCL backend with a forced 1-rank group (every
    RCCL call executes between graph replays, as it will with N > 1)."""
    port = 29900 + (os.getpid() % 2000)
    res = run_ranks(_worker_graph, world, port, args=(backend,), timeout=240)
    for r in res:
        assert r[1] != "error", r[2]
    for rank, l_eager, l_graph, worst, n_graphs, n_coll in res:
        print(f"rank {rank}: eager {l_eager} graph {l_graph} worst param diff {worst:.2e}; {n_graphs} graphs, {n_coll} collectives")
        assert n_coll >= 16 and n_graphs == n_coll + 1
        for a, b in zip(l_eager, l_graph):
            assert abs(a - b) <= 1e-5 * abs(a), (l_eager, l_graph)
        assert worst < 1e-4


def _worker_full_graph(rank, world, port, q):
    rank_env(rank, world, port, FACL_DP_GRAPH="full")
    import torch.distributed as dist
    from facl_amd import dist as fdist
    import facl_amd.train_common as TC
    from facl_amd.optim import FusedAdam
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1)
    fdist.is_distributed = lambda: True                          # force every collective on with a 1-rank RCCL group
    TC.fdist.is_distributed = fdist.is_distributed
    try:
        torch.manual_seed(3)
        G, B, N, D = 4, 2, 512, 4
        clips = [(torch.rand(B, G, N, D) - 0.5).cuda() for _ in range(3)]
        order = np.array([2, 0, 3, 1])
        out = []
        for graphed in (False, True):
            net = make_net(D, G, opt=step_opt(D, B, N), device="cuda").train()
            net.bn_reduce_fn = fdist.make_bn_reduce_fn()
            step = TC.ContrastiveStep(net, FusedAdam(net.parameters(), lr=3e-4, betas=(0.5, 0.999), eps=1e-6), step_opt(D, B, N), G)
            if graphed:
                step = TC.GraphedStep(step, clips[0], G, restore=True)
                assert step.segments is None and step.full_dp_graph
            out.append([float(step(c, epoch=0, order=order)[0].item()) for c in clips])
        q.put(("ok", out))
    except BaseException:
        import traceback
        q.put(("error", traceback.format_exc()))
    dist.destroy_process_group()


def test_optin_full_graph_capture_of_the_data_parallel_step():
    """FACL_DP_GRAPH=full (opt-in, never the default): the data-parallel step with its 19 collectives captured INSIDE one HIP
    graph (torch's RCCL process group joins the stream capture) -- no cut, no eager collective.  On the real RCCL backend with
    a forced 1-rank group: three optimizer steps equal the eager sharded step (GraphedStep validated the replay against one
    eager step before handing it out)."""
    (status, payload), = run_ranks(_worker_full_graph, 1, 30100 + (os.getpid() % 2000), timeout=300)
    assert status == "ok", payload
    eager, graph = payload
    print("eager", eager, "full graph", graph)
    for a, b in zip(eager, graph):
        assert abs(a - b) <= 1e-5 * abs(a)


def _worker_mailbox(rank, world, port, q):
    rank_env(rank, world, port)
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from facl_amd.mailbox import OneShotAllReduce
    ar = OneShotAllReduce(None, n_max=4608)

    def vals(r, it, n):                                     # magnitudes over five decades: the ORDER of the additions matters
        g = torch.Generator().manual_seed(1000 * it + r)
        return torch.randn(n, generator=g, dtype=torch.float64) * (10.0 ** (it % 5 - 2))

    def expect(it, n):
        ref = torch.zeros(n, dtype=torch.float64)
        for r in range(world):
            ref = ref + vals(r, it, n)                      # rank order
        return ref
    ok = True
    for it, n in enumerate([128, 2048, 4608, 1, 512] * 6):  # 30 calls: both slot parities, every size class
        t = vals(rank, it, n).cuda()
        ar(t)
        ok = ok and torch.equal(t.cpu(), expect(it, n))
    # the same kernel inside a captured graph, replayed with fresh inputs: the sequence number lives on the device
    a, b = (torch.zeros(n, dtype=torch.float64, device="cuda") for n in (128, 2048))
    s_ = torch.cuda.Stream()
    s_.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s_):
        ar(a); ar(b)
    torch.cuda.current_stream().wait_stream(s_)
    torch.cuda.synchronize(); dist.barrier()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ar(a); ar(b)
    for rep in range(4):
        for j, t in enumerate((a, b)):
            t.copy_(vals(rank, 100 + 10 * rep + j, t.numel()).cuda())
        torch.cuda.synchronize(); dist.barrier()
        g.replay()
        torch.cuda.synchronize()
        for j, t in enumerate((a, b)):
            ok = ok and torch.equal(t.cpu(), expect(100 + 10 * rep + j, t.numel()))
    ar.check()
    q.put((rank, bool(ok)))
    dist.barrier()
    ar.close()
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 4])
def test_oneshot_mailbox_allreduce_equals_rank_ordered_sum(world):
    """facl_mailbox_allreduce with `world` processes sharing the one GPU, each opening the others' IPC
    handles exactly as peers on other devices would: 30 eager calls (sizes 1 .. 4608 doubles, values over five decades) and a
    captured graph replayed four times must equal the sum in RANK ORDER bit for bit on every rank; no time-out was raised.
    What this cannot show is cross-device visibility over xGMI: the path stays opt-in."""
    port = 31000 + (os.getpid() % 2000) + world
    res = run_ranks(_worker_mailbox, world, port, timeout=240, check_exit=True)
    assert res == [(r, True) for r in range(world)], res
