"""Consecutive training steps, eager and graph-replayed, against a plain torch-fp64 evaluation of the reference's step from
the state the kernels actually left behind.  The one-step parity tests (test_gpu_headline.py, test_gpu_encoder.py) start
from fresh memory; what carries over between steps does not: the fp16x3 operand-scale words raised with atomics,
Adam's device-resident step and lr, the BatchNorm running buffers and the
host-side num_batches_tracked, and whatever a graph replay reuses.  The four steps of SCHEDULE are chosen so that state
left over from the previous step is wrong for the next one: the input scale drops 4x, then rises 16x, the learning rate
changes twice and the circle-loss order changes.  The whole module runs on NaN-poisoned scratch."""
import io

import numpy as np
import pytest
import torch

from helpers import FUSED_ADAM_BETAS, PRE_BN_BIAS, SA_T_BN, adam64, forward64, max_rel_rows, reference_step64, rel_err, routing_taps, snapshot
from poison import poisoned_scratch  # noqa: F401
from step_factory import grouped, make_contrastive_step, points

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-4              # features / losses / gradients: the one-step bounds of the suite
STAT_TOL = 1e-5         # running statistics
ADAM_TOL = 2e-6         # Adam on the kernel's own gradients: test_gpu_tail.py::test_fused_adam_equals_torch_adam
S = K = 64

CONFIGS = {
    # --synthetic 0: view-major (10*B, 512, 4) rows as DiskBatches delivers them; SAMPLE_NUM 512 -> group_points_3DV (r^2 0.06)
    "ref_default": dict(B=32, G=10, N=512, D=4, view_major=True),
    # N not a power of two, tiny batch (the tail below the row-streamed size), knn_radius_group(..., 0.16)
    "ragged": dict(B=3, G=5, N=1000, D=3, view_major=False),
    # what bench.py times
    "headline": dict(B=32, G=24, N=2048, D=3, view_major=False),
}
# (input scale, lr, order): step 1 drops the input-scaled operand maxima 4x below step 0's, step 2 raises them 16x above
# step 1's.  2^-2 / 2^2 is the widest power of two at which the step stays well conditioned; measured with plain torch fp32
# (same routing) against fp64 on the MI355X: 2^-6 -- features 4.7e-5 (ragged), ReLU decisions flipped 2.3e-5 from zero;
# 2^-4 -- gradients 1.9e-4 (ragged); 2^-3 -- gradients 9e-5..1.1e-4 (ragged, every tensor in front of netR_FC.1 alike), at
# the bound itself; 2^6 -- features 1.5e-4, gradients 2.6e-2 (ref_default) .. 1.3e-1 (ragged).  At 2^-2 / 2^2 the worst
# torch-fp32 errors are 2.3e-5 on features and 8.5e-5 on the ragged gradients (the kernels: 4.2e-5 there).
SCHEDULE = [(1.0, 3e-4, 0), (2.0 ** -2, 3e-4, 1), (2.0 ** 2, 1e-3, 2), (1.0, 3e-5, 0)]


def _make(c):
    """Model with the formula weights + FusedAdam (the optimizer of the training entries) + ContrastiveStep."""
    return make_contrastive_step(c, lr=SCHEDULE[0][1])


def _schedule(c):
    """[(points, lr, order)] of the four steps: new clouds every step, permutations A, B, C, A."""
    r = np.random.RandomState(7)
    perms = [r.permutation(c["G"]) for _ in range(3)]
    assert len({tuple(p) for p in perms}) == 3
    return [(points(c, 100 + k, sc), lr, perms[o]) for k, (sc, lr, o) in enumerate(SCHEDULE)]


def _state(net, optim, out):
    """Everything one step produces, cloned: losses, every p.grad, parameters + running buffers + num_batches_tracked
    (state_dict), Adam moments and step."""
    torch.cuda.synchronize()
    st = {"loss." + n: t.detach().clone() for n, t in zip(("loss", "loss_c", "loss_circle"), out)}
    for n, p in net.named_parameters():
        st["grad." + n] = None if p.grad is None else p.grad.detach().clone()
    for k, v in net.state_dict().items():
        st["sd." + k] = v.detach().clone()
    names = {id(p): n for n, p in net.named_parameters()}
    osd = optim.state_dict()
    for i, p in enumerate(optim.param_groups[0]["params"]):
        for k, v in osd["state"][i].items():
            st["adam.%s.%s" % (names[id(p)], k)] = v.detach().clone()
    return st


def _bitwise_diff(a, b):
    """Keys whose tensors are not bit-identical (NaN never is), with the largest difference."""
    assert a.keys() == b.keys()
    bad = []
    for k in a:
        x, y = a[k], b[k]
        if x is None or y is None:
            if (x is None) != (y is None):
                bad.append((k, "None on one side"))
        elif x.shape != y.shape or x.dtype != y.dtype or not torch.equal(x, y):
            bad.append((k, float((x.double() - y.double()).abs().max()) if x.shape == y.shape else "shape"))
    return bad


def _check_counters(after, before):
    """num_batches_tracked: +1 per step, +2 for netR_FC.1 (two BatchNorm calls per step)."""
    for key in SA_T_BN + ("netR_FC.1",):
        k = key + ".num_batches_tracked"
        got, want = int(after["net"][k]), int(before["net"][k]) + (2 if key == "netR_FC.1" else 1)
        assert got == want, (k, got, want)


def _check_running(after, ref, tag):
    errs = []
    for key, (rm, rv) in ref["running"].items():
        e = max(rel_err(after["net"][f"{key}.running_mean"].numpy(), rm.cpu().numpy()),
                rel_err(after["net"][f"{key}.running_var"].numpy(), rv.cpu().numpy()))
        assert e < STAT_TOL, (tag, key, e)
        errs.append(e)
    return max(errs)


# ---- the per-step comparison with fp64 (tests A and B) -------------------------------------------------------------------
HEADER = ("step  scale    lr     | x        xg       loss_c   loss_cir  grad     | torch-fp32: x        xg       loss_c   "
          "loss_cir  grad     | stats    adam(k)  ties")


def _step_vs_fp64(c, tag, before, after, pts, order, routing, x, xg, losses, grads, params):
    """One step against reference_step64(before): features (1e-4 per row), losses (1e-4), every gradient (1e-4 of its
    norm, floor 1e-2 of the largest; routed through the kernel's decisions, each differing decision a tie), running
    statistics (1e-5), num_batches_tracked (+1, +2 for netR_FC.1), Adam -- fp64 torch.optim.Adam on the kernel's own
    gradients (2e-6 of max |.|: parameters and both moments) and on the fp64 gradients (the moments within (1 - beta) x the
    gradient bound); the moments with the betas FusedAdam holds, FUSED_ADAM_BETAS -- and the optimizer's step count.
    Prints one row of the error table, torch fp32 beside the kernels."""
    B, G = c["B"], c["G"]
    k = tag[-1]
    b1, b2 = FUSED_ADAM_BETAS
    x_rows, centers = grouped(c, pts)
    ref = reference_step64(before, x_rows, centers, G, B, S, K, order, routing, betas=FUSED_ADAM_BETAS)
    loss, loss_c, loss_circle = (float(v.detach()) for v in losses)
    rl = lambda a, b: abs(a - b) / abs(b)
    e_x, e_xg = (max_rel_rows(a.cpu().numpy(), ref[n].cpu().numpy()) for a, n in ((x, "x"), (xg, "xg")))
    e_x32, e_xg32 = (max_rel_rows(ref[n + "32"].cpu().numpy(), ref[n].cpu().numpy()) for n in ("x", "xg"))
    e_lc, e_lo = rl(loss_c, ref["loss_c"]), rl(loss_circle, ref["loss_circle"])
    e_lc32, e_lo32 = rl(ref["loss_c32"], ref["loss_c"]), rl(ref["loss_circle32"], ref["loss_circle"])
    g64 = ref["g64"]
    ties = max(v for n, v in ref["ties"].items() if not n.endswith("_flips"))
    gmax = max(float(g64[n].norm()) for n in grads)
    e_g = e_g32 = 0.0
    bad = []
    for n, mine in grads.items():
        r = g64[n].reshape(mine.shape)
        den = max(float(r.norm()), 1e-2 * gmax)
        err, e32 = float((mine.double() - r).norm()) / den, float((ref["g32"][n].reshape(mine.shape) - r).norm()) / den
        e_g, e_g32 = max(e_g, err), max(e_g32, e32)
        if not err <= TOL:
            bad.append((n, err, e32))
    # fp64 Adam on the kernel's own gradients (isolates the optimizer): the parameters against torch.optim.Adam with the
    # reference's betas, the moments against the betas FusedAdam holds (fp32: FUSED_ADAM_BETAS)
    ak, akf = adam64(before, grads), adam64(before, grads, FUSED_ADAM_BETAS)
    e_ad, bad_adam = 0.0, []
    for n, (p64, _, _) in ak.items():
        _, m64, v64 = akf[n]
        for what, got, want in (("param", params[n], p64), ("exp_avg", after["adam"][n]["exp_avg"], m64),
                                ("exp_avg_sq", after["adam"][n]["exp_avg_sq"], v64)):
            d = float((got.to(DEV).double().reshape(want.shape) - want).abs().max()) / max(float(want.abs().max()), 1e-30)
            e_ad = max(e_ad, d)
            if not d <= ADAM_TOL:
                bad_adam.append((n, what, d))
    e_st = max(max(rel_err(after["net"][f"{key}.running_mean"].numpy(), rm.cpu().numpy()),
                   rel_err(after["net"][f"{key}.running_var"].numpy(), rv.cpu().numpy())) for key, (rm, rv) in ref["running"].items())
    print(f"[{tag[0]}] {k}     {SCHEDULE[k][0]:<8g} {SCHEDULE[k][1]:<6g} | {e_x:.2e} {e_xg:.2e} {e_lc:.2e} {e_lo:.2e}  {e_g:.2e} |"
          f"             {e_x32:.2e} {e_xg32:.2e} {e_lc32:.2e} {e_lo32:.2e}  {e_g32:.2e} | {e_st:.2e} {e_ad:.2e} {ties:.1e}")

    assert e_x < TOL and e_xg < TOL, (tag, e_x, e_xg)
    assert e_lc < TOL and e_lo < TOL, (tag, e_lc, e_lo)
    assert rl(loss, ref["loss_c"] + ref["loss_circle"]) < TOL, tag
    assert ties < 1e-5, (tag, {n: v for n, v in ref["ties"].items() if not n.endswith("_flips") and v >= 1e-6})
    assert set(grads) == set(g64) - PRE_BN_BIAS, (tag, sorted(set(grads) ^ (set(g64) - PRE_BN_BIAS)))
    assert not bad, (tag, bad)
    assert e_st < STAT_TOL, (tag, e_st)
    _check_counters(after, before)
    assert not bad_adam, (tag, bad_adam)
    for n in set(params) - set(grads):                     # no gradient (the pre-BN biases, mapping.weight): no update
        assert n in PRE_BN_BIAS | {"mapping.weight"} and torch.equal(after["net"][n], before["net"][n]), (tag, n)
    for n in grads:                                        # fp64 Adam on the fp64 gradients: the moments
        _, m64, v64 = ref["adam64"][n]
        m, v = (after["adam"][n][s_].to(DEV).double().reshape(m64.shape) for s_ in ("exp_avg", "exp_avg_sq"))
        tg = TOL * max(float(g64[n].norm()), 1e-2 * gmax)
        assert float((m - m64).norm()) <= (1 - b1) * tg + 1e-6 * float(m64.norm()), (tag, n)
        gm = float(g64[n].abs().max())
        assert float((v - v64).norm()) <= (1 - b2) * tg * (2 * gm + tg) + 1e-6 * float(v64.norm()), (tag, n)
    assert after["step"] == k + 1, (tag, after["step"])
    assert after["lr"] == SCHEDULE[k][1], tag


# ---- A -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", ["ref_default", "ragged"])
def test_consecutive_eager_steps_vs_fp64(cfg):
    """Four eager ContrastiveStep + FusedAdam steps of one model; after each, everything the step produced against
    reference_step64 from the snapshot taken before it (_step_vs_fp64).  Measured on the MI355X: the printed table."""
    c = CONFIGS[cfg]
    net, optim, step = _make(c)
    print(f"\n[{cfg}] " + HEADER)
    for k, (pts, lr, order) in enumerate(_schedule(c)):
        optim.param_groups[0]["lr"] = lr
        before = snapshot(net, optim)
        taps = {}
        h = net.register_forward_hook(lambda m, i, o: taps.update(x=o[0].detach().clone(), xg=o[3].detach().clone()))
        with routing_taps() as routing:
            losses = step(pts, epoch=0, order=order)
        h.remove()
        torch.cuda.synchronize()
        grads = {n: p.grad.detach().clone() for n, p in net.named_parameters() if p.grad is not None}
        params = {n: p.detach().clone() for n, p in net.named_parameters()}
        assert float(optim._step[0]) == k + 1
        _step_vs_fp64(c, (cfg, k), before, snapshot(net, optim), pts, order, routing, taps["x"], taps["xg"], losses, grads, params)


# ---- B -------------------------------------------------------------------------------------------------------------------
def _assert_same_state(a, b, what):
    for part in ("net", "adam"):
        for k in a[part]:
            x, y = a[part][k], b[part][k]
            if isinstance(x, dict):
                for kk in x:
                    assert torch.equal(x[kk], y[kk]), (what, part, k, kk)
            else:
                assert torch.equal(x, y), (what, part, k)
    assert a["step"] == b["step"] and a["lr"] == b["lr"], what


def _graph_vs_eager_twin(c, tag, check=None):
    """Capture GraphedStep(restore=True) under poison, then the four steps of the schedule: snapshot, replay, the same step
    eagerly on a twin loaded from the snapshot, bitwise comparison.  `check(k, before, after, replayed, pts, order, net_g,
    routing)`: per-step checks of the replay against fp64 (routing: the twin's max-pool / ReLU decisions)."""
    from facl_amd.train_common import GraphedStep
    net_g, opt_g, step_g = _make(c)
    snap0 = snapshot(net_g, opt_g)
    g = GraphedStep(step_g, points(c, 99), c["G"], restore=True)
    torch.cuda.synchronize()
    _assert_same_state(snapshot(net_g, opt_g), snap0, (tag, "restore=True"))      # the three warm-up steps undone
    net_t, opt_t, step_t = _make(c)
    for k, (pts, lr, order) in enumerate(_schedule(c)):
        opt_g.param_groups[0]["lr"] = lr
        before = snapshot(net_g, opt_g)
        rg = _state(net_g, opt_g, g(pts, order=order))                           # p.grad: graph-pool tensors, rewritten by each replay
        net_t.load_state_dict(before["net"])
        opt_t.load_state_dict(before["optim"])
        with routing_taps() as routing:
            rt = _state(net_t, opt_t, step_t(pts, order=order))
        bad = _bitwise_diff(rg, rt)
        assert not bad, (tag, k, bad)
        assert all(torch.isfinite(v).all() for v in rg.values() if v is not None and v.is_floating_point()), (tag, k)
        after = snapshot(net_g, opt_g)
        _check_counters(after, before)
        assert after["step"] == k + 1, (tag, k, after["step"])
        if check is not None:
            check(k, before, after, rg, pts, order, net_g, routing)
    return net_g, opt_g


@pytest.mark.parametrize("cfg", ["ref_default", "ragged"])
def test_graph_replay_steps_equal_eager_steps_bitwise(cfg):
    """Every replay of the captured step == one eager step from the same state, bit for bit: losses, every p.grad,
    parameters, running buffers, num_batches_tracked, Adam moments and step.  Both run the same kernels in the same order
    and the step has no float atomics (csrc/ has no atomicAdd at all; reductions sum in a fixed slice order),
    so nothing may differ.  Every replay is also held to fp64 like test A (_step_vs_fp64): a defect shared by the graph and
    the eager path does not pass."""
    c = CONFIGS[cfg]
    M = c["G"] * c["B"]
    print(f"\n[{cfg} graph] " + HEADER)

    def check(k, before, after, rg, pts, order, net_g, routing):
        stacked = net_g._stacked.detach()                  # the replay's (M + B, 512) embeddings (graph pool)
        grads = {n[5:]: v for n, v in rg.items() if n.startswith("grad.") and v is not None}
        params = {n: rg["sd." + n] for n, _ in net_g.named_parameters()}
        losses = (rg["loss.loss"], rg["loss.loss_c"], rg["loss.loss_circle"])
        _step_vs_fp64(c, (cfg + " graph", k), before, after, pts, order, routing, stacked[:M], stacked[M:], losses, grads, params)

    _graph_vs_eager_twin(c, cfg, check)


# ---- C -------------------------------------------------------------------------------------------------------------------
def test_graph_replay_at_headline_size():
    """The schedule of test B at the size bench.py times (graph mode only; the one-step fp64 gradient check at this size is
    test_gpu_headline.py): bit-identity with the eager twin, features and losses of every replay within 1e-4 of a forward64
    evaluation of the snapshot, running statistics and num_batches_tracked following the schedule."""
    from oracle import loss as OL
    c = CONFIGS["headline"]
    B, G = c["B"], c["G"]
    M = G * B
    print("\n[headline] step  scale    lr     | x        xg       loss_c   loss_cir | torch-fp32: x        xg       loss_c   "
          "loss_cir | stats")

    def check(k, before, after, rg, pts, order, net_g, routing):
        stacked = net_g._stacked.detach()                  # the replay's (M + B, 512) embeddings (graph pool)
        x_rows, centers = grouped(c, pts)
        ref = reference_step64(before, x_rows, centers, G, B, S, K, order, None, backward=False)
        e_x = max_rel_rows(stacked[:M].cpu().numpy(), ref["x"].cpu().numpy())
        e_xg = max_rel_rows(stacked[M:].cpu().numpy(), ref["xg"].cpu().numpy())
        lc, lo = float(rg["loss.loss_c"]), float(rg["loss.loss_circle"])
        e_lc, e_lo = abs(lc - ref["loss_c"]) / abs(ref["loss_c"]), abs(lo - ref["loss_circle"]) / abs(ref["loss_circle"])
        with torch.no_grad():                              # plain torch fp32 of the same forward: the conditioning yardstick
            x32, xg32, _, _, _ = forward64(x_rows, centers, before["net"], G, S, K, DEV, dtype=torch.float32)
            e32 = (max_rel_rows(x32.cpu().numpy(), ref["x"].cpu().numpy()), max_rel_rows(xg32.cpu().numpy(), ref["xg"].cpu().numpy()),
                   abs(float(OL.global_contrast(G, xg32, x32, B)) - ref["loss_c"]) / abs(ref["loss_c"]),
                   abs(float(OL.circle_contrast(G, x32, B, order)) - ref["loss_circle"]) / abs(ref["loss_circle"]))
        del x32, xg32
        e_st = _check_running(after, ref, ("headline", k))
        print(f"[headline] {k}     {SCHEDULE[k][0]:<8g} {SCHEDULE[k][1]:<6g} | {e_x:.2e} {e_xg:.2e} {e_lc:.2e} {e_lo:.2e} |"
              "             %.2e %.2e %.2e %.2e | %.2e" % (*e32, e_st))
        assert e_x < TOL and e_xg < TOL, (k, e_x, e_xg)
        assert e_lc < TOL and e_lo < TOL, (k, e_lc, e_lo)

    _graph_vs_eager_twin(c, "headline", check)


# ---- D -------------------------------------------------------------------------------------------------------------------
def test_resume_from_state_dicts_continues_the_trajectory():
    """Two graph replays, then net.state_dict() + optimizer.state_dict() through torch.save / torch.load into a fresh
    model and FusedAdam: the third step of the schedule taken eagerly on the fresh pair equals the graph's third replay bit
    for bit (the device-resident Adam step and lr survive the round trip)."""
    from facl_amd.train_common import GraphedStep
    c = CONFIGS["ref_default"]
    net_g, opt_g, step_g = _make(c)
    g = GraphedStep(step_g, points(c, 99), c["G"], restore=True)
    sched = _schedule(c)
    for pts, lr, order in sched[:2]:
        opt_g.param_groups[0]["lr"] = lr
        g(pts, order=order)
    torch.cuda.synchronize()
    buf = io.BytesIO()
    torch.save({"net": net_g.state_dict(), "optim": opt_g.state_dict()}, buf)
    buf.seek(0)
    ck = torch.load(buf, map_location="cpu")
    net_r, opt_r, step_r = _make(c)
    net_r.load_state_dict(ck["net"])
    opt_r.load_state_dict(ck["optim"])
    assert float(opt_r._step[0]) == 2 and opt_r.param_groups[0]["lr"] == sched[1][1]
    pts, lr, order = sched[2]
    opt_g.param_groups[0]["lr"] = opt_r.param_groups[0]["lr"] = lr
    rg = _state(net_g, opt_g, g(pts, order=order))
    rr = _state(net_r, opt_r, step_r(pts, order=order))
    bad = _bitwise_diff(rg, rr)
    assert not bad, bad
    assert int(rg["adam.net3DV_1.0.weight.step"]) == 3
