"""GPU tests of the optimizer recipe (FusedAdam's weight_decay / max_grad_norm / schedule): the kernels
facl_grad_sqnorm, facl_adam_prep_ex and facl_adamw_apply on guard-banded tensors against fp64, the ABI refusals beside a device,
the training step (eager and graph-replayed), the default path against the direct facl_adam_prep / facl_adam_apply sequence, and
the entries.  The kernel cases are those of chunk_cases.py, the step runs at test_gpu_key_encoder.py's `ragged` size and mode.  The whole
module runs on NaN-poisoned scratch."""
import contextlib
import os
import re

import numpy as np
import pytest
import torch

from chunk_cases import CHUNK, DEV, _banded, _bands_intact, _case, _chunks, _ints, _ptrs
from helpers import FUSED_ADAM_BETAS, snapshot
from step_factory import make_contrastive_step, points
from synth_tree import assert_same_state, run_train_entry
from poison import poisoned_scratch  # noqa: F401

pytestmark = pytest.mark.gpu
ADAM_TOL = 2e-6                      # test_gpu_trajectory.py / test_gpu_tail.py: Adam on given gradients, of max |.| per tensor
NORM_TOL = 2.0 ** -22                # the gradient norm: see test_grad_sqnorm_and_prep_ex
B1, B2 = 0.5, 0.999
f32 = lambda x: float(np.float32(x))
LR, EPS, WD = f32(1e-3), f32(1e-6), f32(0.05)             # what the kernels hold: fp32 launch constants and an fp32 device lr


def _norm64(gs):
    return float(torch.sqrt(sum((g.double() ** 2).sum() for g in gs)))


def _inputs(nt, steps=3):
    """Parameters of unit scale and `steps` gradient sets of scale 0.05: the global norm is then ~7 (nt = 14) / ~11 (nt = 64),
    small enough that max_norm / (norm + 1e-6) at max_norm == norm lies more than half an fp32 ulp below 1."""
    gen = torch.Generator(device=DEV)
    gen.manual_seed(nt)
    case = _case(nt)
    assert len(case) == nt
    p0 = [torch.randn(n, device=DEV, generator=gen) for n, _ in case]
    gs = [[0.05 * torch.randn(n, device=DEV, generator=gen) for n, _ in case] for _ in range(steps)]
    return case, p0, gs


# ---- 5: facl_grad_sqnorm + facl_adam_prep_ex ---------------------------------------------------------------------------------
@pytest.mark.parametrize("nt", [14, 64])
def test_grad_sqnorm_and_prep_ex(nt):
    """The norm against sqrt(sum g^2) in fp64.  Bound (derived, not measured): the squares are exact in fp64; the fp64 sum of n
    non-negative terms, in any order, errs by at most n 2^-53 relative (n <= 5e4 here: 6e-12), the square root halves it; the
    one rounding to fp32 is 2^-24.  Asserted: relative error <= 2^-22.  The clip coefficient at max_norm = 0.5 x, 2 x and 1 x
    the fp64 norm; two launches give the same partial sums bit for bit; the gradients and every guard band stay as they were."""
    from facl_amd import _lib
    lib = _lib.load_library()
    st = _lib.stream()
    case, _, gs = _inputs(nt, steps=1)
    G = [_banded(g, s) for g, (_, s) in zip(gs[0], case)]
    g_before = [b.clone() for b, _ in G]
    nc = _chunks(case)
    n64 = _norm64([d for _, d in G])
    N = _ints([n for n, _ in case])
    parts = []
    for _ in range(2):
        pbuf, part = _banded(torch.full((nc,), float("nan"), dtype=torch.float64), 0, torch.float64)
        _lib.check(lib.facl_grad_sqnorm(nt, _ptrs([d for _, d in G]), N, part.data_ptr(), st), "facl_grad_sqnorm")
        torch.cuda.synchronize()
        assert _bands_intact(pbuf, 0, nc) and torch.isfinite(part).all()
        parts.append(part)
    assert torch.equal(parts[0].view(torch.int64), parts[1].view(torch.int64))
    # every partial is the sum of its own chunk
    c = 0
    for (n, _), (_, d) in zip(case, G):
        for lo in range(0, n, CHUNK):
            want = float((d[lo:lo + CHUNK].double() ** 2).sum())
            assert abs(float(parts[0][c]) - want) <= 2 * CHUNK * 2.0 ** -53 * want, (n, lo)      # either sum's n 2^-53
            c += 1
    assert c == nc
    lr = torch.full((1,), LR, device=DEV)
    cbuf0, consts0 = _banded(torch.zeros(2), 0)
    _lib.check(lib.facl_adam_prep(lr.data_ptr(), torch.zeros(1, device=DEV).data_ptr(), B1, B2, consts0.data_ptr(), st), "facl_adam_prep")
    seen = {}
    for factor in (0.5, 2.0, 1.0, None):                     # None: no clipping, no partials
        step = torch.zeros(1, device=DEV)
        cbuf, consts = _banded(torch.full((5,), float("nan")), 0)
        _lib.check(lib.facl_adam_prep_ex(lr.data_ptr(), step.data_ptr(), B1, B2, parts[0].data_ptr() if factor else None,
                                         nc if factor else 0, factor * n64 if factor else 0.0, 0, 0, 0, 0.0, consts.data_ptr(), st),
                   "facl_adam_prep_ex")
        torch.cuda.synchronize()
        assert _bands_intact(cbuf, 0, 5) and float(step) == 1.0
        assert torch.equal(consts[:2].view(torch.int32), consts0.view(torch.int32))     # facl_adam_prep's two constants
        assert float(consts[2]) == LR
        seen[factor] = (float(consts[3]), float(consts[4]))
    print("nt=%d: norm fp64 %.9g, kernel %.9g (rel %.2e), c at 0.5x / 2x / 1x: %r %r %r"
          % (nt, n64, seen[1.0][1], abs(seen[1.0][1] - n64) / n64, seen[0.5][0], seen[2.0][0], seen[1.0][0]))
    for factor in (0.5, 2.0, 1.0):
        assert abs(seen[factor][1] - n64) <= NORM_TOL * n64, factor
    assert seen[0.5][0] < 1.0 and abs(seen[0.5][0] - 0.5 * n64 / (n64 + 1e-6)) <= 2.0 ** -23
    assert seen[2.0][0] == 1.0
    assert seen[1.0][0] < 1.0 and 1.0 - seen[1.0][0] <= 1e-6             # through the 1e-6 of the denominator
    assert seen[None] == (1.0, 0.0)
    for (buf, _), before in zip(G, g_before):
        assert torch.equal(buf, before)


# ---- 6: facl_adamw_apply -----------------------------------------------------------------------------------------------------
def _kernel_run(case, p0, gs, decay, mode, wd=0.0, max_norm=0.0):
    """`len(gs)` optimizer steps on guard-banded copies of p0 with zero moments.  mode "plain": facl_adam_prep + facl_adam_apply;
    "ex": [facl_grad_sqnorm when max_norm] + facl_adam_prep_ex + facl_adamw_apply.  Returns per step [(p, m, v) clones per
    tensor] and the (lr_t, c, norm) the step used; asserts the guard bands and the gradients untouched after every step."""
    from facl_amd import _lib
    lib = _lib.load_library()
    st = _lib.stream()
    nt = len(case)
    P = [_banded(p, s) for p, (_, s) in zip(p0, case)]
    M = [_banded(torch.zeros(n), s) for n, s in case]
    V = [_banded(torch.zeros(n), s) for n, s in case]
    G = [_banded(torch.zeros(n), s) for n, s in case]
    N, D = _ints([n for n, _ in case]), _ints(decay)
    nc = _chunks(case)
    pbuf, part = _banded(torch.full((nc,), float("nan"), dtype=torch.float64), 0, torch.float64)
    cbuf, consts = _banded(torch.full((5,), float("nan")), 0)
    lr, step = torch.full((1,), LR, device=DEV), torch.zeros(1, device=DEV)
    tabs = [_ptrs([d for _, d in T]) for T in (P, G, M, V)]
    out, used = [], []
    for k, g_k in enumerate(gs):
        for (_, d), g in zip(G, g_k):
            d.copy_(g)
        if mode == "plain":
            _lib.check(lib.facl_adam_prep(lr.data_ptr(), step.data_ptr(), B1, B2, consts.data_ptr(), st), "facl_adam_prep")
            _lib.check(lib.facl_adam_apply(nt, *tabs, N, consts.data_ptr(), B1, B2, EPS, st), "facl_adam_apply")
        else:
            if max_norm:
                _lib.check(lib.facl_grad_sqnorm(nt, tabs[1], N, part.data_ptr(), st), "facl_grad_sqnorm")
            _lib.check(lib.facl_adam_prep_ex(lr.data_ptr(), step.data_ptr(), B1, B2, part.data_ptr() if max_norm else None,
                                             nc if max_norm else 0, max_norm, 0, 0, 0, 0.0, consts.data_ptr(), st), "facl_adam_prep_ex")
            _lib.check(lib.facl_adamw_apply(nt, *tabs, N, D, consts.data_ptr(), B1, B2, EPS, wd, st), "facl_adamw_apply")
        torch.cuda.synchronize()
        assert float(step) == k + 1
        for T in (P, G, M, V):
            for (buf, _), (n, s) in zip(T, case):
                assert _bands_intact(buf, s, n), (k, n, s)
        assert _bands_intact(pbuf, 0, nc) and _bands_intact(cbuf, 0, 5)
        for (_, d), g in zip(G, g_k):
            assert torch.equal(d, g)                            # the stored gradient is only read
        out.append([(p[1].clone(), m[1].clone(), v[1].clone()) for p, m, v in zip(P, M, V)])
        used.append(tuple(float(x) for x in consts[2:5]) if mode == "ex" else None)
    return out, used


def _adamw64(p0, gs, decay, wd, max_norm):
    """torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW in fp64 on the CPU from the same fp32 inputs, with the fp32 betas the
    kernels hold.  Returns per step [(p, exp_avg, exp_avg_sq)]."""
    ps = [p.detach().cpu().double().clone().requires_grad_(True) for p in p0]
    groups = [{"params": [p for p, d in zip(ps, decay) if d], "weight_decay": wd},
              {"params": [p for p, d in zip(ps, decay) if not d], "weight_decay": 0.0}]
    opt = torch.optim.AdamW([g for g in groups if g["params"]], lr=LR, betas=FUSED_ADAM_BETAS, eps=EPS, foreach=False)
    out = []
    for g_k in gs:
        for p, g in zip(ps, g_k):
            p.grad = g.detach().cpu().double().clone()
        torch.nn.utils.clip_grad_norm_(ps, max_norm)
        opt.step()
        out.append([(p.detach().clone(), opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone()) for p in ps])
    return out


def _worst(got, want):
    """max over tensors and (p, m, v) of max |got - want| / max |want|."""
    w = 0.0
    for i, (gt, wt) in enumerate(zip(got, want)):
        for a, b in zip(gt, wt):
            assert torch.isfinite(a).all(), i
            w = max(w, float((a.cpu().double() - b).abs().max()) / max(float(b.abs().max()), 1e-30))
    return w


def _bits_equal(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for ta, tb in zip(a, b) for x, y in zip(ta, tb))


@pytest.mark.parametrize("nt", [14, 64])
def test_adamw_apply_vs_fp64_with_guard_bands(nt):
    """Three steps with clipping at half the first step's norm and wd = 0.05 on every second tensor, against clip_grad_norm_ +
    AdamW in fp64: parameters and both moments within ADAM_TOL of max |.| after every step.  The undecayed tensors equal the
    wd = 0 run bit for bit (and the decayed ones do not); max_norm = 1e30, wd = 0 equals facl_adam_prep + facl_adam_apply bit
    for bit.  Guard bands and gradients are checked inside every run."""
    case, p0, gs = _inputs(nt)
    decay = [i % 2 == 0 for i in range(nt)]
    max_norm = 0.5 * _norm64(gs[0])
    got, used = _kernel_run(case, p0, gs, decay, "ex", wd=WD, max_norm=max_norm)
    want = _adamw64(p0, gs, decay, WD, max_norm)
    for k in range(3):
        lr_t, c, norm = used[k]
        n64 = _norm64(gs[k])
        assert lr_t == LR and c < 1.0 and abs(c - max_norm / (n64 + 1e-6)) <= 2.0 ** -23 and abs(norm - n64) <= NORM_TOL * n64
        w = _worst(got[k], want[k])
        print("nt=%d step %d: c %.6f, worst error / max|.| %.2e" % (nt, k + 1, c, w))
        assert w <= ADAM_TOL, (k, w)
    # the reference itself tells decay and clipping from their absence by far more than the bound
    assert _worst(want[2], _adamw64(p0, gs, decay, 0.0, max_norm)[2]) > 10 * ADAM_TOL
    assert _worst(want[2], _adamw64(p0, gs, decay, WD, 1e30)[2]) > 10 * ADAM_TOL
    no_wd, _ = _kernel_run(case, p0, gs, decay, "ex", wd=0.0, max_norm=max_norm)
    for k in range(3):
        for i, d in enumerate(decay):
            same = _bits_equal([got[k][i]], [no_wd[k][i]])
            assert same == (not d), (k, i, d)
    plain, _ = _kernel_run(case, p0, gs, decay, "plain")
    for args in (dict(wd=0.0, max_norm=1e30), dict(wd=0.0, max_norm=0.0)):
        ex, used = _kernel_run(case, p0, gs, decay, "ex", **args)
        assert all(u[1] == 1.0 for u in used)
        for k in range(3):
            assert _bits_equal(ex[k], plain[k]), (args, k)


# ---- 7: the ABI refusals, beside a device ------------------------------------------------------------------------------------
def test_abi_refusals_launch_nothing():
    from facl_amd import _lib
    from test_optim_recipe_cpu import abi_refusals
    torch.zeros(1, device=DEV)
    abi_refusals(_lib.load_library())                       # made-up addresses: a launch would fault
    torch.cuda.synchronize()


# ---- 8-10: the training step (helpers as in test_gpu_key_encoder.py) ---------------------------------------------------------
RAGGED = dict(B=3, G=5, N=1000, D=3)
STEP_MODE = dict(loss_normalize=1, loss_temperature=0.1, loss_mask="exclude")
LR0 = f32(3e-4)
RECIPE = dict(weight_decay=0.05, schedule="cosine", warmup_steps=2, decay_steps=6)


def _make_step(c=RAGGED, **recipe):
    return make_contrastive_step(c, adam=recipe, **STEP_MODE)


class _Calls:
    """The library with every call's name recorded."""

    def __init__(self, lib):
        self.lib, self.names = lib, []

    def __getattr__(self, name):                            # once per name: callers compare entries by identity
        fn = getattr(self.lib, name)

        def call(*a):
            self.names.append(name)
            return fn(*a)
        setattr(self, name, call)
        return call

    def optimizer(self):
        return [n for n in self.names if "adam" in n or "sqnorm" in n]


@contextlib.contextmanager
def _recorded(monkeypatch):
    from facl_amd import _lib
    calls = _Calls(_lib.load_library())
    with monkeypatch.context() as m:
        m.setattr(_lib, "load_library", lambda: calls)
        yield calls


@pytest.fixture(scope="module")
def step_a():
    """Model A: one step of today's optimizer at the ragged size.  (the parameters before the step, the gradients, their fp64
    norm, the state after the step.)"""
    from facl_amd import _lib
    with _lib.poisoned():
        net, optim, step = _make_step()
        before = snapshot(net, optim)
        step(points(RAGGED, 100), order=np.random.RandomState(7).permutation(RAGGED["G"]))
        torch.cuda.synchronize()
        grads = {n: p.grad.detach().clone() for n, p in net.named_parameters() if p.grad is not None}
        after = snapshot(net, optim)
    return before, grads, _norm64(list(grads.values())), after


def test_default_optimizer_is_the_direct_call_sequence(step_a, monkeypatch):
    """FusedAdam with default arguments issues facl_adam_prep + facl_adam_apply and nothing else of the optimizer, and the step's
    parameters and moments are those of the two entries called directly on copies of the same buffers, bit for bit."""
    from facl_amd import _lib
    before, grads, _, after = step_a
    net, optim, step = _make_step()
    assert not optim.recipe and optim._partial is None
    with _recorded(monkeypatch) as calls:
        step(points(RAGGED, 100), order=np.random.RandomState(7).permutation(RAGGED["G"]))
    torch.cuda.synchronize()
    assert calls.optimizer() == ["facl_adam_prep", "facl_adam_apply"]
    assert float(optim.clip_coef()) == 1.0 and float(optim.grad_norm()) == 0.0 and float(optim.current_lr()) == LR0
    lib, st = _lib.load_library(), _lib.stream()
    names = [n for n, p in net.named_parameters() if p.grad is not None]
    assert names == list(grads) and len(names) >= 20
    P = [before["net"][n].to(DEV).clone().contiguous() for n in names]
    Gr = [grads[n].contiguous() for n in names]
    M, V = [torch.zeros_like(p) for p in P], [torch.zeros_like(p) for p in P]
    lr, cnt, consts = torch.full((1,), 3e-4, device=DEV), torch.zeros(1, device=DEV), torch.zeros(2, device=DEV)
    _lib.check(lib.facl_adam_prep(lr.data_ptr(), cnt.data_ptr(), 0.5, 0.999, consts.data_ptr(), st), "facl_adam_prep")
    _lib.check(lib.facl_adam_apply(len(P), _ptrs(P), _ptrs(Gr), _ptrs(M), _ptrs(V), _ints([p.numel() for p in P]),
                                   consts.data_ptr(), 0.5, 0.999, 1e-6, st), "facl_adam_apply")
    torch.cuda.synchronize()
    sd = net.state_dict()
    for n, p, m, v in zip(names, P, M, V):
        assert torch.equal(net.get_parameter(n).grad, grads[n]), n
        assert torch.equal(sd[n], p) and torch.equal(sd[n].cpu(), after["net"][n]), n
        state = optim.state[net.get_parameter(n)]
        assert torch.equal(state["exp_avg"], m) and torch.equal(state["exp_avg_sq"], v), n
    assert float(optim._step) == 1.0 == float(cnt)
    assert optim.state_dict()["param_groups"][0]["weight_decay"] == 0


def test_step_with_clipping_decay_and_cosine(step_a, monkeypatch):
    """Model B = model A with max_grad_norm = half of A's fp64 gradient norm, weight_decay 0.05 and cosine W = 2, T = 6."""
    from facl_amd.optim import lr_at_step
    before, grads_a, n64, _ = step_a
    net, optim, step = _make_step(max_grad_norm=0.5 * n64, **RECIPE)
    assert optim.recipe
    with _recorded(monkeypatch) as calls:
        step(points(RAGGED, 100), order=np.random.RandomState(7).permutation(RAGGED["G"]))
    torch.cuda.synchronize()
    assert calls.optimizer() == ["facl_grad_sqnorm", "facl_adam_prep_ex", "facl_adamw_apply"]
    named = dict(net.named_parameters())
    assert [n for n, p in named.items() if p.grad is not None] == list(grads_a)
    for n, g in grads_a.items():
        assert torch.equal(named[n].grad.view(torch.int32), g.view(torch.int32)), n      # the stored gradients: A's, unclipped
    gn, c, lr1 = float(optim.grad_norm()), float(optim.clip_coef()), float(optim.current_lr())
    print("norm fp64 %.9g kernel %.9g (rel %.2e), c %.7f, lr %.9g" % (n64, gn, abs(gn - n64) / n64, c, lr1))
    assert abs(gn - n64) <= NORM_TOL * n64
    assert c < 1.0 and abs(c - 0.5 * n64 / (n64 + 1e-6)) <= 2.0 ** -23
    want_lr = lr_at_step(LR0, 1, "cosine", 2, 6, 0.0)
    assert want_lr == 0.5 * LR0 and lr1 == f32(want_lr)
    # fp64 clip + AdamW on those gradients at that rate, from A's starting point
    names = list(grads_a)
    decay = [before["net"][n].ndim >= 2 for n in names]
    assert any(decay) and not all(decay)
    ps = [before["net"][n].double().clone().requires_grad_(True) for n in names]
    for p, n in zip(ps, names):
        p.grad = grads_a[n].cpu().double().clone()
    torch.nn.utils.clip_grad_norm_(ps, 0.5 * n64)
    ref = torch.optim.AdamW([{"params": [p for p, d in zip(ps, decay) if d], "weight_decay": 0.05},
                             {"params": [p for p, d in zip(ps, decay) if not d], "weight_decay": 0.0}],
                            lr=want_lr, betas=FUSED_ADAM_BETAS, eps=1e-6, foreach=False)
    ref.step()
    worst = 0.0
    for n, p in zip(names, ps):
        state = optim.state[named[n]]
        for what, got, want in (("param", named[n], p.detach()), ("exp_avg", state["exp_avg"], ref.state[p]["exp_avg"]),
                                ("exp_avg_sq", state["exp_avg_sq"], ref.state[p]["exp_avg_sq"])):
            d = float((got.detach().cpu().double() - want).abs().max()) / max(float(want.abs().max()), 1e-30)
            worst = max(worst, d)
            assert d <= ADAM_TOL, (n, what, d)
    print("worst error / max|.| %.2e" % worst)
    sd = optim.state_dict()
    assert sd["param_groups"][0]["weight_decay"] == 0.05 and float(sd["state"][0]["step"]) == 1.0


def test_recipe_graph_replay_equals_eager(step_a):
    """Six eager steps and six replayed ones (GraphedStep(restore=True)) from the same start, points and orders: parameters,
    BatchNorm buffers, moments, the step count and current_lr() bit-identical after every step, and current_lr() is
    fp32(lr_at_step) for t = 1..6: the schedule advances inside the replayed graph, with no host fill."""
    from facl_amd.optim import lr_at_step
    from facl_amd.train_common import GraphedStep
    n64 = step_a[2]
    G = RAGGED["G"]
    r = np.random.RandomState(7)
    orders = [r.permutation(G) for _ in range(6)]
    runs = []
    for graphed in (False, True):
        net, optim, step = _make_step(max_grad_norm=0.5 * n64, lr_min=1e-5, **RECIPE)
        run = GraphedStep(step, points(RAGGED, 99), G, restore=True) if graphed else step
        if graphed:
            assert float(optim._step) == 0.0
        per_step = []
        for k in range(6):
            out = [t.detach().clone() for t in run(points(RAGGED, 100 + k), order=orders[k])]
            torch.cuda.synchronize()
            assert all(torch.isfinite(t).all() for t in out)
            snap = snapshot(net, optim)
            per_step.append((out, snap["net"], snap["adam"], snap["step"], optim.current_lr().clone(), optim.clip_coef().clone(),
                             optim.grad_norm().clone()))
        assert float(optim._lr) == LR0 and optim.param_groups[0]["lr"] == 3e-4    # the host left the base rate alone
        runs.append(per_step)
    for k, (e, g) in enumerate(zip(*runs)):
        t = k + 1
        for a, b in zip(e[0], g[0]):
            assert torch.equal(a, b), (k, float(a), float(b))
        assert e[1].keys() == g[1].keys() and e[2].keys() == g[2].keys()
        for name in e[1]:
            assert torch.equal(e[1][name], g[1][name]), (k, name)
        for name in e[2]:
            for what in ("exp_avg", "exp_avg_sq"):
                assert torch.equal(e[2][name][what], g[2][name][what]), (k, name, what)
        assert e[3] == g[3] == t
        for i in (4, 5, 6):
            assert torch.equal(e[i].view(torch.int32), g[i].view(torch.int32)), (k, i)
        assert float(g[4]) == f32(lr_at_step(LR0, t, "cosine", 2, 6, 1e-5)), (t, float(g[4]))
        assert float(g[6]) > 0.0
    assert float(runs[1][5][4]) == f32(1e-5) and float(runs[1][0][5]) < 1.0       # lr_min at t = T; the first step was clipped


# ---- 11: the entries ---------------------------------------------------------------------------------------------------------
ENTRY = ["--synthetic", "1", "--steps_per_epoch", "3", "--batchSize", "4", "--num_crop", "4", "--SAMPLE_NUM", "512",
         "--clip_grad_norm", "1.0", "--adamw_decay", "0.05", "--lr_schedule", "cosine", "--lr_decay_epochs", "2", "--warmup_steps", "2",
         "--save_state_every", "1"]
LINE = r"epoch: %d loss mode is : 1 --loss: (\S+) \| clips/s: \S+ \| grad norm mean/max: (\S+)/(\S+), clipped (\d+)/3 steps"


def _run(folder, *extra):
    return run_train_entry(ENTRY + ["--save_root_dir", str(folder)] + [str(a) for a in extra])


def test_train_entry_with_the_recipe_and_resume(tmp_path):
    from facl_amd import cn3d_train_motion_GL as train
    from facl_amd import train_state
    a, b = tmp_path / "a", tmp_path / "b"
    sd_a, out_a = _run(a, "--nepoch", 2)
    for epoch in (0, 1):
        m = re.search(LINE % epoch, out_a)
        assert m, out_a
        loss, mean, mx, clipped = float(m.group(1)), float(m.group(2)), float(m.group(3)), int(m.group(4))
        assert np.isfinite(loss) and 0.0 < mean <= mx and np.isfinite(mx) and 0 <= clipped <= 3
    state_a = train_state.load_state(os.path.join(str(a), "state_1.pth"))
    assert state_a["flags"]["lr_schedule"] == "cosine" and state_a["flags"]["warmup_steps"] == 2
    assert state_a["optimizer"]["param_groups"][0]["weight_decay"] == 0.05 and float(state_a["optimizer"]["state"][0]["step"]) == 6.0
    # the same run stopped after epoch 0 and continued
    _run(b, "--nepoch", 1)
    sd_b, out_b = _run(b, "--nepoch", 2, "--resume", "auto")
    assert "resumed from %s: epoch 1" % os.path.join(str(b), "state_0.pth") in out_b
    assert re.search(LINE % 1, out_b) and not re.search(LINE % 0, out_b)
    assert_same_state(sd_b, sd_a, "model")
    assert_same_state(train_state.load_state(os.path.join(str(b), "state_1.pth")), state_a, "state_1")
    assert re.search(LINE % 1, out_b).groups() == re.search(LINE % 1, out_a).groups()
    # another warm-up would not continue the trajectory
    args = list(ENTRY)
    args[args.index("--warmup_steps") + 1] = "3"
    with pytest.raises(RuntimeError, match=r"--warmup_steps 3 \(the state: 2\)"):
        train.main(args + ["--save_root_dir", str(b), "--nepoch", "2", "--resume", "auto"])


def test_finetune_entry_with_the_recipe(tmp_path, capsys):
    from facl_amd import finetune
    finetune.main(ENTRY[:-2] + ["--nepoch", "1", "--num_class", "4", "--save_root_dir", str(tmp_path)])
    out = capsys.readouterr().out
    m = re.search(r"epoch: 0 --loss: (\S+) train top1: \S+ \| clips/s: \S+ \| grad norm mean/max: (\S+)/(\S+), clipped (\d+)/3 steps", out)
    assert m, out
    assert np.isfinite(float(m.group(1))) and 0.0 < float(m.group(2)) <= float(m.group(3))
    assert os.path.exists(os.path.join(str(tmp_path), "finetune_enc_0.pth"))
