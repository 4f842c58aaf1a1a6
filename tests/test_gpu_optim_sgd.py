"""SGD with momentum and LARS on the optimizer's chunk table: facl_tensor_sqnorms, facl_sgd_prep, facl_sgd_apply and
facl_amd.optim.FusedSGD, on ONE tensor list chosen for the walk's edges (both sides of a chunk and of a float4, a tensor one
element off a 16-byte boundary whose n % 4 == 0, an all-zero gradient, an all-zero masked parameter, a parameter without a
gradient), every buffer between guard bands.  The fp64 reference is tests/sgd_reference.py, pinned against torch.optim.SGD by
test_optim_sgd_cpu.py."""
import numpy as np
import pytest
import torch

from chunk_cases import CHUNK, DEV, _banded, _bands_intact, _ints, _ptrs
from sgd_reference import lars_trust, sgd_step
from test_optim_sgd_cpu import sgd_abi_refusals

pytestmark = pytest.mark.gpu
f32 = np.float32
LR, MU, WD, ETA = 0.05, 0.9, 1e-2, 1e-2

# (elements, shift off a 16-byte boundary, mask, kind)
TENSORS = [(1, 0, False, ""), (3, 0, True, ""), (2048, 0, False, ""), (2049, 0, True, ""), (4100, 0, True, ""), (8192, 0, True, ""),
           (4096, 1, True, ""),                               # misaligned with n % 4 == 0: the scalar walk
           (260, 0, True, "zero_grad"), (12, 0, True, "zero_param"), (2050, 0, True, "no_grad")]
ACT = [t for t in TENSORS if t[3] != "no_grad"]               # what reaches the kernels
NT = len(ACT)
MASK = [m for _, _, m, _ in ACT]
NCHUNK = sum((n + CHUNK - 1) // CHUNK for n, _, _, _ in ACT)
CHUNK0 = np.concatenate([[0], np.cumsum([(n + CHUNK - 1) // CHUNK for n, _, _, _ in ACT])])


def _values(seed, tensors=ACT):
    """Parameters of unit scale and gradients of scale 0.05 as NumPy fp32, the zero tensors zero."""
    r = np.random.RandomState(seed)
    p = [np.zeros(n, f32) if k == "zero_param" else r.randn(n).astype(f32) for n, _, _, k in tensors]
    g = [np.zeros(n, f32) if k == "zero_grad" else (0.05 * r.randn(n)).astype(f32) for n, _, _, k in tensors]
    return p, g


def _grads(seed, tensors=ACT):
    return _values(seed, tensors)[1]


class _Bufs:
    """Guard-banded device copies of a list of arrays."""

    def __init__(self, arrays, tensors=ACT, dtype=torch.float32):
        self.tensors = tensors
        self.pairs = [_banded(torch.from_numpy(a), s, dtype) for a, (_, s, _, _) in zip(arrays, tensors)]
        self.data = [d for _, d in self.pairs]

    def intact(self):
        return all(_bands_intact(b, s, n) for (b, _), (n, s, _, _) in zip(self.pairs, self.tensors))

    def numpy(self):
        return [d.cpu().numpy().copy() for d in self.data]

    def set(self, arrays):
        for d, a in zip(self.data, arrays):
            d.copy_(torch.from_numpy(a))


def _scalars(n, fill, dtype=torch.float32):
    return _banded(torch.full((n,), fill, dtype=dtype), 0, dtype)


def _bits(t):
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _same_bits(a, b):
    """NumPy fp32 arrays, bit for bit."""
    return np.array_equal(a.view(np.int32), b.view(np.int32))


N_ARR = lambda: _ints([n for n, _, _, _ in ACT])


# ---- 1: facl_tensor_sqnorms ----------------------------------------------------------------------------------------------------
def test_tensor_sqnorms():
    from facl_amd import _lib
    p, g = _values(1)
    P, G = _Bufs(p), _Bufs(g)
    gbuf, part0 = _scalars(NCHUNK, float("nan"), torch.float64)
    _lib.call("facl_grad_sqnorm", NT, _ptrs(G.data), N_ARR(), part0)
    runs = []
    for _ in range(2):
        (pb, pp), (qb, pg) = _scalars(NCHUNK, float("nan"), torch.float64), _scalars(NCHUNK, float("nan"), torch.float64)
        _lib.call("facl_tensor_sqnorms", NT, _ptrs(P.data), _ptrs(G.data), N_ARR(), pp, pg)
        torch.cuda.synchronize()
        assert _bands_intact(pb, 0, NCHUNK) and _bands_intact(qb, 0, NCHUNK)
        runs.append((pp, pg))
    assert _bands_intact(gbuf, 0, NCHUNK)
    (pp, pg), (pp2, pg2) = runs
    assert torch.equal(_bits(pg), _bits(part0))                                   # facl_grad_sqnorm's bits
    assert torch.equal(_bits(pp), _bits(pp2)) and torch.equal(_bits(pg), _bits(pg2))
    c = 0
    for a, b in zip(p, g):
        for lo in range(0, len(a), CHUNK):
            for got, x in ((pp, a), (pg, b)):
                want = float(np.sum(x[lo:lo + CHUNK].astype(np.float64) ** 2))
                assert abs(float(got[c]) - want) <= 1e-13 * want, (len(a), lo)
            c += 1
    assert c == NCHUNK
    assert P.intact() and G.intact()
    for x, y in zip(P.numpy() + G.numpy(), p + g):                                 # only read
        assert _same_bits(x, y)


# ---- 2: facl_sgd_prep ------------------------------------------------------------------------------------------------------------
def _prep(lr, step, pg, pp, npartial, consts, trust, max_norm=0.0, schedule=0, W=0, T=0, lr_min=0.0, eta=ETA, wd=WD, mask=MASK):
    from facl_amd import _lib
    _lib.call("facl_sgd_prep", lr, step, pg, pp, npartial, NT, N_ARR(), _ints(mask), max_norm, int(max_norm > 0), schedule, W, T,
              lr_min, eta, wd, consts, trust)


def _trust_want(pp, pg, c, mask=MASK, eta=ETA, wd=WD):
    pp, pg = pp.cpu().numpy(), pg.cpu().numpy()
    out = []
    for i in range(NT):
        wn = float(np.sqrt(pp[CHUNK0[i]:CHUNK0[i + 1]].sum()))
        gn = float(c) * float(np.sqrt(pg[CHUNK0[i]:CHUNK0[i + 1]].sum()))
        out.append(eta * wn / (gn + wd * wn) if (mask[i] and wn > 0 and gn > 0) else 1.0)
    return out


@pytest.mark.parametrize("name,kw", [("plain", {}), ("warmup", dict(W=3)), ("cosine", dict(schedule=1, W=2, T=5, lr_min=1e-3)),
                                     ("clip", dict(max_norm=0.5)), ("clip_cosine", dict(max_norm=0.5, schedule=1, W=2, T=5))])
def test_sgd_prep_against_adam_prep_ex(name, kw):
    """lr_t, c and norm are the bits facl_adam_prep_ex writes for the same inputs over six steps; with the parameter partials
    (LARS) every trust ratio is within 2 fp32 ulps of the fp64 formula on the partials, with the fp32 clip coefficient the
    kernel itself reports, and exactly 1 on the zero-gradient, zero-weight and unmasked tensors."""
    from facl_amd import _lib
    p, g = _values(2)
    P, G = _Bufs(p), _Bufs(g)
    (ppb, pp), (pgb, pg) = _scalars(NCHUNK, float("nan"), torch.float64), _scalars(NCHUNK, float("nan"), torch.float64)
    _lib.call("facl_tensor_sqnorms", NT, _ptrs(P.data), _ptrs(G.data), N_ARR(), pp, pg)
    lr = torch.full((1,), LR, device=DEV)
    steps = [torch.zeros(1, device=DEV) for _ in range(3)]
    (ab, ca), (sb, cs), (lb, cl) = (_scalars(5, float("nan")) for _ in range(3))
    (tb, trust), (ub, untouched) = _scalars(NT, float("nan")), _scalars(NT, float("nan"))
    clip = kw.get("max_norm", 0.0)
    for t in range(1, 7):
        _lib.call("facl_adam_prep_ex", lr, steps[0], 0.5, 0.999, pg if clip else None, NCHUNK if clip else 0, clip,
                  kw.get("schedule", 0), kw.get("W", 0), kw.get("T", 0), kw.get("lr_min", 0.0), ca)
        _prep(lr, steps[1], pg if clip else None, None, NCHUNK if clip else 0, cs, untouched, **kw)     # plain SGD
        _prep(lr, steps[2], pg, pp, NCHUNK, cl, trust, **kw)                                            # LARS
        torch.cuda.synchronize()
        assert [float(s) for s in steps] == [t, t, t]
        for c in (cs, cl):
            assert torch.equal(_bits(c[2:]), _bits(ca[2:])), (t, c.tolist(), ca.tolist())
            assert torch.equal(_bits(c[0:1]), _bits(c[2:3])) and float(c[1]) == 0.0
        if not clip:
            assert float(cs[3]) == 1.0 and float(cs[4]) == 0.0
        else:
            assert 0.0 < float(cs[3]) < 1.0 and float(cs[4]) > 0.5
        want = _trust_want(pp, pg, float(cl[3]))
        got = trust.cpu().numpy()
        for i, (w, (_, _, m, kind)) in enumerate(zip(want, ACT)):
            assert abs(float(got[i]) - w) <= 2 * float(np.spacing(f32(w))), (i, got[i], w)
            if kind or not m:
                assert got[i] == 1.0, (i, kind)
            else:
                assert got[i] != 1.0 and 0.0 < got[i] < 10.0
        assert torch.isnan(untouched).all()                                        # plain SGD writes no trust ratio
    assert all(_bands_intact(b, 0, 5) for b in (ab, sb, lb)) and _bands_intact(tb, 0, NT) and _bands_intact(ub, 0, NT)
    assert _bands_intact(ppb, 0, NCHUNK) and _bands_intact(pgb, 0, NCHUNK)


# ---- 3: facl_sgd_apply -----------------------------------------------------------------------------------------------------------
def _kernel_steps(mode, steps=4, mu=MU, wd=0.0, nesterov=0, max_norm=0.0, mask=MASK, seed=3):
    """`steps` steps of the entries on guard-banded buffers with fresh gradients each; after every step p and buf must hold the
    bits of the NumPy fp32 restatement (sgd_reference.sgd_step on fp32 arrays) given the consts and trust the DEVICE wrote.
    Returns the final (p, buf) as NumPy."""
    from facl_amd import _lib
    lars = mode == "lars"
    p, _ = _values(seed)
    buf = [np.zeros_like(a) for a in p]
    P, B, G = _Bufs(p), _Bufs(buf), _Bufs(_grads(seed))
    (ppb, pp), (pgb, pg) = _scalars(NCHUNK, float("nan"), torch.float64), _scalars(NCHUNK, float("nan"), torch.float64)
    (cb, consts), (tb, trust) = _scalars(5, float("nan")), _scalars(NT, float("nan"))
    lr, step = torch.full((1,), LR, device=DEV), torch.zeros(1, device=DEV)
    tabs = lambda: (_ptrs(P.data), _ptrs(G.data), _ptrs(B.data))
    for k in range(steps):
        g = _grads(100 * seed + k)
        G.set(g)
        if lars:
            _lib.call("facl_tensor_sqnorms", NT, tabs()[0], tabs()[1], N_ARR(), pp, pg)
        elif max_norm:
            _lib.call("facl_grad_sqnorm", NT, tabs()[1], N_ARR(), pg)
        _prep(lr, step, pg if (lars or max_norm) else None, pp if lars else None, NCHUNK if (lars or max_norm) else 0, consts,
              trust if lars else None, max_norm=max_norm, wd=wd, mask=mask)
        torch.cuda.synchronize()
        lr_t, c = consts.cpu().numpy()[2], consts.cpu().numpy()[3]
        q = trust.cpu().numpy() if lars else None
        assert lr_t == f32(LR) and (c < 1.0 if max_norm else c == 1.0)
        sgd_step(p, g, buf, lr_t, f32(mu), f32(wd), mask, nesterov, c, q)          # fp32 arrays and scalars: the five lines
        _lib.call("facl_sgd_apply", NT, *tabs(), N_ARR(), _ints(mask), consts, trust if lars else None, mu, wd, nesterov)
        torch.cuda.synchronize()
        for i, (x, y, a, b) in enumerate(zip(P.numpy(), B.numpy(), p, buf)):
            assert _same_bits(x, a) and _same_bits(y, b), (mode, k, i)
        for x, y in zip(G.numpy(), g):
            assert _same_bits(x, y)                                                # g is only read
        assert P.intact() and B.intact() and G.intact()
        assert all(_bands_intact(b, 0, n) for b, n in ((ppb, NCHUNK), (pgb, NCHUNK), (cb, 5), (tb, NT)))
    assert all(np.isfinite(a).all() for a in p)
    return p, buf


@pytest.mark.parametrize("mode,kw", [("sgd", {}), ("sgd", dict(nesterov=1)), ("sgd", dict(wd=WD)), ("sgd", dict(wd=WD, max_norm=0.5)),
                                     ("lars", dict(wd=WD)), ("lars", dict(wd=WD, nesterov=1, max_norm=0.5))])
def test_sgd_apply_is_the_five_line_rule_to_the_bit(mode, kw):
    _kernel_steps(mode, **kw)


def test_sgd_apply_identities():
    """mu = 0, wd = 0: p - lr * g to the bit; LARS with an all-zero mask: the bits of SGD."""
    p0, _ = _values(3)
    g0 = _grads(300)
    p, buf = _kernel_steps("sgd", steps=1, mu=0.0, wd=0.0)
    for a, x, g in zip(p, p0, g0):
        assert _same_bits(a, x - f32(LR) * g)
    none = [False] * NT
    a = _kernel_steps("sgd", wd=WD, mask=none)
    b = _kernel_steps("lars", wd=WD, mask=none)
    for x, y in zip(a[0] + a[1], b[0] + b[1]):
        assert _same_bits(x, y)


# ---- 4: FusedSGD ------------------------------------------------------------------------------------------------------------------
def _fused(seed, tensors=TENSORS, **kw):
    """(optimizer, parameters, P, G): the parameters are views into guard-banded buffers, their gradients too (the last tensor
    has none); the NumPy start values."""
    from facl_amd.optim import FusedSGD
    p0, g0 = _values(seed, tensors)
    P, G = _Bufs(p0, tensors), _Bufs(g0, tensors)
    params = [torch.nn.Parameter(d) for d in P.data]
    for w, d, x, (_, _, _, kind) in zip(params, G.data, P.data, tensors):
        w.grad = None if kind == "no_grad" else d
        assert w.data_ptr() == x.data_ptr()
    opt = FusedSGD(params, lr=LR, decay_mask=[m for _, _, m, _ in tensors], **kw)
    return opt, params, P, G, p0


def _set_grads(G, seed, tensors=TENSORS):
    g = _grads(seed, tensors)
    G.set(g)
    return [None if k == "no_grad" else a for a, (_, _, _, k) in zip(g, tensors)]


def _err(got, ref):
    return [float(np.abs(a.astype(np.float64) - b).max()) for a, b in zip(got, ref)]


def test_fused_sgd_against_fp64(monkeypatch):
    """Five steps with fresh gradients, SGD (momentum 0.9, Nesterov, decay on the mask) and LARS, against the fp64 reference fed
    the same fp32 gradients.  The bar is measured in the test: torch.optim.SGD in fp32 on the device on the same data has a
    maximum error e_t per tensor against the same reference, and FusedSGD must stay within 2 e_t + one fp32 ulp of max |p|; LARS
    (no torch counterpart) is held to the bar measured for SGD, against the fp64 LARS reference.  Also: the launch sequences."""
    from facl_amd import _lib
    mask = [m for _, _, m, _ in TENSORS]
    names = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a, **k: (names.append(name), real(name, *a, **k))[1])
    bars = None
    for kind in ("sgd", "lars"):
        opt, params, P, G, p0 = _fused(5, momentum=MU, nesterov=True, weight_decay=WD, lars=kind == "lars", lars_eta=ETA)
        ref, rbuf = [a.astype(np.float64) for a in p0], [np.zeros(len(a)) for a in p0]
        tp = [torch.nn.Parameter(torch.from_numpy(a).to(DEV)) for a in p0]
        topt = torch.optim.SGD([{"params": [t for t, m in zip(tp, mask) if m], "weight_decay": float(f32(WD))},
                                {"params": [t for t, m in zip(tp, mask) if not m], "weight_decay": 0.0}],
                               lr=float(f32(LR)), momentum=float(f32(MU)), dampening=0, nesterov=True)   # the kernels' fp32 constants
        for k in range(5):
            g = _set_grads(G, 500 + k)
            del names[:]
            opt.step()
            assert names == (["facl_tensor_sqnorms"] if kind == "lars" else []) + ["facl_sgd_prep", "facl_sgd_apply"]
            g64 = [None if a is None else a.astype(np.float64) for a in g]
            trust = lars_trust(ref, g64, mask, ETA, WD) if kind == "lars" else None
            sgd_step(ref, g64, rbuf, float(f32(LR)), float(f32(MU)), float(f32(WD)), mask, True, 1.0, trust)
            if kind == "sgd":
                for t, a in zip(tp, g):
                    t.grad = None if a is None else torch.from_numpy(a).to(DEV)
                topt.step()
        torch.cuda.synchronize()
        assert P.intact() and G.intact() and float(opt._step) == 5.0
        assert _same_bits(P.numpy()[-1], p0[-1])                                   # no gradient: skipped
        e_f = _err(P.numpy(), ref)
        if kind == "sgd":
            e_t = _err([t.detach().cpu().numpy() for t in tp], ref)
            bars = [2 * e + float(np.spacing(f32(np.abs(r).max()))) for e, r in zip(e_t, ref)]
            print("SGD: max error vs fp64, torch fp32 %.3e, FusedSGD %.3e" % (max(e_t), max(e_f)))
            assert bool((opt.trust_ratios() == 1).all())
        else:
            print("LARS: max error vs fp64, FusedSGD %.3e (bar from SGD: %.3e)" % (max(e_f), max(bars)))
            r = opt.trust_ratios().cpu().numpy()
            # the zero parameter has moved since its first step; the zero gradient keeps its ratio at 1
            assert len(r) == NT and all((x != 1.0) == (m and k != "zero_grad") for x, (_, _, m, k) in zip(r, ACT))
        for i, (e, bar) in enumerate(zip(e_f, bars)):
            assert e <= bar, (kind, i, e, bar)
        sd = opt.state_dict()
        assert set(sd["state"][0]) == {"step", "momentum_buffer"} and float(sd["state"][0]["step"]) == 5.0
        grp = sd["param_groups"][0]
        assert (grp["lr"], grp["momentum"], grp["dampening"], grp["weight_decay"], grp["nesterov"]) == (LR, MU, 0, WD, True)
    del names[:]
    opt, params, P, G, _ = _fused(5, max_grad_norm=0.5)
    opt.step()
    assert names == ["facl_grad_sqnorm", "facl_sgd_prep", "facl_sgd_apply"] and 0.0 < float(opt.clip_coef()) < 1.0
    assert float(opt.grad_norm()) > 0.5 and float(opt.current_lr()) == float(f32(LR))


@pytest.mark.parametrize("kind", ["sgd", "lars"])
def test_graph_replay_equals_eager(kind):
    """Three replays of one captured step, the rate changed on the host between them (sync_lr), against three eager steps on a
    fresh copy: parameters, buffers, the step counter, consts and trust bit for bit.  With clipping."""
    kw = dict(momentum=MU, weight_decay=WD, lars=kind == "lars", lars_eta=ETA, max_grad_norm=0.5, warmup_steps=2)
    lrs = (LR, 0.5 * LR, 0.25 * LR)
    runs = []
    for graphed in (False, True):
        opt, params, P, G, _ = _fused(6, **kw)
        graph = None
        if graphed:
            opt.sync_lr()                                     # the fill is not part of the graph
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                opt.step()
            torch.cuda.synchronize()
            assert float(opt._step) == 0.0                    # the capture ran nothing
        seen = []
        for k, lr in enumerate(lrs):
            _set_grads(G, 600 + k)
            opt.param_groups[0]["lr"] = lr
            if graphed:
                opt.sync_lr()
                graph.replay()
            else:
                opt.step()
            torch.cuda.synchronize()
            seen.append((P.numpy(), [opt.state[w]["momentum_buffer"].cpu().numpy() for w in params], opt._step.clone(),
                         opt._consts.clone(), opt._trust.clone()))
            assert P.intact() and G.intact()
        runs.append(seen)
    for k, (e, g) in enumerate(zip(*runs)):
        for x, y in zip(e[0] + e[1], g[0] + g[1]):
            assert _same_bits(x, y), k
        for i in (2, 3, 4):
            assert torch.equal(_bits(e[i]), _bits(g[i])), (k, i)
        assert float(g[2]) == k + 1 and float(g[3][2]) == float(f32(min(1.0, (k + 1) / 2.0) * float(f32(lrs[k]))))
        assert 0.0 < float(g[3][3]) < 1.0
    if kind == "lars":
        assert bool((runs[1][-1][4][:NT] != 1).any())


def test_non_finite_gradient():
    """One NaN gradient element.  Without clipping the update is elementwise: that element of that tensor is NaN, so a value
    reduced from the parameters is non-finite for the loss check, and every other tensor holds the bits of the run without
    the NaN (LARS too: a NaN norm gives the ratio 1).  With clipping the norm is NaN, c is NaN and every parameter is NaN, as for
    Adam."""
    from facl_amd.train_common import check_finite_loss
    hit = 4                                                   # the 4100-element tensor
    for kind, clip in (("sgd", 0.0), ("lars", 0.0), ("sgd", 0.5)):
        kw = dict(momentum=MU, weight_decay=WD, lars=kind == "lars", lars_eta=ETA, max_grad_norm=clip)
        clean, _, Pc, Gc, _ = _fused(7, **kw)
        opt, params, P, G, _ = _fused(7, **kw)
        G.data[hit][2077] = float("nan")
        clean.step()
        opt.step()
        torch.cuda.synchronize()
        got, want = P.numpy(), Pc.numpy()
        assert np.isnan(got[hit][2077])
        with pytest.raises(FloatingPointError):
            check_finite_loss(float(sum(w.detach().double().sum() for w in params)), 0, 0)
        if clip:
            assert all(np.isnan(a).all() for a in got[:-1]) and np.isnan(float(opt.clip_coef()))
        else:
            assert np.isnan(got[hit]).sum() == 1
            for i, (a, b) in enumerate(zip(got, want)):
                if i != hit:
                    assert _same_bits(a, b), (kind, i)
            if kind == "lars":
                assert float(opt.trust_ratios()[hit]) == 1.0
        assert _same_bits(got[-1], want[-1]) and P.intact() and G.intact()       # the tensor without a gradient


def test_abi_refusals_beside_a_device():
    from facl_amd import _lib
    torch.zeros(1, device=DEV)
    sgd_abi_refusals(_lib.load_library())
    torch.cuda.synchronize()
