"""GPU tests of the loss modes of the global / circle losses (cosine similarity, temperature, negatives-only mask): the row
pass, the two mask modes of the fused pair-loss kernels, utils_my.contrastive_losses_stacked, the training step (eager and
graph-replayed) and the training entry.  The fp64 truth is the device-agnostic closed form of utils_my (held to materialised
logits in test_loss_modes_cpu.py).  The whole module runs on NaN-poisoned scratch."""

import numpy as np
import pytest
import torch

from helpers import snapshot
from poison import poisoned_scratch  # noqa: F401
from step_factory import make_contrastive_step, points

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LOSS_TOL, GRAD_TOL = 2e-6, 2e-5      # test_gpu_tail.py::test_contrastive_pair_on_stacked_embeddings_vs_closed_form_fp64


# ---- 1: the row pass ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tau", [1.0, 0.07])
@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("R,C", [(5, 512), (33, 64), (7, 8)])
def test_loss_rows_vs_torch_fp64(R, C, normalize, tau):
    """n = x s / max(||x||, 1e-12) resp. x s and its gradient against torch in fp64, with one all-zero row: forward within
    1e-6 s absolute, gradient within 1e-5 of its norm without the zero row (the bounds of test_normalize_map_vs_torch);
    every row of both outputs is written (poison)."""
    from facl_amd.utils_my import loss_rows, loss_scale
    torch.manual_seed(R + C)
    x0 = torch.randn(R, C, device=DEV)
    x0[R // 2] = 0.0
    s = loss_scale(tau)
    assert s == float(np.float32(1.0 / np.sqrt(tau)))
    xa = x0.clone().requires_grad_(True)
    n = loss_rows(xa, normalize, tau)
    xr = x0.double().requires_grad_(True)
    nr = (torch.nn.functional.normalize(xr, p=2, dim=1, eps=1e-12) if normalize else xr) * s
    assert torch.isfinite(n).all()
    err = float((n.detach().double() - nr.detach()).abs().max())
    print("rows fwd R=%d C=%d norm=%d tau=%g: max abs err %.3e (bound %.3e)" % (R, C, normalize, tau, err, 1e-6 * s))
    assert err <= 1e-6 * s
    g = torch.randn_like(x0)
    (n * g).sum().backward()
    (nr * g.double()).sum().backward()
    assert torch.isfinite(xa.grad).all()
    keep = torch.ones(R, dtype=torch.bool, device=DEV)
    keep[R // 2] = False                                     # d/dx at x = 0 is not defined (torch returns 0/eps terms)
    e = float((xa.grad.double() - xr.grad)[keep].norm() / xr.grad[keep].norm())
    print("rows bwd: rel err %.3e" % e)
    assert e < 1e-5


def test_loss_rows_refuses_bad_shapes():
    from facl_amd import _lib
    lib = _lib.load_library()
    x = torch.randn(4, 8, device=DEV)
    n, inv = torch.empty_like(x), torch.empty(4, device=DEV)
    call = lambda R, C, nm, s: lib.facl_loss_rows_fwd(_lib.ptr(x), R, C, nm, s, _lib.ptr(n), _lib.ptr(inv), _lib.stream())
    assert call(4, 8, 1, 1.0) == 0
    for R, C, nm, s in ((4, 6, 1, 1.0), (4, 2, 0, 1.0), (0, 8, 1, 1.0), (4, 8, 2, 1.0), (4, 8, 1, 0.0), (4, 8, 1, float("inf")),
                        (4, 8, 1, float("nan"))):
        assert call(R, C, nm, s) == -1, (R, C, nm, s)
        assert lib.facl_loss_rows_bwd(_lib.ptr(n), _lib.ptr(n), _lib.ptr(inv), R, C, nm, s, _lib.ptr(x), _lib.stream()) == -1
    torch.cuda.synchronize()


@pytest.mark.parametrize("normalize", [1, 0])
def test_loss_rows_inv_norm_output(normalize):
    """facl_loss_rows_fwd's second output: inv_norm_r = 1 / max(||x_r||, 1e-12) (1e12 for the all-zero row), and 1 with
    normalize = 0; every entry written (poison).  fp64 sum of squares rounded once: within 2 ulp of the fp64 value."""
    from facl_amd import _lib
    lib = _lib.load_library()
    torch.manual_seed(9)
    R, C = 33, 64
    x = torch.randn(R, C, device=DEV)
    x[R // 2] = 0.0
    n, inv = _lib.empty_like(x), _lib.empty(R, device=DEV)
    _lib.check(lib.facl_loss_rows_fwd(_lib.ptr(x), R, C, normalize, 2.0, _lib.ptr(n), _lib.ptr(inv), _lib.stream()), "rows_fwd")
    want = 1.0 / x.double().norm(dim=1).clamp_min(1e-12) if normalize else torch.ones(R, dtype=torch.float64, device=DEV)
    assert torch.isfinite(inv).all()
    assert float(((inv.double() - want).abs() / want).max()) <= 2 * 2.0 ** -24
    if not normalize:
        assert torch.equal(inv, torch.ones_like(inv)) and torch.equal(n, x * 2.0)


# ---- 2: the pair loss on a synthetic similarity matrix -----------------------------------------------------------------------
def _pair_closed_form(sim, G, B, Bk, order, off, mask):
    """(loss_c, loss_circle) of loss.hip:1-13 on a given ((G+1) B, G Bk) similarity matrix, in sim's dtype."""
    J = G * Bk
    col_clip = torch.arange(J, device=sim.device) % Bk
    same = col_clip[None, :] == (torch.arange(B, device=sim.device) + off)[:, None]              # (B, J)
    fill = torch.full((), 0.0 if mask == "zero" else float("-inf"), dtype=sim.dtype, device=sim.device)
    blocks = sim.view(G + 1, B, J)
    n = torch.arange(B, device=sim.device)
    lse_g = torch.logsumexp(torch.where(same, fill, blocks[G]), dim=1)
    pos_g = torch.stack([blocks[G][n, g * Bk + n + off] for g in range(G)])
    loss_c = (torch.logaddexp(pos_g, lse_g[None, :]) - pos_g).mean(dim=1).sum()
    order = [int(o) for o in order]
    neg = torch.cat([torch.where(same, fill, blocks[order[i]]) for i in range(G - 1)], dim=1)
    lse_o = torch.logsumexp(neg, dim=1)
    pos_o = torch.stack([blocks[order[i]][n, order[i + 1] * Bk + n + off] for i in range(G - 1)])
    loss_o = (torch.logaddexp(pos_o, lse_o[None, :]) - pos_o).mean(dim=1).sum()
    return loss_c, loss_o


def _fp32_yardstick(f, *inputs64):
    """Relative errors of a plain torch-fp32 evaluation of the closed form `f` against its fp64 evaluation on the same
    inputs: ((loss_c, loss_circle) errors, gradient error of loss_c + loss_circle wrt inputs64[0])."""
    outs, grads = [], []
    for dt in (torch.float64, torch.float32):
        xs = [t.detach().to(dt).requires_grad_(True) for t in inputs64]
        lc, lo = f(*xs)
        (g,) = torch.autograd.grad(lc + lo, xs[:1])
        outs.append((float(lc.detach()), float(lo.detach())))
        grads.append(g.double())
    e_l = tuple(abs(a - b) / abs(b) for a, b in zip(outs[1], outs[0]))
    return e_l, float((grads[1] - grads[0]).norm() / grads[0].norm())


@pytest.mark.parametrize("filling", ["normal", "minus200"])
@pytest.mark.parametrize("mask", ["zero", "exclude"])
@pytest.mark.parametrize("G,B,Bk,off", [(6, 5, 5, 0), (4, 3, 6, 3), (24, 2, 48, 3)])
def test_pair_loss_entry_on_synthetic_sim(G, B, Bk, off, mask, filling):
    """facl_contrast_pair_sum_mask against the fp64 closed form on the same fp32 similarities: the register kernel with a
    ragged tail, a sharded shape, and the streaming kernel ((G - 1) J > 24 * 1024).  Filling N(0, 2^2), and uniform in
    [-203, -197]: there a log-sum-exp that keeps a floor of 0 under `exclude` returns -inf (true value about -198)."""
    from facl_amd import _lib
    from facl_amd.sa_mlp import _Workspace
    from facl_amd.utils_my import MASK_MODES
    lib = _lib.load_library()
    torch.manual_seed(G * 1000 + Bk)
    J = G * Bk
    if G == 24:
        assert (G - 1) * J > 24 * 1024
    sim = torch.randn((G + 1) * B, J, device=DEV) * 2.0 if filling == "normal" else \
        torch.rand((G + 1) * B, J, device=DEV) * 6.0 - 203.0
    order = torch.as_tensor(np.random.RandomState(G).permutation(G), device=DEV)
    ws = _Workspace.get(torch.device(DEV))
    dsim = _lib.empty_like(sim)
    l64, l32 = _lib.empty(2, dtype=torch.float64, device=DEV), _lib.empty(3, device=DEV)
    _lib.check(lib.facl_contrast_pair_sum_mask(_lib.ptr(sim), G, B, Bk, J, _lib.ptr(order), off, MASK_MODES[mask], _lib.ptr(dsim),
                                               _lib.ptr(l64), _lib.ptr(l32), _lib.ptr(ws), _lib.stream()), "pair_sum_mask")
    torch.cuda.synchronize()
    s64 = sim.double().requires_grad_(True)
    rc, ro = _pair_closed_form(s64, G, B, Bk, order.tolist(), off, mask)
    (gr,) = torch.autograd.grad(rc + ro, s64)
    rc, ro = rc.detach(), ro.detach()
    e_c, e_o = abs(float(l64[0]) - float(rc)) / abs(float(rc)), abs(float(l64[1]) - float(ro)) / abs(float(ro))
    e_g = float((dsim.double() - gr).norm() / gr.norm())
    y_l, y_g = _fp32_yardstick(lambda s_: _pair_closed_form(s_, G, B, Bk, order.tolist(), off, mask), sim.double())
    print("pair G=%d B=%d Bk=%d %s %s: loss_c %.3e loss_circle %.3e dsim %.3e | torch-fp32 %.3e %.3e %.3e"
          % (G, B, Bk, mask, filling, e_c, e_o, e_g, y_l[0], y_l[1], y_g))
    assert torch.isfinite(l64).all() and torch.isfinite(dsim).all()
    assert e_c <= LOSS_TOL and e_o <= LOSS_TOL
    assert e_g <= GRAD_TOL
    c, o = l64[0].float(), l64[1].float()
    assert torch.equal(l32, torch.stack((c, o, o + c)))
    if mask == "zero":                                      # mode 0 IS the entry without the argument
        d0 = _lib.empty_like(sim)
        m64, m32 = _lib.empty(2, dtype=torch.float64, device=DEV), _lib.empty(3, device=DEV)
        _lib.check(lib.facl_contrast_pair_sum(_lib.ptr(sim), G, B, Bk, J, _lib.ptr(order), off, _lib.ptr(d0), _lib.ptr(m64),
                                              _lib.ptr(m32), _lib.ptr(ws), _lib.stream()), "pair_sum")
        assert torch.equal(d0, dsim) and torch.equal(m64, l64) and torch.equal(m32, l32)
    else:                                                   # same-clip columns: no gradient except at the positives
        same = (torch.arange(J, device=DEV) % Bk)[None, :] == (torch.arange(B, device=DEV) + off).repeat(G + 1)[:, None]
        assert int((dsim[same] != 0).sum()) <= 2 * G * B


# ---- 3: contrastive_losses_stacked -------------------------------------------------------------------------------------------
MODES = [(True, 0.07, "exclude"), (True, 0.2, "zero"), (False, 4.0, "exclude")]


@pytest.mark.parametrize("normalize,tau,mask", MODES)
@pytest.mark.parametrize("G,B,C,world", [(6, 5, 32, 1), (4, 3, 16, 2), (10, 4, 512, 1)])
def test_stacked_losses_with_modes_vs_closed_form_fp64(G, B, C, world, normalize, tau, mask):
    """Row pass + similarity GEMM + pair loss + their backward against the fp64 closed form of global_contrast /
    circle_contrast: both values and the gradient wrt the stacked embeddings, single-process and sharded (gathered keys: as
    raw embeddings, and through the callable form the data-parallel step uses)."""
    from facl_amd.utils_my import circle_contrast, contrastive_losses_stacked, global_contrast, loss_rows
    torch.manual_seed(G * B + C)
    Bk, off = B * world, B * (world - 1)
    keys0 = (torch.randn(G, Bk, C, dtype=torch.float64) * 0.3).to(DEV)
    x0 = keys0[:, off:off + B].reshape(G * B, C).clone()
    xg0 = (torch.randn(B, C, dtype=torch.float64) * 0.3).to(DEV)
    order = np.random.RandomState(1).permutation(G)
    kw = dict(normalize=normalize, temperature=tau, mask=mask)

    def keys_of(x, base):
        k = base.clone()
        k[:, off:off + B] = x.view(G, B, C)
        return k.reshape(G * Bk, C)

    def truth(xg, x):
        k = keys_of(x, keys0.to(x.dtype)) if world > 1 else None
        return (global_contrast(G, xg, x, None, x_keys=k, clip_offset=off, **kw),
                circle_contrast(G, x, B, order=order, x_keys=k, clip_offset=off, **kw))

    xg64, x64 = xg0.clone().requires_grad_(True), x0.clone().requires_grad_(True)
    lc_r, lo_r = truth(xg64, x64)
    gr = torch.autograd.grad(0.7 * lc_r + 1.3 * lo_r, (xg64, x64))
    lc_r, lo_r = lc_r.detach(), lo_r.detach()
    st = torch.cat((x0, xg0), 0).float().requires_grad_(True)
    k32 = keys_of(st[:G * B], keys0.float()) if world > 1 else None
    lc, lo = contrastive_losses_stacked(G, st, order, x_keys=k32, clip_offset=off, **kw)
    (0.7 * lc + 1.3 * lo).backward()                        # distinct upstream gradients exercise facl_scale_rows2
    g = st.grad.double()
    e = (abs(float(lc.detach()) - float(lc_r)) / abs(float(lc_r)), abs(float(lo.detach()) - float(lo_r)) / abs(float(lo_r)),
         float((g[:G * B] - gr[1]).norm() / gr[1].norm()), float((g[G * B:] - gr[0]).norm() / gr[0].norm()))
    # the yardstick: plain torch fp32 of the same closed form (gradient wrt x)
    y_l, y_g = _fp32_yardstick(lambda x_, xg_: truth(xg_, x_), x0, xg0)
    print("stacked G=%d B=%d C=%d world=%d %s: loss_c %.3e loss_circle %.3e dx %.3e dxg %.3e | torch-fp32 %.3e %.3e dx %.3e"
          % (G, B, C, world, (normalize, tau, mask), *e, y_l[0], y_l[1], y_g))
    assert torch.isfinite(g).all()
    assert e[0] <= LOSS_TOL and e[1] <= LOSS_TOL
    assert e[2] < GRAD_TOL and e[3] < GRAD_TOL
    if world > 1:
        # the data-parallel wiring: the local view rows are mapped, then "gathered" (the other ranks' rows mapped alike)
        others = loss_rows(keys0.float().reshape(G * Bk, C), normalize, tau).view(G, Bk, C).detach()
        st2 = st.detach().clone().requires_grad_(True)
        lc2, lo2 = contrastive_losses_stacked(G, st2, order, x_keys=lambda nv: keys_of(nv, others), clip_offset=off, **kw)
        (0.7 * lc2 + 1.3 * lo2).backward()
        assert torch.equal(lc2, lc) and torch.equal(lo2, lo)
        g2 = st2.grad.double()
        assert float((g2[:G * B] - gr[1]).norm() / gr[1].norm()) < GRAD_TOL
        assert float((g2[G * B:] - gr[0]).norm() / gr[0].norm()) < GRAD_TOL


# ---- 4: default-mode identity ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G,B,C,world", [(6, 5, 32, 1), (4, 3, 16, 2)])
def test_explicit_defaults_are_bit_identical(G, B, C, world):
    from facl_amd.utils_my import contrastive_losses_stacked
    torch.manual_seed(5)
    Bk, off = B * world, B * (world - 1)
    st0 = torch.randn((G + 1) * B, C, device=DEV) * 0.3
    keys = torch.randn(G * Bk, C, device=DEV) * 0.3 if world > 1 else None
    order = np.random.RandomState(2).permutation(G)
    res = []
    for kw in ({}, dict(normalize=False, temperature=1.0, mask="zero")):
        st = st0.clone().requires_grad_(True)
        lc, lo, ls = contrastive_losses_stacked(G, st, order, x_keys=keys, clip_offset=off, with_sum=True, **kw)
        (0.7 * lc + 1.3 * lo).backward()
        res.append((lc.detach(), lo.detach(), ls.detach(), st.grad))
    for a, b in zip(*res):
        assert torch.isfinite(a).all() and torch.equal(a, b)


# ---- 5: refusals -------------------------------------------------------------------------------------------------------------
def test_mode_refusals():
    """Host side: ValueError before any launch.  C ABI: FACL_E_SHAPE for a mask mode outside {0, 1} and for `exclude` with
    one key clip."""
    from facl_amd import _lib
    from facl_amd.sa_mlp import _Workspace
    from facl_amd.utils_my import contrastive_losses_stacked
    G, B, C = 4, 3, 16
    st = torch.randn((G + 1) * B, C, device=DEV)
    order = np.arange(G)
    for tau in (0.0, -0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="temperature"):
            contrastive_losses_stacked(G, st, order, temperature=tau)
    with pytest.raises(ValueError, match="mask"):
        contrastive_losses_stacked(G, st, order, mask="drop")
    with pytest.raises(ValueError, match="negative"):
        contrastive_losses_stacked(G, st[:G + 1], order, mask="exclude")          # B = 1, one rank: one key clip
    lib = _lib.load_library()
    ws = _Workspace.get(torch.device(DEV))
    J = G * B
    sim, dsim = torch.randn((G + 1) * B, J, device=DEV), torch.empty((G + 1) * B, J, device=DEV)
    l64, l32 = torch.empty(2, dtype=torch.float64, device=DEV), torch.empty(3, device=DEV)
    o = torch.arange(G, device=DEV)
    call = lambda B_, Bk_, mode: lib.facl_contrast_pair_sum_mask(_lib.ptr(sim), G, B_, Bk_, G * Bk_, _lib.ptr(o), 0, mode,
                                                                 _lib.ptr(dsim), _lib.ptr(l64), _lib.ptr(l32), _lib.ptr(ws), _lib.stream())
    assert call(B, B, 0) == 0 and call(B, B, 1) == 0
    for mode in (2, -1):
        assert call(B, B, mode) == -1
    assert call(1, 1, 1) == -1 and call(1, 1, 0) == 0
    torch.cuda.synchronize()


# ---- 6: the training step ----------------------------------------------------------------------------------------------------
RAGGED = dict(B=3, G=5, N=1000, D=3)                       # config `ragged` of test_gpu_trajectory.py
STEP_MODE = dict(loss_normalize=1, loss_temperature=0.1, loss_mask="exclude")
TOL = 1e-4                                                 # test_gpu_trajectory.py: losses of one step


def test_step_with_modes_vs_closed_form_and_graph_replay():
    """ContrastiveStep in mode (normalize, 0.1, exclude) at the ragged size: the first step's two losses against the fp64
    closed form on the HIP forward's own stacked embeddings (1e-4), and they differ from the default-mode losses; then three
    steps, GraphedStep(restore=True) replays against eager steps of a twin from the same state: losses, parameters and
    running buffers bit-identical."""
    from facl_amd.train_common import GraphedStep
    from facl_amd.utils_my import circle_contrast, global_contrast
    c = RAGGED
    B, G = c["B"], c["G"]
    r = np.random.RandomState(7)
    orders = [r.permutation(G) for _ in range(3)]
    kw = dict(normalize=True, temperature=0.1, mask="exclude")
    net, optim, step = make_contrastive_step(c, **STEP_MODE)
    assert step.loss_mode == kw
    loss, loss_c, loss_circle = step(points(c, 100), order=orders[0])
    torch.cuda.synchronize()
    loss, loss_c, loss_circle = loss.detach(), loss_c.detach(), loss_circle.detach()
    st = net._stacked.detach().double()
    rc = float(global_contrast(G, st[G * B:], st[:G * B], None, **kw))
    ro = float(circle_contrast(G, st[:G * B], B, order=orders[0], **kw))
    dc = float(global_contrast(G, st[G * B:], st[:G * B], None))
    print("step: loss_c %.6f (fp64 %.6f) loss_circle %.6f (fp64 %.6f); default-mode loss_c %.4f" % (float(loss_c), rc, float(loss_circle), ro, dc))
    assert abs(float(loss_c) - rc) < TOL * abs(rc) and abs(float(loss_circle) - ro) < TOL * abs(ro)
    assert abs(float(loss) - (rc + ro)) < TOL * abs(rc + ro)
    assert abs(rc - dc) > 1e-2 * abs(dc)                   # the mode reached the loss
    del net, optim, step

    net_g, opt_g, step_g = make_contrastive_step(c, **STEP_MODE)
    g = GraphedStep(step_g, points(c, 99), G, restore=True)
    net_t, opt_t, step_t = make_contrastive_step(c, **STEP_MODE)
    for k, order in enumerate(orders):
        pts = points(c, 100 + k)
        before = snapshot(net_g, opt_g)
        out_g = [t.detach().clone() for t in g(pts, order=order)]
        net_t.load_state_dict(before["net"])
        opt_t.load_state_dict(before["optim"])
        out_t = [t.detach().clone() for t in step_t(pts, order=order)]
        torch.cuda.synchronize()
        for a, b in zip(out_g, out_t):
            assert torch.isfinite(a).all() and torch.equal(a, b), (k, float(a), float(b))
        sd_g, sd_t = net_g.state_dict(), net_t.state_dict()
        for name in sd_g:
            assert torch.equal(sd_g[name], sd_t[name]), (k, name)


# ---- 7: the training entry -----------------------------------------------------------------------------------------------------
def test_train_entry_with_loss_flags(tmp_path, capsys):
    import re
    from facl_amd import cn3d_train_motion_GL as train
    args = ["--synthetic", "1", "--nepoch", "1", "--steps_per_epoch", "2", "--batchSize", "4", "--num_crop", "4", "--SAMPLE_NUM", "512"]
    losses = []
    for extra in (["--loss_normalize", "1", "--loss_temperature", "0.1", "--loss_mask", "exclude"], []):
        train.main(args + extra + ["--save_root_dir", str(tmp_path / ("ck%d" % len(losses)))])
        out = capsys.readouterr().out
        m = re.search(r"--loss: (\S+)", out)
        assert m, out
        losses.append(float(m.group(1)))
    assert all(np.isfinite(v) for v in losses), losses
    assert abs(losses[0] - losses[1]) > 1e-3 * abs(losses[1]), losses
