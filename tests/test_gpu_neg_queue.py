"""GPU tests of the cross-batch queue of negative keys (--neg_queue): the queue form of the fused pair loss
(facl_contrast_pair_queue), the device-side ring buffer (facl_queue_push), utils_my.contrastive_losses_stacked(queue=...), the
training step (eager and graph-replayed) and the training entry.  The fp64 truth is the device-agnostic closed form of utils_my
(held to materialised logits in test_neg_queue_cpu.py).  Bounds: those of test_gpu_loss_modes.py.  The whole module runs on
NaN-poisoned scratch."""

import numpy as np
import pytest
import torch

import neg_queue_paths
from helpers import snapshot
from poison import poisoned_scratch  # noqa: F401
from step_factory import make_contrastive_step, points

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LOSS_TOL, GRAD_TOL = 2e-6, 2e-5      # test_gpu_loss_modes.py
TOL = 1e-4                           # test_gpu_trajectory.py: losses of one step


def _state(head, valid):
    return torch.tensor([head, valid], dtype=torch.int32, device=DEV)


# ---- 1: the pair loss with a queue on synthetic similarity matrices ------------------------------------------------------------
def _pair_queue_closed_form(sim, sim_q, valid, G, B, Bk, order, off, mask):
    """(loss_c, loss_circle) of loss.hip on a ((G+1) B, G Bk) similarity matrix plus the first `valid` columns of a
    ((G+1) B, L) queue similarity matrix as extra negatives of every clip, in sim's dtype."""
    J = G * Bk
    col_clip = torch.arange(J, device=sim.device) % Bk
    same = col_clip[None, :] == (torch.arange(B, device=sim.device) + off)[:, None]              # (B, J)
    fill = torch.full((), 0.0 if mask == "zero" else float("-inf"), dtype=sim.dtype, device=sim.device)
    blocks = sim.view(G + 1, B, J)
    q = sim_q.view(G + 1, B, -1)[:, :, :valid]
    n = torch.arange(B, device=sim.device)
    lse_g = torch.logsumexp(torch.cat((torch.where(same, fill, blocks[G]), q[G]), dim=1), dim=1)
    pos_g = torch.stack([blocks[G][n, g * Bk + n + off] for g in range(G)])
    loss_c = (torch.logaddexp(pos_g, lse_g[None, :]) - pos_g).mean(dim=1).sum()
    order = [int(o) for o in order]
    neg = torch.cat([torch.where(same, fill, blocks[order[i]]) for i in range(G - 1)] + [q[order[i]] for i in range(G - 1)], dim=1)
    lse_o = torch.logsumexp(neg, dim=1)
    pos_o = torch.stack([blocks[order[i]][n, order[i + 1] * Bk + n + off] for i in range(G - 1)])
    loss_o = (torch.logaddexp(pos_o, lse_o[None, :]) - pos_o).mean(dim=1).sum()
    return loss_c, loss_o


def _fp32_yardstick(f, inputs64, ngrad):
    """Relative errors of a plain torch-fp32 evaluation of the closed form `f` against its fp64 evaluation on the same inputs:
    ((loss_c, loss_circle) errors, error of the gradient of loss_c + loss_circle wrt the first `ngrad` inputs, concatenated)."""
    outs, grads = [], []
    for dt in (torch.float64, torch.float32):
        xs = [t.detach().to(dt).requires_grad_(True) for t in inputs64]
        lc, lo = f(*xs)
        g = torch.autograd.grad(lc + lo, xs[:ngrad])
        outs.append((float(lc.detach()), float(lo.detach())))
        grads.append(torch.cat([t.double().reshape(-1) for t in g]))
    e_l = tuple(abs(a - b) / abs(b) for a, b in zip(outs[1], outs[0]))
    return e_l, float((grads[1] - grads[0]).norm() / grads[0].norm())


def _run_pair_queue(sim, sim_q, G, B, Bk, L, order, off, mask, state):
    from facl_amd import _lib
    from facl_amd.sa_mlp import _Workspace
    from facl_amd.utils_my import MASK_MODES
    lib = _lib.load_library()
    ws = _Workspace.get(torch.device(DEV))
    dsim, dsim_q = _lib.empty_like(sim), _lib.empty_like(sim_q)
    l64, l32 = _lib.empty(2, dtype=torch.float64, device=DEV), _lib.empty(3, device=DEV)
    _lib.check(lib.facl_contrast_pair_queue(_lib.ptr(sim), _lib.ptr(sim_q), G, B, Bk, G * Bk, L, _lib.ptr(order), off,
                                            MASK_MODES[mask], _lib.ptr(state), _lib.ptr(dsim), _lib.ptr(dsim_q), _lib.ptr(l64),
                                            _lib.ptr(l32), _lib.ptr(ws), _lib.stream()), "pair_queue")
    torch.cuda.synchronize()
    return dsim, dsim_q, l64, l32


def _synthetic(G, B, Bk, L, valid, filling):
    torch.manual_seed(G * 1000 + Bk + L)
    R, J = (G + 1) * B, G * Bk
    draw = (lambda *s: torch.randn(*s, device=DEV) * 2.0) if filling == "normal" else \
        (lambda *s: torch.rand(*s, device=DEV) * 6.0 - 203.0)
    sim, sim_q = draw(R, J), draw(R, L)
    sim_q[:, valid:] = float("nan")                          # columns >= valid are never used
    order = torch.as_tensor(np.random.RandomState(G).permutation(G), device=DEV)
    return sim, sim_q, order


# (G, B, Bk, off, L, valid) -> (chunks of sim, chunks of sim_q, 16-byte path) from the launcher's constants
# (neg_queue_paths reads them from csrc/loss.hip: 2048 columns per workgroup; the vector path needs J % 4 == L % 4 == 0 and
# 16-byte aligned matrices, which the allocator gives)
PAIR_CASES = {
    (6, 5, 5, 0, 20, 0): (1, 1, False), (6, 5, 5, 0, 20, 5): (1, 1, False), (6, 5, 5, 0, 20, 20): (1, 1, False),
    (4, 3, 6, 3, 12, 9): (1, 1, True),
    (24, 2, 48, 3, 64, 64): (1, 1, True),
    (2, 2, 1024, 5, 2048, 2048): (1, 1, True),               # J = L = CHUNK: the last size of one chunk each
    (2, 2, 1026, 5, 2052, 2049): (2, 2, True),               # one vector past it: ragged last chunks of 4, valid inside the second
    (3, 2, 682, 7, 2047, 2047): (1, 1, False),               # scalar path below the threshold
    (2, 2, 1025, 1000, 2051, 2050): (2, 2, False),           # scalar path above it: ragged last chunks of 2 and 3
}


@pytest.mark.parametrize("filling", ["normal", "minus200"])
@pytest.mark.parametrize("mask", ["zero", "exclude"])
@pytest.mark.parametrize("G,B,Bk,off,L,valid", list(PAIR_CASES))
def test_pair_queue_entry_on_synthetic_sim(G, B, Bk, off, L, valid, mask, filling):
    """facl_contrast_pair_queue against the fp64 closed form on the same fp32 similarities; sim_q is NaN from column `valid` on.
    Every element of dsim / dsim_q is written, dsim_q is exactly 0 from `valid` on, losses32 = [c, o, o + c]; with an empty
    queue the values agree with facl_contrast_pair_sum_mask within the same bounds (another summation order)."""
    from facl_amd import _lib
    from facl_amd.sa_mlp import _Workspace
    from facl_amd.utils_my import MASK_MODES
    J = G * Bk
    sim, sim_q, order = _synthetic(G, B, Bk, L, valid, filling)
    dsim, dsim_q, l64, l32 = _run_pair_queue(sim, sim_q, G, B, Bk, L, order, off, mask, _state(0, valid))
    assert neg_queue_paths.chunks(J, L) + (neg_queue_paths.vectorised(J, L, sim, sim_q, dsim, dsim_q),) == \
        PAIR_CASES[(G, B, Bk, off, L, valid)]
    s64, q64 = sim.double().requires_grad_(True), sim_q.double().requires_grad_(True)
    rc, ro = _pair_queue_closed_form(s64, q64, valid, G, B, Bk, order.tolist(), off, mask)
    gr, gq = torch.autograd.grad(rc + ro, (s64, q64))
    rc, ro = rc.detach(), ro.detach()
    e_c, e_o = abs(float(l64[0]) - float(rc)) / abs(float(rc)), abs(float(l64[1]) - float(ro)) / abs(float(ro))
    got, want = torch.cat((dsim, dsim_q), dim=1).double(), torch.cat((gr, gq), dim=1)
    e_g = float((got - want).norm() / want.norm())
    y_l, y_g = _fp32_yardstick(lambda s_, q_: _pair_queue_closed_form(s_, q_, valid, G, B, Bk, order.tolist(), off, mask),
                               (sim.double(), sim_q.double()), 2)
    print("pair+queue G=%d B=%d Bk=%d L=%d valid=%d %s %s: loss_c %.3e loss_circle %.3e [dsim|dsim_q] %.3e | torch-fp32 %.3e %.3e %.3e"
          % (G, B, Bk, L, valid, mask, filling, e_c, e_o, e_g, y_l[0], y_l[1], y_g))
    assert torch.isfinite(l64).all() and torch.isfinite(dsim).all() and torch.isfinite(dsim_q).all()
    assert e_c <= LOSS_TOL and e_o <= LOSS_TOL
    assert e_g <= GRAD_TOL
    assert int((dsim_q[:, valid:] != 0).sum()) == 0
    c, o = l64[0].float(), l64[1].float()
    assert torch.equal(l32, torch.stack((c, o, o + c)))
    if valid == 0:
        lib = _lib.load_library()
        ws = _Workspace.get(torch.device(DEV))
        d0 = _lib.empty_like(sim)
        m64, m32 = _lib.empty(2, dtype=torch.float64, device=DEV), _lib.empty(3, device=DEV)
        _lib.check(lib.facl_contrast_pair_sum_mask(_lib.ptr(sim), G, B, Bk, J, _lib.ptr(order), off, MASK_MODES[mask], _lib.ptr(d0),
                                                   _lib.ptr(m64), _lib.ptr(m32), _lib.ptr(ws), _lib.stream()), "pair_sum_mask")
        torch.cuda.synchronize()
        e_m = ((m64 - l64).abs() / m64.abs()).max()
        e_d = float((d0.double() - dsim.double()).norm() / d0.double().norm())
        print("  empty queue vs facl_contrast_pair_sum_mask: losses %.3e dsim %.3e" % (float(e_m), e_d))
        assert float(e_m) <= LOSS_TOL and e_d <= GRAD_TOL
        assert int((dsim_q != 0).sum()) == 0


@pytest.mark.parametrize("mask", ["zero", "exclude"])
def test_pair_queue_clamps_a_corrupt_state(mask):
    """valid = L + 7 behaves as L and valid = -3 as 0 (same bits): a corrupt state cannot address outside the matrices."""
    G, B, Bk, off, L = 4, 3, 6, 3, 12
    sim, sim_q, order = _synthetic(G, B, Bk, L, L, "normal")
    for bad, good in ((L + 7, L), (-3, 0)):
        a = _run_pair_queue(sim, sim_q, G, B, Bk, L, order, off, mask, _state(0, bad))
        b = _run_pair_queue(sim, sim_q, G, B, Bk, L, order, off, mask, _state(0, good))
        for x, y in zip(a, b):
            assert torch.isfinite(x).all() and torch.equal(x, y), (bad, good)


# ---- 2: the ring buffer ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,C,L", [(3, 8, 12), (5, 512, 20)])
def test_push_against_a_host_ring_model(P, C, L):
    from facl_amd.neg_queue import NegativeQueue
    torch.manual_seed(P + L)
    q = NegativeQueue(L, C, P, DEV)
    model = torch.zeros(L, C)
    head = valid = 0
    assert q.head_valid() == (0, 0) and int((q.buf != 0).sum()) == 0
    for k in range(L // P + 2):
        rows = torch.randn(P, C, device=DEV)
        q.push(rows)
        model[head:head + P] = rows.cpu()
        head, valid = (head + P) % L, min(valid + P, L)
        assert q.head_valid() == (head, valid), k
        assert torch.equal(q.buf.cpu(), model), k            # bitwise; slots never pushed stay 0
        assert torch.equal(q.valid_rows().cpu(), model[:valid])
    snap = q.snapshot()
    q.push(torch.randn(P, C, device=DEV))
    q.restore(snap)
    assert q.head_valid() == (head, valid) and torch.equal(q.buf.cpu(), model)
    q.restore()
    assert q.head_valid() == (0, 0) and int((q.buf != 0).sum()) == 0


def test_push_clamps_a_corrupt_head_and_refuses_bad_arguments():
    from facl_amd import _lib
    from facl_amd.neg_queue import NegativeQueue
    lib = _lib.load_library()
    P, C, L = 3, 8, 12
    rows = torch.randn(P, C, device=DEV)
    for bad_head, slot in ((7, 6), (-5, 0), (100, 9), (12, 9)):           # a multiple of P below L
        q = NegativeQueue(L, C, P, DEV)
        q.state.copy_(_state(bad_head, 40))
        q.push(rows)
        want = torch.zeros(L, C, device=DEV)
        want[slot:slot + P] = rows
        assert torch.equal(q.buf, want), bad_head
        assert q.head_valid() == ((slot + P) % L, L), bad_head
    q = NegativeQueue(L, C, P, DEV)
    call = lambda r, P_, C_, b, L_, s: lib.facl_queue_push(_lib.ptr(r), P_, C_, _lib.ptr(b), L_, _lib.ptr(s), _lib.stream())
    assert call(rows, P, C, q.buf, 10, q.state) == -1                      # L % P
    assert call(rows, P, 6, q.buf, L, q.state) == -1                       # C % 4
    # NULL pointers: FACL_E_NULL (-2), the code of every entry of include/facl_hip.h for them
    assert call(None, P, C, q.buf, L, q.state) == -2 and call(rows, P, C, None, L, q.state) == -2
    assert call(rows, P, C, q.buf, L, None) == -2
    torch.cuda.synchronize()
    assert q.head_valid() == (0, 0) and int((q.buf != 0).sum()) == 0       # nothing was launched


# ---- 3: contrastive_losses_stacked(queue=...) ---------------------------------------------------------------------------------
MODES = [(True, 0.07, "exclude"), (True, 0.2, "zero"), (False, 4.0, "exclude"), (False, 1.0, "zero")]


@pytest.mark.parametrize("normalize,tau,mask", MODES)
@pytest.mark.parametrize("G,B,C,L,pushes", [(6, 5, 32, 15, 2), (10, 4, 512, 16, 3)])
def test_stacked_losses_with_queue_vs_closed_form_fp64(G, B, C, L, pushes, normalize, tau, mask):
    """Row pass + both similarity GEMMs + queue pair loss + their backward against the fp64 closed form with the queue's valid
    rows: both values and the gradient wrt the stacked embeddings.  (6, 5, 32) with L = 15: library GEMMs and the scalar
    kernels; (10, 4, 512) with L = 16: the MFMA GEMMs and the 16-byte kernels.  The queue is partly filled and not written."""
    from facl_amd.neg_queue import NegativeQueue
    from facl_amd.utils_my import circle_contrast, contrastive_losses_stacked, global_contrast
    torch.manual_seed(G * B + C)
    x0 = (torch.randn(G * B, C, dtype=torch.float64) * 0.3).to(DEV)
    xg0 = (torch.randn(B, C, dtype=torch.float64) * 0.3).to(DEV)
    order = np.random.RandomState(1).permutation(G)
    kw = dict(normalize=normalize, temperature=tau, mask=mask)
    q = NegativeQueue(L, C, B, DEV)
    for _ in range(pushes):
        q.push(torch.randn(B, C, device=DEV) * (1.0 if normalize else 0.3))
    assert q.head_valid()[1] == pushes * B < L
    rows64 = q.valid_rows().double()
    buf0, state0 = q.buf.clone(), q.state.clone()

    def truth(xg, x):
        return (global_contrast(G, xg, x, None, queue=rows64.to(x.dtype), **kw),
                circle_contrast(G, x, B, order=order, queue=rows64.to(x.dtype), **kw))

    xg64, x64 = xg0.clone().requires_grad_(True), x0.clone().requires_grad_(True)
    lc_r, lo_r = truth(xg64, x64)
    gr = torch.autograd.grad(0.7 * lc_r + 1.3 * lo_r, (xg64, x64))
    lc_r, lo_r = lc_r.detach(), lo_r.detach()
    lc_0 = float(global_contrast(G, xg0, x0, None, **kw))
    st = torch.cat((x0, xg0), 0).float().requires_grad_(True)
    lc, lo = contrastive_losses_stacked(G, st, order, queue=q, **kw)
    (0.7 * lc + 1.3 * lo).backward()                        # distinct upstream gradients exercise facl_scale_rows2
    g = st.grad.double()
    e = (abs(float(lc.detach()) - float(lc_r)) / abs(float(lc_r)), abs(float(lo.detach()) - float(lo_r)) / abs(float(lo_r)),
         float((g[:G * B] - gr[1]).norm() / gr[1].norm()), float((g[G * B:] - gr[0]).norm() / gr[0].norm()))
    y_l, y_g = _fp32_yardstick(lambda x_, xg_: truth(xg_, x_), (x0, xg0), 1)
    print("stacked+queue G=%d B=%d C=%d L=%d %s: loss_c %.3e loss_circle %.3e dx %.3e dxg %.3e | torch-fp32 %.3e %.3e dx %.3e"
          % (G, B, C, L, (normalize, tau, mask), *e, y_l[0], y_l[1], y_g))
    assert torch.isfinite(g).all()
    assert e[0] <= LOSS_TOL and e[1] <= LOSS_TOL
    assert e[2] < GRAD_TOL and e[3] < GRAD_TOL
    assert float(lc_r) > lc_0                                # the queue reached the loss
    assert torch.equal(q.buf, buf0) and torch.equal(q.state, state0)       # forward and backward leave the queue as it was


# ---- 4: identity ------------------------------------------------------------------------------------------------------------------
def test_no_queue_is_bit_identical():
    """queue=None is the call without the keyword, bit for bit (values and gradient)."""
    from facl_amd.utils_my import contrastive_losses_stacked
    G, B, C = 6, 5, 32
    torch.manual_seed(5)
    st0 = torch.randn((G + 1) * B, C, device=DEV) * 0.3
    order = np.random.RandomState(2).permutation(G)
    res = []
    for kw in ({}, dict(queue=None)):
        st = st0.clone().requires_grad_(True)
        lc, lo, ls = contrastive_losses_stacked(G, st, order, with_sum=True, **kw)
        (0.7 * lc + 1.3 * lo).backward()
        res.append((lc.detach(), lo.detach(), ls.detach(), st.grad))
    for a, b in zip(*res):
        assert torch.isfinite(a).all() and torch.equal(a, b)


# ---- 5: the training step ------------------------------------------------------------------------------------------------------
RAGGED = dict(B=3, G=5, N=1000, D=3)                       # config `ragged` of test_gpu_trajectory.py
STEP_MODE = dict(loss_normalize=1, loss_temperature=0.1, loss_mask="exclude")
KW = dict(normalize=True, temperature=0.1, mask="exclude")


def _key_rows(net, G, B):
    """The rows a step stores: x_global of the step's stacked output after the row map of the step's mode, in fp32."""
    from facl_amd.utils_my import loss_rows
    return loss_rows(net._stacked.detach(), KW["normalize"], KW["temperature"])[G * B:].clone()


def test_step_with_neg_queue_zero_is_bit_identical():
    """A step built with neg_queue=0 is the step built without the flag: losses and parameters, two steps."""
    c = RAGGED
    orders = [np.random.RandomState(3).permutation(c["G"]) for _ in range(2)]
    res = []
    for flags in ({}, dict(neg_queue=0)):
        net, optim, step = make_contrastive_step(c, **STEP_MODE, **flags)
        assert step.queue is None
        outs = []
        for k, order in enumerate(orders):
            outs += [t.detach().clone() for t in step(points(c, 100 + k), order=order)]
        torch.cuda.synchronize()
        assert step.queue is None
        res.append(outs + [v.detach().clone() for v in net.state_dict().values()])
    assert len(res[0]) == len(res[1])
    for a, b in zip(*res):
        assert torch.equal(a, b)


def test_step_with_queue_vs_closed_form_and_graph_replay():
    """ContrastiveStep with neg_queue=6 in mode (normalize, 0.1, exclude) at the ragged size.  Step 1 (empty queue) equals the
    closed form without a queue; step 2 equals the fp64 closed form with the three rows step 1 pushed, on the step's own stacked
    embeddings, and differs from the queue-less form by more than 10 TOL; after step 3 the ring has wrapped and holds the rows
    of steps 3 and 2.  Then four steps of GraphedStep(restore=True) against eager steps of a twin from the same state: losses,
    parameters, running buffers, queue contents and (head, valid) bit-identical; the graphed step starts from an empty queue."""
    from facl_amd.train_common import GraphedStep
    from facl_amd.utils_my import circle_contrast, global_contrast
    c = RAGGED
    B, G = c["B"], c["G"]
    r = np.random.RandomState(7)
    orders = [r.permutation(G) for _ in range(4)]
    net, optim, step = make_contrastive_step(c, neg_queue=6, **STEP_MODE)
    assert step.loss_mode == KW and step.neg_queue == 6 and step.queue is None
    pushed = []
    for k in range(3):
        loss, loss_c, loss_circle = [t.detach().clone() for t in step(points(c, 100 + k), order=orders[k])]
        torch.cuda.synchronize()
        st = net._stacked.detach().double()
        rows = torch.cat(pushed[-2:][::-1]).double() if pushed else None     # what the queue held during this step
        rc = float(global_contrast(G, st[G * B:], st[:G * B], None, queue=rows, **KW))
        ro = float(circle_contrast(G, st[:G * B], B, order=orders[k], queue=rows, **KW))
        nc = float(global_contrast(G, st[G * B:], st[:G * B], None, **KW))
        no = float(circle_contrast(G, st[:G * B], B, order=orders[k], **KW))
        print("step %d: loss_c %.6f (fp64 %.6f, without queue %.6f) loss_circle %.6f (fp64 %.6f, without queue %.6f)"
              % (k + 1, float(loss_c), rc, nc, float(loss_circle), ro, no))
        assert abs(float(loss_c) - rc) < TOL * abs(rc) and abs(float(loss_circle) - ro) < TOL * abs(ro)
        assert abs(float(loss) - (rc + ro)) < TOL * abs(rc + ro)
        if k == 0:
            assert rc == nc and ro == no
        else:                                               # the queue reached the loss
            assert abs(rc - nc) > 10 * TOL * abs(nc) and abs(ro - no) > 10 * TOL * abs(no)
        pushed.append(_key_rows(net, G, B))
        assert step.queue.head_valid() == ((3 * (k + 1)) % 6, min(3 * (k + 1), 6))
    # wrapped: slots 0..2 hold step 3's rows, slots 3..5 step 2's (recomputed from net._stacked through the row pass: same kernel)
    assert torch.equal(step.queue.buf, torch.cat((pushed[2], pushed[1])))
    del net, optim, step

    net_g, opt_g, step_g = make_contrastive_step(c, neg_queue=6, **STEP_MODE)
    g = GraphedStep(step_g, points(c, 99), G, restore=True)
    assert step_g.queue is not None and step_g.queue.head_valid() == (0, 0) and int((step_g.queue.buf != 0).sum()) == 0
    net_t, opt_t, step_t = make_contrastive_step(c, neg_queue=6, **STEP_MODE)
    for k, order in enumerate(orders):
        pts = points(c, 100 + k)
        before = snapshot(net_g, opt_g)
        qsnap = step_g.queue.snapshot()
        out_g = [t.detach().clone() for t in g(pts, order=order)]
        net_t.load_state_dict(before["net"])
        opt_t.load_state_dict(before["optim"])
        if step_t.queue is not None:
            step_t.queue.restore(qsnap)
        out_t = [t.detach().clone() for t in step_t(pts, order=order)]
        torch.cuda.synchronize()
        for a, b in zip(out_g, out_t):
            assert torch.isfinite(a).all() and torch.equal(a, b), (k, float(a), float(b))
        sd_g, sd_t = net_g.state_dict(), net_t.state_dict()
        for name in sd_g:
            assert torch.equal(sd_g[name], sd_t[name]), (k, name)
        assert torch.equal(step_g.queue.buf, step_t.queue.buf), k
        assert step_g.queue.head_valid() == step_t.queue.head_valid() == ((3 * (k + 1)) % 6, min(3 * (k + 1), 6)), k


# ---- 6: the training entry ------------------------------------------------------------------------------------------------------
def test_train_entry_with_neg_queue(tmp_path, capsys):
    import re
    from facl_amd import cn3d_train_motion_GL as train
    args = ["--synthetic", "1", "--nepoch", "1", "--steps_per_epoch", "3", "--batchSize", "4", "--num_crop", "4", "--SAMPLE_NUM", "512"]
    losses = []
    for extra in (["--neg_queue", "8"], []):
        train.main(args + extra + ["--save_root_dir", str(tmp_path / ("ck%d" % len(losses)))])
        out = capsys.readouterr().out
        m = re.search(r"--loss: (\S+)", out)
        assert m, out
        losses.append(float(m.group(1)))
    print("entry: mean loss with --neg_queue 8 %.6f, without %.6f" % tuple(losses))
    assert all(np.isfinite(v) for v in losses), losses
    assert abs(losses[0] - losses[1]) > 1e-3 * abs(losses[1]), losses
