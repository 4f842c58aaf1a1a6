"""GPU tests of class-mates as extra positives of the global / circle losses (--loss_mask class --class_positives w): the three
kernel forms (facl_contrast_pair_sum_sup on the register-cached and the streaming kernel, facl_contrast_pair_queue_sup),
utils_my.contrastive_losses_stacked(class_positives=), the training step (eager and graph-replayed) and the training entry with
--resume.  The fp64 truth is built here from the contract: the class mask's log-sum-exp, the own slots' terms, and the class
cells' mean term times w nS.  Inputs, runners and bounds are those of test_gpu_loss_class.py (LOSS_TOL, GRAD_TOL:
test_gpu_loss_modes.py; TOL: test_gpu_trajectory.py).  The whole module runs on NaN-poisoned scratch."""
import os
import re

import numpy as np
import pytest
import torch

import test_gpu_loss_class as base
from helpers import snapshot
from test_gpu_loss_class import (DEV, GRAD_TOL, LOSS_TOL, PAIR_SHAPES, QUEUE_CASES, TOL, _every_anchor_keeps_a_negative, _i32, _ids,
                                 _masks, _positive_cells, _rel, _sim, _state)
from poison import poisoned_scratch  # noqa: F401
from step_factory import points
from synth_tree import assert_same_state, write_tree

pytestmark = pytest.mark.gpu
WEIGHTS = [1.0, 0.25]


# ---- the truth on a similarity matrix -----------------------------------------------------------------------------------------
def _cells(G, B, Bk, off, cls, qcls, valid):
    """(cell (B, J), qcell (B, valid)): the class cells of an anchor row of clip n -- what the class mask removes for a reason
    other than "own clip"."""
    masked, qmasked = _masks(G, B, Bk, off, cls, qcls, valid)
    own = (torch.arange(G * Bk, device=DEV) % Bk)[None, :] == (torch.arange(B, device=DEV) + off)[:, None]
    return masked & ~own, qmasked


def _closed_form(sim, sim_q, valid, G, B, Bk, order, off, cls, qcls, lam):
    """(loss_c, loss_circle) of the contract in sim's dtype: test_gpu_loss_class._closed_form's value (negatives, lse and own
    slots as under the class mask) plus, per clip with |C| > 0 and a negative, lam nS / |C| times the sum of
    logaddexp(v, lse) - v over its class cells, divided by B."""
    J = G * Bk
    masked, qmasked = _masks(G, B, Bk, off, cls, qcls, valid)
    cell, qcell = _cells(G, B, Bk, off, cls, qcls, valid)
    fill = torch.full((), base.NINF, dtype=sim.dtype, device=sim.device)
    zero = torch.zeros((), dtype=sim.dtype, device=sim.device)
    blocks = sim.view(G + 1, B, J)
    q = None if sim_q is None else sim_q.view(G + 1, B, -1)[:, :, :valid]
    raw = lambda g: blocks[g] if q is None else torch.cat((blocks[g], q[g]), dim=1)
    m_all = masked if q is None else torch.cat((masked, qmasked), dim=1)
    c_all = cell if q is None else torch.cat((cell, qcell), dim=1)
    order = [int(o) for o in order]

    def extra(rows, lse, empty, nS):
        vals = torch.cat([raw(g) for g in rows], dim=1)
        cm = c_all.repeat(1, len(rows))
        use = cm & ~empty[:, None]
        v, l = torch.where(use, vals, zero), torch.where(use, lse[:, None].expand_as(vals), zero)
        t = torch.where(use, torch.logaddexp(v, l) - v, zero).sum(dim=1)
        cnt = cm.sum(dim=1)
        return torch.where(cnt > 0, lam * nS / cnt.clamp_min(1).to(sim.dtype) * t, zero).sum() / B

    rc, ro = base._closed_form(sim, sim_q, valid, G, B, Bk, order, off, cls, qcls)
    lse_g, empty_g = base._lse_or_empty(torch.where(m_all, fill, raw(G)))
    lse_o, empty_o = base._lse_or_empty(torch.cat([torch.where(m_all, fill, raw(order[i])) for i in range(G - 1)], dim=1))
    return rc + extra([G], lse_g, empty_g, G), ro + extra(order[:G - 1], lse_o, empty_o, G - 1)


def _anchor_rows(G, B, order):
    """bool ((G+1) B,): rows that are an anchor of some loss (all but block order[G-1])."""
    rows = torch.ones((G + 1) * B, dtype=torch.bool, device=DEV)
    last = int(order[G - 1])
    rows[last * B:(last + 1) * B] = False
    return rows


def _run_pair(sim, G, B, Bk, order, off, cls, lam):
    """facl_contrast_pair_sum_sup: (dsim, losses, losses32)."""
    from facl_amd import _lib
    from facl_amd.sa_mlp import _Workspace
    lib = _lib.load_library()
    ws = _Workspace.get(torch.device(DEV))
    dsim = _lib.empty_like(sim)
    l64, l32 = _lib.empty(2, dtype=torch.float64, device=DEV), _lib.empty(3, device=DEV)
    _lib.check(lib.facl_contrast_pair_sum_sup(_lib.ptr(sim), G, B, Bk, G * Bk, _lib.ptr(order), off, _lib.ptr(cls), lam, _lib.ptr(dsim),
                                              _lib.ptr(l64), _lib.ptr(l32), _lib.ptr(ws), _lib.stream()), "pair_sum_sup")
    torch.cuda.synchronize()
    return dsim, l64, l32


def _run_queue(sim, sim_q, G, B, Bk, L, order, off, state, cls, qcls, lam):
    """facl_contrast_pair_queue_sup: (dsim, dsim_q, losses, losses32)."""
    from facl_amd import _lib
    from facl_amd.sa_mlp import _Workspace
    lib = _lib.load_library()
    ws = _Workspace.get(torch.device(DEV))
    dsim, dsim_q = _lib.empty_like(sim), _lib.empty_like(sim_q)
    l64, l32 = _lib.empty(2, dtype=torch.float64, device=DEV), _lib.empty(3, device=DEV)
    _lib.check(lib.facl_contrast_pair_queue_sup(_lib.ptr(sim), _lib.ptr(sim_q), G, B, Bk, G * Bk, L, _lib.ptr(order), off,
                                                _lib.ptr(cls), _lib.ptr(qcls), _lib.ptr(state), lam, _lib.ptr(dsim), _lib.ptr(dsim_q),
                                                _lib.ptr(l64), _lib.ptr(l32), _lib.ptr(ws), _lib.stream()), "pair_queue_sup")
    torch.cuda.synchronize()
    return dsim, dsim_q, l64, l32


# ---- 1: the pair entry on synthetic similarities --------------------------------------------------------------------------------
@pytest.mark.parametrize("lam", WEIGHTS)
@pytest.mark.parametrize("filling", ["normal", "minus200"])
@pytest.mark.parametrize("G,B,Bk,off", PAIR_SHAPES)
def test_pair_sup_entry_on_synthetic_sim(G, B, Bk, off, filling, lam):
    J = G * Bk
    if G == 24:
        assert (G - 1) * J > 24 * 1024                      # the streaming kernel
    sim, order = _sim(G, B, Bk, filling)
    cls = _ids(Bk)
    local = cls.tolist()[off:off + B]
    cell = _cells(G, B, Bk, off, cls, None, 0)[0]
    assert _every_anchor_keeps_a_negative(cls, B, Bk, off)
    assert bool(cell.any()) and any(c < 0 for c in local)    # an anchor with class cells, an anchor with an unknown id
    if (G, B, Bk, off) == (4, 3, 6, 3):                      # the mates lie outside the local shard
        col_clip = torch.arange(J, device=DEV) % Bk
        assert not bool(cell[:, (col_clip >= off) & (col_clip < off + B)].any())
    dsim, l64, l32 = _run_pair(sim, G, B, Bk, order, off, cls, lam)
    s64 = sim.double().requires_grad_(True)
    rc, ro = _closed_form(s64, None, 0, G, B, Bk, order.tolist(), off, cls, None, lam)
    (gr,) = torch.autograd.grad(rc + ro, s64)
    e_c, e_o, e_g = _rel(l64[0], rc.detach()), _rel(l64[1], ro.detach()), float((dsim.double() - gr).norm() / gr.norm())
    print("pair sup G=%d B=%d Bk=%d %s w=%g: loss_c %.3e loss_circle %.3e dsim %.3e" % (G, B, Bk, filling, lam, e_c, e_o, e_g))
    assert torch.isfinite(l64).all() and torch.isfinite(dsim).all()
    assert e_c <= LOSS_TOL and e_o <= LOSS_TOL
    assert e_g <= GRAD_TOL
    cells = cell.repeat(G + 1, 1) & _anchor_rows(G, B, order)[:, None]
    assert int(cells.sum()) > 0 and int((dsim[cells] == 0).sum()) == 0          # every class cell carries a gradient ...
    assert int((dsim[cells] > 0).sum()) == 0                                    # ... a pull: d term / d v < 0
    own = (_masks(G, B, Bk, off, cls, None, 0)[0] & ~cell).repeat(G + 1, 1)
    assert int((dsim[own & ~_positive_cells(G, B, Bk, order, off)] != 0).sum()) == 0
    last = int(order[G - 1])
    assert int((dsim[last * B:(last + 1) * B] != 0).sum()) == 0                 # the view that is no anchor
    c, o = l64[0].float(), l64[1].float()
    assert torch.equal(l32, torch.stack((c, o, o + c)))
    m64 = base._run_pair(sim, G, B, Bk, order, off, cls)[1]                     # the class mask on the same inputs: below
    assert float(l64[0]) > float(m64[0]) and float(l64[1]) > float(m64[1])


# ---- 2: without a class cell the entry is exclude, bit for bit --------------------------------------------------------------------
@pytest.mark.parametrize("ids", ["unknown", "distinct"])
@pytest.mark.parametrize("G,B,Bk,off", PAIR_SHAPES)
def test_pair_sup_identities_with_exclude(G, B, Bk, off, ids):
    sim, order = _sim(G, B, Bk, "normal")
    cls = _i32([-1 - k % 3 for k in range(Bk)]) if ids == "unknown" else _i32(np.random.RandomState(Bk).permutation(Bk) + 5)
    want = base._run_pair(sim, G, B, Bk, order, off)
    for lam in WEIGHTS:
        for a, b in zip(_run_pair(sim, G, B, Bk, order, off, cls, lam), want):
            assert torch.isfinite(a).all() and torch.equal(a, b)


# ---- 3: no negative at all: every other cell is a class cell, and all of it is 0 ---------------------------------------------------
@pytest.mark.parametrize("filling", ["normal", "minus200"])
@pytest.mark.parametrize("G,B,Bk,off", PAIR_SHAPES)
def test_pair_sup_one_class_is_exactly_zero(G, B, Bk, off, filling):
    sim, order = _sim(G, B, Bk, filling)
    dsim, l64, l32 = _run_pair(sim, G, B, Bk, order, off, _i32([4] * Bk), 1.0)
    assert torch.isfinite(dsim).all() and torch.isfinite(l64).all() and torch.isfinite(l32).all()
    assert not l64.any() and not l32.any() and not dsim.any()


# ---- 4: the queue form ---------------------------------------------------------------------------------------------------------------
def _queue_case_ids(Bk, B, off, L, valid):
    """Ids with in-batch mates at every size of QUEUE_CASES (test_gpu_loss_class's _ids(3) and _ids(4) have none), and the queue
    ids of that file: 0, 1, 2, -1, ... below `valid`, the first known local class from there on."""
    cls = _i32({3: [1, 0, 1], 4: [2, 1, 2, -1]}.get(Bk) or _ids(Bk).tolist())
    return cls, base._queue_ids(cls, B, off, L, valid)


@pytest.mark.parametrize("lam", WEIGHTS)
@pytest.mark.parametrize("filling", ["normal", "minus200"])
@pytest.mark.parametrize("G,B,Bk,off,L,valid", QUEUE_CASES)
def test_pair_queue_sup_entry_on_synthetic_sim(G, B, Bk, off, L, valid, filling, lam):
    import neg_queue_paths
    J = G * Bk
    sim, sim_q, order = _sim(G, B, Bk, filling, L, valid)
    cls, qcls = _queue_case_ids(Bk, B, off, L, valid)
    cell, qcell = _cells(G, B, Bk, off, cls, qcls, valid)
    assert _every_anchor_keeps_a_negative(cls, B, Bk, off)
    assert bool(cell.any())                                  # class cells in sim ...
    if valid:
        assert bool(qcell.any()) and not bool(qcell.all())   # ... AND in sim_q
    if L == 2052:
        assert bool(qcell[:, 2048:].any())                   # one in the queue's second chunk
    if valid < L:                                            # an anchor's class also sits at columns >= valid: it must change nothing
        known = [c for c in cls.tolist()[off:off + B] if c >= 0]
        assert all(c == known[0] for c in qcls.tolist()[valid:])
    dsim, dsim_q, l64, l32 = _run_queue(sim, sim_q, G, B, Bk, L, order, off, _state(0, valid), cls, qcls, lam)
    assert neg_queue_paths.vectorised(J, L, sim, sim_q, dsim, dsim_q, qcls) == (L == 2052 or L == 8)
    assert neg_queue_paths.chunks(J, L) == ((2, 1) if J == 2304 else (1, 2) if L == 2052 else (1, 1))
    s64, q64 = sim.double().requires_grad_(True), sim_q.double().requires_grad_(True)
    rc, ro = _closed_form(s64, q64, valid, G, B, Bk, order.tolist(), off, cls, qcls, lam)
    gr, gq = torch.autograd.grad(rc + ro, (s64, q64))
    got, want = torch.cat((dsim, dsim_q), dim=1).double(), torch.cat((gr, gq), dim=1)
    e_c, e_o, e_g = _rel(l64[0], rc.detach()), _rel(l64[1], ro.detach()), float((got - want).norm() / want.norm())
    print("pair+queue sup G=%d B=%d Bk=%d L=%d valid=%d %s w=%g: loss_c %.3e loss_circle %.3e [dsim|dsim_q] %.3e"
          % (G, B, Bk, L, valid, filling, lam, e_c, e_o, e_g))
    assert torch.isfinite(l64).all() and torch.isfinite(dsim).all() and torch.isfinite(dsim_q).all()
    assert e_c <= LOSS_TOL and e_o <= LOSS_TOL
    assert e_g <= GRAD_TOL
    anchors = _anchor_rows(G, B, order)[:, None]
    assert int((dsim[cell.repeat(G + 1, 1) & anchors] == 0).sum()) == 0
    assert int((dsim_q[:, :valid][qcell.repeat(G + 1, 1) & anchors] == 0).sum()) == 0
    own = (_masks(G, B, Bk, off, cls, None, 0)[0] & ~cell).repeat(G + 1, 1)
    assert int((dsim[own & ~_positive_cells(G, B, Bk, order, off)] != 0).sum()) == 0
    assert int((dsim_q[:, valid:] != 0).sum()) == 0
    last = int(order[G - 1])
    assert int((dsim[last * B:(last + 1) * B] != 0).sum()) == 0 and int((dsim_q[last * B:(last + 1) * B] != 0).sum()) == 0
    c, o = l64[0].float(), l64[1].float()
    assert torch.equal(l32, torch.stack((c, o, o + c)))


# the last column: what facl_contrast_pair_sum_sup launches for the shape
@pytest.mark.parametrize("G,B,Bk,off,L,pair_kernel", [(4, 3, 3, 0, 6, "register"), (4, 4, 4, 0, 2052, "register"),
                                                      (24, 2, 96, 3, 8, "streaming")])
def test_pair_queue_sup_with_an_empty_queue_is_the_pair_entry(G, B, Bk, off, L, pair_kernel):
    """valid = 0: the rule of test_gpu_loss_class.py's empty-queue test.  Where the pair entry runs the register-cached kernel
    both sides sum exp(), the slots' and the class cells' terms and d/dlse shares in fp64 and round once: bit for bit.  At
    (24, 2, 96, 3, 8) the pair entry runs the streaming kernel, which sums the own slots' d/dlse serially in fp32: the
    tolerances, for the reason written there."""
    assert ((G - 1) * G * Bk <= 24 * 1024) == (pair_kernel == "register")
    sim, sim_q, order = _sim(G, B, Bk, "normal", L, 0)
    cls, qcls = _queue_case_ids(Bk, B, off, L, 0)
    assert bool(_cells(G, B, Bk, off, cls, None, 0)[0].any())
    for lam in WEIGHTS:
        dsim, dsim_q, l64, l32 = _run_queue(sim, sim_q, G, B, Bk, L, order, off, _state(0, 0), cls, qcls, lam)
        d0, m64, m32 = _run_pair(sim, G, B, Bk, order, off, cls, lam)
        e_l = float(((m64 - l64).abs() / m64.abs()).max())
        e_d = float((d0.double() - dsim.double()).norm() / d0.double().norm())
        print("empty queue vs facl_contrast_pair_sum_sup G=%d Bk=%d L=%d w=%g (%s): losses %.3e dsim %.3e, %d of %d dsim elements differ"
              % (G, Bk, L, lam, pair_kernel, e_l, e_d, int((d0 != dsim).sum()), dsim.numel()))
        assert torch.isfinite(dsim).all() and torch.isfinite(l64).all()
        assert int((dsim_q != 0).sum()) == 0
        assert torch.equal(dsim == 0, d0 == 0)
        if pair_kernel == "register":
            assert torch.equal(l64, m64) and torch.equal(l32, m32)
            assert torch.equal(dsim, d0)
        else:
            assert e_l <= LOSS_TOL and e_d <= GRAD_TOL
            c, o = l64[0].float(), l64[1].float()
            assert torch.equal(l32, torch.stack((c, o, o + c)))


@pytest.mark.parametrize("G,B,Bk,off,L,valid", [c for c in QUEUE_CASES if c[5] > 0])
def test_pair_queue_sup_with_unknown_ids_is_the_exclude_queue(G, B, Bk, off, L, valid):
    """Every id of cls < 0: facl_contrast_pair_queue(..., exclude) bit for bit, whatever qcls holds."""
    sim, sim_q, order = _sim(G, B, Bk, "normal", L, valid)
    cls = _i32([-1 - k % 3 for k in range(Bk)])
    qcls = _i32([k % 4 - 2 for k in range(L)])
    want = base._run_queue(sim, sim_q, G, B, Bk, L, order, off, _state(0, valid))
    for a, b in zip(_run_queue(sim, sim_q, G, B, Bk, L, order, off, _state(0, valid), cls, qcls, 1.0), want):
        assert torch.isfinite(a).all() and torch.equal(a, b)


@pytest.mark.parametrize("G,B,Bk,off,L,valid", [(4, 3, 3, 0, 6, 3), (4, 4, 4, 0, 2052, 2050), (24, 2, 96, 3, 8, 8)])
def test_pair_queue_sup_one_class_is_exactly_zero(G, B, Bk, off, L, valid):
    """One class in cls and in qcls: no negative anywhere while every live cell off the own clip is a class cell."""
    sim, sim_q, order = _sim(G, B, Bk, "normal", L, valid)
    out = _run_queue(sim, sim_q, G, B, Bk, L, order, off, _state(0, valid), _i32([1] * Bk), _i32([1] * L), 1.0)
    for t in out:
        assert torch.isfinite(t).all() and not t.any()


# ---- 5: contrastive_losses_stacked(mask='class', class_positives=) ------------------------------------------------------------------
@pytest.mark.parametrize("with_queue", [False, True])
@pytest.mark.parametrize("normalize,tau", [(True, 0.07), (False, 4.0)])
@pytest.mark.parametrize("G,B,C,L", [(6, 5, 32, 15), (10, 4, 512, 16)])
def test_stacked_losses_with_class_positives_vs_closed_form_fp64(G, B, C, L, normalize, tau, with_queue):
    """Row pass + similarity GEMMs + pair loss with class positives + their backward against the fp64 closed forms of utils_my:
    both values and the gradient wrt the stacked embeddings.  (6, 5, 32): library GEMMs and the scalar kernels; (10, 4, 512):
    MFMA GEMMs and the 16-byte kernels."""
    from facl_amd.neg_queue import NegativeQueue
    from facl_amd.utils_my import circle_contrast, contrastive_losses_stacked, global_contrast
    lam = 0.5
    torch.manual_seed(G * B + C)
    x0 = (torch.randn(G * B, C, dtype=torch.float64) * 0.3).to(DEV)
    xg0 = (torch.randn(B, C, dtype=torch.float64) * 0.3).to(DEV)
    order = np.random.RandomState(1).permutation(G)
    cls = _i32([0, 1, 0, -1, 2][:B])                        # clips 0 and 2 are mates
    assert _every_anchor_keeps_a_negative(cls, B, B, 0)
    q = rows64 = qids = None
    if with_queue:
        q = NegativeQueue(L, C, B, DEV, with_ids=True)
        for k in range(2):
            q.push(torch.randn(B, C, device=DEV) * (1.0 if normalize else 0.3), ids=_i32([(k + 2 * i) % 4 - 1 for i in range(B)]))
        rows64, qids = q.valid_rows().double(), q.valid_ids()
        assert rows64.shape[0] == 2 * B < L and 0 in qids.tolist() and 1 in qids.tolist()
        before = q.snapshot()
    kw = dict(normalize=normalize, temperature=tau)

    def truth(xg, x, w):
        ck = dict(key_classes=cls, queue_classes=qids, class_positives=w)
        qr = None if rows64 is None else rows64.to(x.dtype)
        return (global_contrast(G, xg, x, None, queue=qr, mask="class", **kw, **ck),
                circle_contrast(G, x, B, order=order, queue=qr, mask="class", **kw, **ck))

    xg64, x64 = xg0.clone().requires_grad_(True), x0.clone().requires_grad_(True)
    lc_r, lo_r = truth(xg64, x64, lam)
    gr = torch.autograd.grad(0.7 * lc_r + 1.3 * lo_r, (xg64, x64))
    lc_r, lo_r = lc_r.detach(), lo_r.detach()
    st = torch.cat((x0, xg0), 0).float().requires_grad_(True)
    lc, lo = contrastive_losses_stacked(G, st, order, mask="class", classes=cls, queue=q, class_positives=lam, **kw)
    (0.7 * lc + 1.3 * lo).backward()                        # distinct upstream gradients exercise facl_scale_rows2
    g = st.grad.double()
    e = (_rel(lc.detach(), lc_r), _rel(lo.detach(), lo_r),
         float((g[:G * B] - gr[1]).norm() / gr[1].norm()), float((g[G * B:] - gr[0]).norm() / gr[0].norm()))
    print("stacked sup G=%d B=%d C=%d queue=%d %s: loss_c %.3e loss_circle %.3e dx %.3e dxg %.3e" % (G, B, C, with_queue, (normalize, tau), *e))
    assert torch.isfinite(g).all()
    assert e[0] <= LOSS_TOL and e[1] <= LOSS_TOL
    assert e[2] < GRAD_TOL and e[3] < GRAD_TOL
    lc_m, lo_m = truth(xg0, x0, 0.0)
    assert float(lc_r) > float(lc_m) and float(lo_r) > float(lo_m)      # the positives reached the loss
    if with_queue:                                           # forward and backward leave the queue as it was
        for a, b in zip(q.snapshot(), before):
            assert torch.equal(a, b)
    # the class run on the same inputs: the gradient rows of a class-mate's views are other ones
    st_m = st.detach().clone().requires_grad_(True)
    lc2, lo2 = contrastive_losses_stacked(G, st_m, order, mask="class", classes=cls, queue=q, **kw)
    (0.7 * lc2 + 1.3 * lo2).backward()
    gm = st_m.grad.double().view(G + 1, B, C)
    assert bool(((g.view(G + 1, B, C)[:G, 2] - gm[:G, 2]).abs().sum(dim=1) > 0).all())
    with pytest.raises(ValueError, match="mask 'class'"):
        contrastive_losses_stacked(G, st.detach(), order, mask="exclude", class_positives=lam, **kw)


# ---- 6: the training step ---------------------------------------------------------------------------------------------------------------
def test_step_with_class_positives_vs_closed_form_and_graph_replay():
    """ContrastiveStep in mode (normalize, 0.1, class) + class_positives 1 with neg_queue=6 and ids [0, 0, 1] at the ragged
    size, in train() mode.  Step 2's losses equal the fp64 closed form with the three rows and ids step 1 pushed, on the step's
    own stacked embeddings, and differ from the class mask's closed form.  Then four replays of GraphedStep(restore=True),
    another id vector copied into clip_classes before each (one all-equal: no in-batch negative), against eager steps of a twin
    from the same state: losses, parameters, running buffers, queue rows, ids and (head, valid) bit-identical."""
    from facl_amd.train_common import GraphedStep
    from facl_amd.utils_my import circle_contrast, global_contrast, loss_rows
    c, KW = base.RAGGED, base.KW
    B, G = c["B"], c["G"]
    r = np.random.RandomState(7)
    orders = [r.permutation(G) for _ in range(4)]
    ids = _i32([0, 0, 1])
    net, optim, step = base._make_step(c, neg_queue=6, class_positives=1.0)
    assert step.loss_mode == dict(KW, mask="class") and step.class_positives == 1.0 and step.queue is None
    step.clip_classes.copy_(ids)
    for k in range(2):
        assert net.training
        out = [t.detach().clone() for t in step(points(c, 100 + k), order=orders[k])]
        torch.cuda.synchronize()
        if k == 0:
            rows1 = loss_rows(net._stacked.detach(), True, 0.1)[G * B:].clone()
            assert step.queue.head_valid() == (3, 3) and step.queue.ids.tolist() == [0, 0, 1, -1, -1, -1]
            assert torch.equal(step.queue.buf[:3], rows1)
    loss, loss_c, loss_circle = out
    st = net._stacked.detach().double()
    ck = dict(KW, mask="class", key_classes=ids, queue=rows1.double(), queue_classes=ids)
    rc = float(global_contrast(G, st[G * B:], st[:G * B], None, class_positives=1.0, **ck))
    ro = float(circle_contrast(G, st[:G * B], B, order=orders[1], class_positives=1.0, **ck))
    mc = float(global_contrast(G, st[G * B:], st[:G * B], None, **ck))
    mo = float(circle_contrast(G, st[:G * B], B, order=orders[1], **ck))
    print("step 2: loss_c %.6f (fp64 %.6f, class mask %.6f) loss_circle %.6f (fp64 %.6f, class mask %.6f): errors %.3e %.3e"
          % (float(loss_c), rc, mc, float(loss_circle), ro, mo, abs(float(loss_c) - rc) / abs(rc), abs(float(loss_circle) - ro) / abs(ro)))
    assert abs(float(loss_c) - rc) < TOL * abs(rc) and abs(float(loss_circle) - ro) < TOL * abs(ro)
    assert abs(float(loss) - (rc + ro)) < TOL * abs(rc + ro)
    assert abs(rc - mc) > 10 * TOL * abs(mc) and abs(ro - mo) > 10 * TOL * abs(mo)
    assert step.queue.head_valid() == (0, 6) and step.queue.ids.tolist() == [0, 0, 1, 0, 0, 1]
    del net, optim, step

    net_g, opt_g, step_g = base._make_step(c, neg_queue=6, class_positives=1.0)
    g = GraphedStep(step_g, points(c, 99), G, restore=True)
    assert step_g.queue.head_valid() == (0, 0) and int((step_g.queue.buf != 0).sum()) == 0 and step_g.queue.ids.tolist() == [-1] * 6
    net_t, opt_t, step_t = base._make_step(c, neg_queue=6, class_positives=1.0)
    vectors = [[0, 0, 1], [1, -1, 1], [2, 2, 2], [-1, 0, 0]]             # [2, 2, 2]: no in-batch negative
    want_ids = [-1] * 6
    for k, order in enumerate(orders):
        pts = points(c, 100 + k)
        before = snapshot(net_g, opt_g)
        qsnap = step_g.queue.snapshot()
        step_g.clip_classes.copy_(_i32(vectors[k]))
        out_g = [t.detach().clone() for t in g(pts, order=order)]
        net_t.load_state_dict(before["net"])
        opt_t.load_state_dict(before["optim"])
        if step_t.queue is not None:
            step_t.queue.restore(qsnap)
        step_t.clip_classes.copy_(_i32(vectors[k]))
        out_t = [t.detach().clone() for t in step_t(pts, order=order)]
        torch.cuda.synchronize()
        assert net_g.training and net_t.training
        for a, b in zip(out_g, out_t):
            assert torch.isfinite(a).all() and torch.equal(a, b), (k, float(a), float(b))
        sd_g, sd_t = net_g.state_dict(), net_t.state_dict()
        for name in sd_g:
            assert torch.equal(sd_g[name], sd_t[name]), (k, name)
        want_ids[3 * (k % 2):3 * (k % 2) + 3] = vectors[k]
        assert torch.equal(step_g.queue.buf, step_t.queue.buf), k
        assert step_g.queue.ids.tolist() == step_t.queue.ids.tolist() == want_ids, k
        assert step_g.queue.head_valid() == step_t.queue.head_valid() == ((3 * (k + 1)) % 6, min(3 * (k + 1), 6)), k


# ---- 7: the training entry on a tiny dataset ----------------------------------------------------------------------------------------------
def test_train_entry_with_class_positives_and_resume(tmp_path):
    """--loss_mask class --class_positives 1 --label_fraction 0.5 --neg_queue 8 --save_state_every 1 on the 24-clip tree of
    test_gpu_loss_class.py: a 2-epoch run and a 1-epoch run resumed with --resume auto end in the same state_1.pth."""
    from facl_amd import train_state
    root = tmp_path / "d"
    write_tree(str(root))
    state = lambda d, e: train_state.load_state(os.path.join(str(d), "state_%d.pth" % e))
    run = lambda folder, *extra: base._run_entry(root, folder, "--class_positives", 1, *extra)
    sd_a, out_a = run(tmp_path / "a", "--nepoch", 2)
    assert "class mask: 8 of 16 train clips labelled, 4 classes\nclass positives: weight 1\n" in out_a
    losses = re.findall(r"epoch: (\d+) loss mode is : 1 --loss: (\S+)", out_a)
    assert [e for e, _ in losses] == ["0", "1"] and all(np.isfinite(float(v)) for _, v in losses)
    s1 = state(tmp_path / "a", 1)
    assert s1["flags"]["class_positives"] == 1.0 and s1["flags"]["loss_mask"] == "class"
    assert s1["queue"]["state"].tolist() == [0, 8] and (s1["queue"]["ids"] >= 0).any()
    run(tmp_path / "c", "--nepoch", 1)
    assert not os.path.exists(os.path.join(str(tmp_path / "c"), "state_1.pth"))
    sd_c, out_c = run(tmp_path / "c", "--nepoch", 2, "--resume", "auto")
    assert "resumed from %s: epoch 1" % os.path.join(str(tmp_path / "c"), "state_0.pth") in out_c
    assert_same_state(sd_c, sd_a, "model")
    assert_same_state(state(tmp_path / "c", 1), s1, "state_1")
    with pytest.raises(RuntimeError, match="class_positives"):
        base._run_entry(root, tmp_path / "c", "--nepoch", 2, "--resume", "auto", "--class_positives", "0.5")
