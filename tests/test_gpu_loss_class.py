"""GPU tests of the class-aware negative mask of the global / circle losses (--loss_mask class): the three forms of the fused pair
loss (facl_contrast_pair_sum_cls on the register-cached and the streaming kernel, facl_contrast_pair_queue_cls), the ids of the
ring buffer (facl_queue_push_ids), utils_my.contrastive_losses_stacked(mask='class'), the training step (eager and
graph-replayed) and the training entry with --resume.  The fp64 truth is built here from the contract: the full logits with the
masked columns at -inf, an empty negative set contributing exactly 0.  Bounds: those of test_gpu_loss_modes.py and
test_gpu_trajectory.py.  The whole module runs on NaN-poisoned scratch."""
import os
import re

import numpy as np
import pytest
import torch

from helpers import snapshot
from poison import poisoned_scratch  # noqa: F401
from step_factory import make_contrastive_step, points
from synth_tree import assert_same_state, run_train_entry, train_argv, write_tree

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LOSS_TOL, GRAD_TOL = 2e-6, 2e-5      # test_gpu_loss_modes.py
TOL = 1e-4                           # test_gpu_trajectory.py: losses of one step
NINF = float("-inf")


def _state(head, valid):
    return torch.tensor([head, valid], dtype=torch.int32, device=DEV)


def _i32(v):
    return torch.as_tensor(v, dtype=torch.int32).to(DEV)


# ---- the truth on a similarity matrix -----------------------------------------------------------------------------------------
def _masks(G, B, Bk, off, cls, qcls, valid):
    """(masked (B, J), qmasked (B, valid)) of the contract: column j of anchor clip n is masked iff j % Bk == myclip or the
    anchor's class is known and is the column's clip's; queue column k < valid iff the anchor's class is known and is qcls[k]."""
    cls = cls.long()
    col_clip = torch.arange(G * Bk, device=DEV) % Bk
    my = torch.arange(B, device=DEV) + off
    mine = cls[my]
    masked = (col_clip[None, :] == my[:, None]) | ((mine[:, None] >= 0) & (cls[col_clip][None, :] == mine[:, None]))
    if qcls is None or valid == 0:
        return masked, torch.zeros(B, 0, dtype=torch.bool, device=DEV)
    return masked, (mine[:, None] >= 0) & (qcls.long()[None, :valid] == mine[:, None])


def _lse_or_empty(neg):
    empty = (neg == NINF).all(dim=1)
    lse = torch.logsumexp(torch.where(empty[:, None], torch.zeros((), dtype=neg.dtype, device=neg.device), neg), dim=1)
    return lse, empty


def _terms(pos, lse, empty):
    """sum over slots, mean over clips of logaddexp(pos, lse) - pos; a clip without a negative contributes exactly 0."""
    zero = torch.zeros((), dtype=pos.dtype, device=pos.device)
    t = torch.logaddexp(pos, lse[None, :]) - pos
    return torch.where(empty[None, :], zero, t).mean(dim=1).sum()


def _closed_form(sim, sim_q, valid, G, B, Bk, order, off, cls, qcls):
    """(loss_c, loss_circle) of the contract on a ((G+1) B, G Bk) similarity matrix and the first `valid` columns of a
    ((G+1) B, L) queue similarity matrix (None: no queue), in sim's dtype."""
    J = G * Bk
    masked, qmasked = _masks(G, B, Bk, off, cls, qcls, valid)
    fill = torch.full((), NINF, dtype=sim.dtype, device=sim.device)
    blocks = sim.view(G + 1, B, J)
    q = None if sim_q is None else sim_q.view(G + 1, B, -1)[:, :, :valid]
    block = lambda g: torch.where(masked, fill, blocks[g]) if q is None else \
        torch.cat((torch.where(masked, fill, blocks[g]), torch.where(qmasked, fill, q[g])), dim=1)
    n = torch.arange(B, device=sim.device)
    lse_g, empty_g = _lse_or_empty(block(G))
    pos_g = torch.stack([blocks[G][n, g * Bk + n + off] for g in range(G)])
    order = [int(o) for o in order]
    lse_o, empty_o = _lse_or_empty(torch.cat([block(order[i]) for i in range(G - 1)], dim=1))
    pos_o = torch.stack([blocks[order[i]][n, order[i + 1] * Bk + n + off] for i in range(G - 1)])
    return _terms(pos_g, lse_g, empty_g), _terms(pos_o, lse_o, empty_o)


def _positive_cells(G, B, Bk, order, off):
    """bool ((G+1) B, J): the cells the positives are read from."""
    pos = torch.zeros((G + 1) * B, G * Bk, dtype=torch.bool, device=DEV)
    order = [int(o) for o in order]
    for n in range(B):
        for g in range(G):
            pos[G * B + n, g * Bk + n + off] = True
        for i in range(G - 1):
            pos[order[i] * B + n, order[i + 1] * Bk + n + off] = True
    return pos


def _ids(Bk):
    """ids from 3 classes with some -1: 2, 1, 0, -1, 2, 1, ..."""
    return _i32([(3 + 7 * k) % 4 - 1 for k in range(Bk)])


def _every_anchor_keeps_a_negative(cls, B, Bk, off):
    c = cls.tolist()
    return all(any(k != n + off and not (c[n + off] >= 0 and c[k] == c[n + off]) for k in range(Bk)) for n in range(B))


def _sim(G, B, Bk, filling, L=0, valid=0):
    torch.manual_seed(G * 1000 + Bk + L)
    R, J = (G + 1) * B, G * Bk
    draw = (lambda *s: torch.randn(*s, device=DEV) * 2.0) if filling == "normal" else \
        (lambda *s: torch.rand(*s, device=DEV) * 6.0 - 203.0)
    sim = draw(R, J)
    order = torch.as_tensor(np.random.RandomState(G).permutation(G), device=DEV)
    if not L:
        return sim, order
    sim_q = draw(R, L)
    sim_q[:, valid:] = float("nan")                          # columns >= valid are never used
    return sim, sim_q, order


def _run_pair(sim, G, B, Bk, order, off, cls=None, mask="exclude"):
    """facl_contrast_pair_sum_cls (cls given) or facl_contrast_pair_sum_mask: (dsim, losses, losses32)."""
    from facl_amd import _lib
    from facl_amd.sa_mlp import _Workspace
    from facl_amd.utils_my import MASK_MODES
    lib = _lib.load_library()
    ws = _Workspace.get(torch.device(DEV))
    dsim = _lib.empty_like(sim)
    l64, l32 = _lib.empty(2, dtype=torch.float64, device=DEV), _lib.empty(3, device=DEV)
    if cls is not None:
        _lib.check(lib.facl_contrast_pair_sum_cls(_lib.ptr(sim), G, B, Bk, G * Bk, _lib.ptr(order), off, _lib.ptr(cls), _lib.ptr(dsim),
                                                  _lib.ptr(l64), _lib.ptr(l32), _lib.ptr(ws), _lib.stream()), "pair_sum_cls")
    else:
        _lib.check(lib.facl_contrast_pair_sum_mask(_lib.ptr(sim), G, B, Bk, G * Bk, _lib.ptr(order), off, MASK_MODES[mask],
                                                   _lib.ptr(dsim), _lib.ptr(l64), _lib.ptr(l32), _lib.ptr(ws), _lib.stream()), "pair_sum_mask")
    torch.cuda.synchronize()
    return dsim, l64, l32


def _run_queue(sim, sim_q, G, B, Bk, L, order, off, state, cls=None, qcls=None, mask="exclude"):
    """facl_contrast_pair_queue_cls (cls given) or facl_contrast_pair_queue: (dsim, dsim_q, losses, losses32)."""
    from facl_amd import _lib
    from facl_amd.sa_mlp import _Workspace
    from facl_amd.utils_my import MASK_MODES
    lib = _lib.load_library()
    ws = _Workspace.get(torch.device(DEV))
    dsim, dsim_q = _lib.empty_like(sim), _lib.empty_like(sim_q)
    l64, l32 = _lib.empty(2, dtype=torch.float64, device=DEV), _lib.empty(3, device=DEV)
    if cls is not None:
        _lib.check(lib.facl_contrast_pair_queue_cls(_lib.ptr(sim), _lib.ptr(sim_q), G, B, Bk, G * Bk, L, _lib.ptr(order), off,
                                                    _lib.ptr(cls), _lib.ptr(qcls), _lib.ptr(state), _lib.ptr(dsim), _lib.ptr(dsim_q),
                                                    _lib.ptr(l64), _lib.ptr(l32), _lib.ptr(ws), _lib.stream()), "pair_queue_cls")
    else:
        _lib.check(lib.facl_contrast_pair_queue(_lib.ptr(sim), _lib.ptr(sim_q), G, B, Bk, G * Bk, L, _lib.ptr(order), off,
                                                MASK_MODES[mask], _lib.ptr(state), _lib.ptr(dsim), _lib.ptr(dsim_q), _lib.ptr(l64),
                                                _lib.ptr(l32), _lib.ptr(ws), _lib.stream()), "pair_queue")
    torch.cuda.synchronize()
    return dsim, dsim_q, l64, l32


def _rel(a, b):
    return abs(float(a) - float(b)) / abs(float(b))


# register kernel with a ragged tail, a sharded offset, the streaming kernel ((G - 1) J > 24 * 1024)
PAIR_SHAPES = [(6, 5, 5, 0), (4, 3, 6, 3), (24, 2, 48, 3)]


# ---- 1: the pair loss under the class mask on synthetic similarities -----------------------------------------------------------
@pytest.mark.parametrize("filling", ["normal", "minus200"])
@pytest.mark.parametrize("G,B,Bk,off", PAIR_SHAPES)
def test_pair_cls_entry_on_synthetic_sim(G, B, Bk, off, filling):
    J = G * Bk
    if G == 24:
        assert (G - 1) * J > 24 * 1024
    sim, order = _sim(G, B, Bk, filling)
    cls = _ids(Bk)
    assert _every_anchor_keeps_a_negative(cls, B, Bk, off)    # a relative error on a zero loss means nothing
    assert (cls < 0).any() and len(set(cls.tolist()) - {-1}) == 3
    dsim, l64, l32 = _run_pair(sim, G, B, Bk, order, off, cls)
    s64 = sim.double().requires_grad_(True)
    rc, ro = _closed_form(s64, None, 0, G, B, Bk, order.tolist(), off, cls, None)
    (gr,) = torch.autograd.grad(rc + ro, s64)
    e_c, e_o, e_g = _rel(l64[0], rc.detach()), _rel(l64[1], ro.detach()), float((dsim.double() - gr).norm() / gr.norm())
    print("pair cls G=%d B=%d Bk=%d %s: loss_c %.3e loss_circle %.3e dsim %.3e" % (G, B, Bk, filling, e_c, e_o, e_g))
    assert torch.isfinite(l64).all() and torch.isfinite(dsim).all()
    assert e_c <= LOSS_TOL and e_o <= LOSS_TOL
    assert e_g <= GRAD_TOL
    masked = _masks(G, B, Bk, off, cls, None, 0)[0].repeat(G + 1, 1)
    assert int(masked.sum()) > (G + 1) * B * G                # the ids masked more than the clips' own columns
    assert int((dsim[masked & ~_positive_cells(G, B, Bk, order, off)] != 0).sum()) == 0
    c, o = l64[0].float(), l64[1].float()
    assert torch.equal(l32, torch.stack((c, o, o + c)))
    # the mask reached the values: exclude on the same similarities gives another loss
    assert not torch.equal(_run_pair(sim, G, B, Bk, order, off)[1], l64)


# ---- 2: the identities with exclude, bit for bit ---------------------------------------------------------------------------------
@pytest.mark.parametrize("ids", ["unknown", "distinct"])
@pytest.mark.parametrize("G,B,Bk,off", PAIR_SHAPES)
def test_pair_cls_identities_with_exclude(G, B, Bk, off, ids):
    sim, order = _sim(G, B, Bk, "normal")
    cls = _i32([-1 - k % 3 for k in range(Bk)]) if ids == "unknown" else _i32(np.random.RandomState(Bk).permutation(Bk) + 5)
    got = _run_pair(sim, G, B, Bk, order, off, cls)
    want = _run_pair(sim, G, B, Bk, order, off)
    for a, b in zip(got, want):
        assert torch.isfinite(a).all() and torch.equal(a, b)


# ---- 3: no negative at all -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filling", ["normal", "minus200"])
@pytest.mark.parametrize("G,B,Bk,off", PAIR_SHAPES)
def test_pair_cls_one_class_is_exactly_zero(G, B, Bk, off, filling):
    sim, order = _sim(G, B, Bk, filling)
    dsim, l64, l32 = _run_pair(sim, G, B, Bk, order, off, _i32([4] * Bk))
    assert torch.isfinite(dsim).all() and torch.isfinite(l64).all() and torch.isfinite(l32).all()
    assert not l64.any() and not l32.any() and not dsim.any()


# ---- 4: the queue form -----------------------------------------------------------------------------------------------------------
# (G, B, Bk, off, L, valid): the scalar path; the 16-byte path with L across the 2048-column chunk; J = 2304 across the chunk
QUEUE_CASES = [(4, 3, 3, 0, 6, 0), (4, 3, 3, 0, 6, 3), (4, 3, 3, 0, 6, 6), (4, 4, 4, 0, 2052, 2050), (4, 4, 4, 0, 2052, 2052),
               (24, 2, 96, 3, 8, 8), (24, 2, 96, 3, 8, 5)]


def _queue_ids(cls, B, off, L, valid):
    """ids of the queue rows from 3 classes with some -1; from `valid` on the class of an anchor of known class."""
    known = [c for c in cls.tolist()[off:off + B] if c >= 0]
    q = [(5 * k + 1) % 4 - 1 for k in range(L)]
    return _i32(q[:valid] + [known[0]] * (L - valid))


@pytest.mark.parametrize("filling", ["normal", "minus200"])
@pytest.mark.parametrize("G,B,Bk,off,L,valid", QUEUE_CASES)
def test_pair_queue_cls_entry_on_synthetic_sim(G, B, Bk, off, L, valid, filling):
    import neg_queue_paths
    J = G * Bk
    sim, sim_q, order = _sim(G, B, Bk, filling, L, valid)
    cls = _ids(Bk)
    qcls = _queue_ids(cls, B, off, L, valid)
    assert _every_anchor_keeps_a_negative(cls, B, Bk, off)
    dsim, dsim_q, l64, l32 = _run_queue(sim, sim_q, G, B, Bk, L, order, off, _state(0, valid), cls, qcls)
    assert neg_queue_paths.vectorised(J, L, sim, sim_q, dsim, dsim_q, qcls) == (L == 2052 or L == 8)
    assert neg_queue_paths.chunks(J, L) == ((2, 1) if J == 2304 else (1, 2) if L == 2052 else (1, 1))
    s64, q64 = sim.double().requires_grad_(True), sim_q.double().requires_grad_(True)
    rc, ro = _closed_form(s64, q64, valid, G, B, Bk, order.tolist(), off, cls, qcls)
    gr, gq = torch.autograd.grad(rc + ro, (s64, q64))
    got, want = torch.cat((dsim, dsim_q), dim=1).double(), torch.cat((gr, gq), dim=1)
    e_c, e_o, e_g = _rel(l64[0], rc.detach()), _rel(l64[1], ro.detach()), float((got - want).norm() / want.norm())
    print("pair+queue cls G=%d B=%d Bk=%d L=%d valid=%d %s: loss_c %.3e loss_circle %.3e [dsim|dsim_q] %.3e"
          % (G, B, Bk, L, valid, filling, e_c, e_o, e_g))
    assert torch.isfinite(l64).all() and torch.isfinite(dsim).all() and torch.isfinite(dsim_q).all()
    assert e_c <= LOSS_TOL and e_o <= LOSS_TOL
    assert e_g <= GRAD_TOL
    masked, qmasked = _masks(G, B, Bk, off, cls, qcls, valid)
    assert int((dsim[masked.repeat(G + 1, 1) & ~_positive_cells(G, B, Bk, order, off)] != 0).sum()) == 0
    assert int((dsim_q[:, :valid][qmasked.repeat(G + 1, 1)] != 0).sum()) == 0
    assert int((dsim_q[:, valid:] != 0).sum()) == 0
    if valid:
        assert bool(qmasked.any()) and not bool(qmasked.all())
    c, o = l64[0].float(), l64[1].float()
    assert torch.equal(l32, torch.stack((c, o, o + c)))


@pytest.mark.parametrize("G,B,Bk,off,L,valid", [c for c in QUEUE_CASES if c[5] > 0])
def test_pair_queue_cls_with_unknown_ids_is_the_exclude_queue(G, B, Bk, off, L, valid):
    """Every id of cls < 0: the outputs equal facl_contrast_pair_queue(..., exclude) bit for bit, whatever qcls holds."""
    sim, sim_q, order = _sim(G, B, Bk, "normal", L, valid)
    cls = _i32([-1 - k % 3 for k in range(Bk)])
    qcls = _i32([k % 4 - 2 for k in range(L)])
    got = _run_queue(sim, sim_q, G, B, Bk, L, order, off, _state(0, valid), cls, qcls)
    want = _run_queue(sim, sim_q, G, B, Bk, L, order, off, _state(0, valid))
    for a, b in zip(got, want):
        assert torch.isfinite(a).all() and torch.equal(a, b)


# the third column: what facl_contrast_pair_sum_cls launches for the shape
@pytest.mark.parametrize("G,B,Bk,off,L,pair_kernel", [(4, 3, 3, 0, 6, "register"), (4, 4, 4, 0, 2052, "register"),
                                                      (24, 2, 96, 3, 8, "streaming")])
def test_pair_queue_cls_with_an_empty_queue_is_the_pair_entry(G, B, Bk, off, L, pair_kernel):
    """valid = 0: dsim_q is all zero, masked cells are exactly 0 in both entries, and the outputs are those of
    facl_contrast_pair_sum_cls.  How equal follows from what the two entries accumulate in, not from their outputs:

    * where the pair entry runs the register-cached kernel -- (4, 3, 3, 0, 6), the empty-queue case of the scalar shape, and
      (4, 4, 4, 0, 2052) -- both sides sum exp() and the slots' d/dlse in fp64 and round once: bit for bit, losses, losses32
      and all of dsim;
    * at (24, 2, 96, 3, 8) the pair entry runs the streaming kernel, which sums the slots' d/dlse serially in fp32 (as its
      `exclude` instantiation does, whose bits the identity test above holds it to), while the queue kernels sum it in fp64 (as
      THEIR `exclude` instantiations do, whose bits the unknown-ids test above holds them to).  Bit equality there would be an
      equality between the two existing `exclude` kernels, which test_gpu_neg_queue.py holds to the tolerances for the same
      reason.  So: the losses (fp64 on both sides) within LOSS_TOL, dsim within GRAD_TOL of its norm.  Measured: losses
      bit-identical, dsim 9.1e-9 of its norm, 84315 of 115200 elements differ in their last bits."""
    assert ((G - 1) * G * Bk <= 24 * 1024) == (pair_kernel == "register")
    sim, sim_q, order = _sim(G, B, Bk, "normal", L, 0)
    cls = _ids(Bk)
    qcls = _queue_ids(cls, B, off, L, 0)
    dsim, dsim_q, l64, l32 = _run_queue(sim, sim_q, G, B, Bk, L, order, off, _state(0, 0), cls, qcls)
    d0, m64, m32 = _run_pair(sim, G, B, Bk, order, off, cls)
    e_l = float(((m64 - l64).abs() / m64.abs()).max())
    e_d = float((d0.double() - dsim.double()).norm() / d0.double().norm())
    print("empty queue vs facl_contrast_pair_sum_cls G=%d Bk=%d L=%d (%s): losses %.3e dsim %.3e, %d of %d dsim elements differ"
          % (G, Bk, L, pair_kernel, e_l, e_d, int((d0 != dsim).sum()), dsim.numel()))
    assert torch.isfinite(dsim).all() and torch.isfinite(l64).all()
    assert int((dsim_q != 0).sum()) == 0
    quiet = _masks(G, B, Bk, off, cls, None, 0)[0].repeat(G + 1, 1) & ~_positive_cells(G, B, Bk, order, off)
    assert int((dsim[quiet] != 0).sum()) == 0 and int((d0[quiet] != 0).sum()) == 0
    assert torch.equal(dsim == 0, d0 == 0)
    if pair_kernel == "register":
        assert torch.equal(l64, m64) and torch.equal(l32, m32)
        assert torch.equal(dsim, d0)
    else:
        assert e_l <= LOSS_TOL and e_d <= GRAD_TOL
        c, o = l64[0].float(), l64[1].float()
        assert torch.equal(l32, torch.stack((c, o, o + c)))


@pytest.mark.parametrize("G,B,Bk,off,L,valid", [(4, 3, 3, 0, 6, 3), (4, 4, 4, 0, 2052, 2050), (24, 2, 96, 3, 8, 8)])
def test_pair_queue_cls_every_live_column_masked_is_exactly_zero(G, B, Bk, off, L, valid):
    """One class in cls and in qcls: no negative anywhere, zeros and finite values."""
    sim, sim_q, order = _sim(G, B, Bk, "normal", L, valid)
    dsim, dsim_q, l64, l32 = _run_queue(sim, sim_q, G, B, Bk, L, order, off, _state(0, valid), _i32([1] * Bk), _i32([1] * L))
    for t in (dsim, dsim_q, l64, l32):
        assert torch.isfinite(t).all() and not t.any()


# ---- 5: the ids of the ring buffer -------------------------------------------------------------------------------------------------
def test_push_ids_beside_the_rows():
    from facl_amd.neg_queue import NegativeQueue
    P, L, C = 4, 8, 8
    GUARD = 0x5A5A5A5A
    q = NegativeQueue(L, C, P, DEV, with_ids=True)
    assert q.ids.tolist() == [-1] * L
    held = torch.full((L + 8,), GUARD, dtype=torch.int32, device=DEV)     # guard words around the ids
    q.ids = held[4:4 + L]
    q.ids.fill_(-1)
    rows_model, ids_model = torch.zeros(L, C), [-1] * L
    head = valid = 0
    for k in range(3):                                       # the third push wraps and overwrites the oldest
        rows = torch.randn(P, C, device=DEV)
        ids = _i32([10 * k + i if i != 1 else -1 for i in range(P)])
        q.push(rows, ids=ids)
        rows_model[head:head + P] = rows.cpu()
        ids_model[head:head + P] = ids.tolist()
        head, valid = (head + P) % L, min(valid + P, L)
        assert q.head_valid() == (head, valid), k            # as without ids
        assert torch.equal(q.buf.cpu(), rows_model) and q.ids.tolist() == ids_model, k
        assert q.valid_ids().tolist() == ids_model[:valid]
        assert held[:4].tolist() == [GUARD] * 4 and held[4 + L:].tolist() == [GUARD] * 4, k
    assert ids_model == [20, -1, 22, 23, 10, -1, 12, 13]
    snap = q.snapshot()
    q.push(torch.randn(P, C, device=DEV), ids=_i32([7] * P))
    q.restore(snap)
    assert q.ids.tolist() == ids_model and q.head_valid() == (head, valid) and torch.equal(q.buf.cpu(), rows_model)
    with pytest.raises(ValueError):
        q.push(torch.randn(P, C, device=DEV))                # a queue with ids takes them with every push
    with pytest.raises(ValueError):
        NegativeQueue(L, C, P, DEV).push(torch.randn(P, C, device=DEV), ids=_i32([7] * P))
    q.restore()
    assert q.ids.tolist() == [-1] * L and q.head_valid() == (0, 0)


# ---- 6: contrastive_losses_stacked(mask='class') -----------------------------------------------------------------------------------
@pytest.mark.parametrize("with_queue", [False, True])
@pytest.mark.parametrize("normalize,tau", [(True, 0.07), (False, 4.0)])
@pytest.mark.parametrize("G,B,C,L", [(6, 5, 32, 15), (10, 4, 512, 16)])
def test_stacked_losses_with_class_mask_vs_closed_form_fp64(G, B, C, L, normalize, tau, with_queue):
    """Row pass + similarity GEMMs + class-masked pair loss + their backward against the fp64 closed form: both values and the
    gradient wrt the stacked embeddings.  (6, 5, 32): library GEMMs and the scalar kernels; (10, 4, 512): MFMA GEMMs and the
    16-byte kernels."""
    from facl_amd.neg_queue import NegativeQueue
    from facl_amd.utils_my import circle_contrast, contrastive_losses_stacked, global_contrast
    torch.manual_seed(G * B + C)
    x0 = (torch.randn(G * B, C, dtype=torch.float64) * 0.3).to(DEV)
    xg0 = (torch.randn(B, C, dtype=torch.float64) * 0.3).to(DEV)
    order = np.random.RandomState(1).permutation(G)
    cls = _i32([0, 1, 0, -1, 2][:B])
    assert _every_anchor_keeps_a_negative(cls, B, B, 0)
    q = rows64 = qids = None
    if with_queue:
        q = NegativeQueue(L, C, B, DEV, with_ids=True)
        for k in range(2):
            q.push(torch.randn(B, C, device=DEV) * (1.0 if normalize else 0.3), ids=_i32([(k + 2 * i) % 4 - 1 for i in range(B)]))
        rows64, qids = q.valid_rows().double(), q.valid_ids()
        assert rows64.shape[0] == 2 * B < L
        before = q.snapshot()
    kw = dict(normalize=normalize, temperature=tau)

    def truth(xg, x, mask="class"):
        ck = dict(key_classes=cls, queue_classes=qids) if mask == "class" else {}
        qr = None if rows64 is None else rows64.to(x.dtype)
        return (global_contrast(G, xg, x, None, queue=qr, mask=mask, **kw, **ck),
                circle_contrast(G, x, B, order=order, queue=qr, mask=mask, **kw, **ck))

    xg64, x64 = xg0.clone().requires_grad_(True), x0.clone().requires_grad_(True)
    lc_r, lo_r = truth(xg64, x64)
    gr = torch.autograd.grad(0.7 * lc_r + 1.3 * lo_r, (xg64, x64))
    lc_r, lo_r = lc_r.detach(), lo_r.detach()
    st = torch.cat((x0, xg0), 0).float().requires_grad_(True)
    lc, lo = contrastive_losses_stacked(G, st, order, mask="class", classes=cls, queue=q, **kw)
    (0.7 * lc + 1.3 * lo).backward()                        # distinct upstream gradients exercise facl_scale_rows2
    g = st.grad.double()
    e = (_rel(lc.detach(), lc_r), _rel(lo.detach(), lo_r),
         float((g[:G * B] - gr[1]).norm() / gr[1].norm()), float((g[G * B:] - gr[0]).norm() / gr[0].norm()))
    print("stacked cls G=%d B=%d C=%d queue=%d %s: loss_c %.3e loss_circle %.3e dx %.3e dxg %.3e" % (G, B, C, with_queue, (normalize, tau), *e))
    assert torch.isfinite(g).all()
    assert e[0] <= LOSS_TOL and e[1] <= LOSS_TOL
    assert e[2] < GRAD_TOL and e[3] < GRAD_TOL
    lc_x, lo_x = truth(xg0, x0, "exclude")
    assert float(lc_r) < float(lc_x) and float(lo_r) < float(lo_x)      # the ids reached the loss
    if with_queue:                                           # forward and backward leave the queue as it was; the ids are staged
        for a, b in zip(q.snapshot(), before):
            assert torch.equal(a, b)
        assert torch.equal(q._staged_ids, cls)
    with pytest.raises(ValueError, match="with_ids"):
        contrastive_losses_stacked(G, st.detach(), order, mask="class", classes=cls, queue=NegativeQueue(L, C, B, DEV), **kw)
    with pytest.raises(ValueError, match="one id per key clip"):
        contrastive_losses_stacked(G, st.detach(), order, mask="class", classes=cls[:B - 1].contiguous(), **kw)


# ---- 7: the training step -----------------------------------------------------------------------------------------------------------
RAGGED = dict(B=3, G=5, N=1000, D=3)                       # config `ragged` of test_gpu_trajectory.py
KW = dict(normalize=True, temperature=0.1)


def _make_step(c, mask="class", **flags):
    return make_contrastive_step(c, loss_normalize=1, loss_temperature=0.1, loss_mask=mask, **flags)


def test_step_with_class_mask_vs_closed_form_and_graph_replay():
    """ContrastiveStep in mode (normalize, 0.1, class) with neg_queue=6 and ids [0, 0, 1] at the ragged size, in train() mode.
    Step 2's losses equal the fp64 closed form with the three rows and ids step 1 pushed, on the step's own stacked embeddings,
    and differ from `exclude`'s -- the closed form's on the same embeddings and an exclude run's.  Then four replays of
    GraphedStep(restore=True), another id vector copied into clip_classes before each, against eager steps of a twin from the
    same state: losses, parameters, running buffers, queue rows, ids and (head, valid) bit-identical."""
    from facl_amd.train_common import GraphedStep
    from facl_amd.utils_my import circle_contrast, global_contrast, loss_rows
    c = RAGGED
    B, G = c["B"], c["G"]
    r = np.random.RandomState(7)
    orders = [r.permutation(G) for _ in range(4)]
    ids = _i32([0, 0, 1])
    net, optim, step = _make_step(c, neg_queue=6)
    assert step.loss_mode == dict(KW, mask="class") and step.queue is None and step.clip_classes.tolist() == [-1] * B
    net_x, optim_x, step_x = _make_step(c, mask="exclude", neg_queue=6)
    step.clip_classes.copy_(ids)
    outs = []
    for k in range(2):
        assert net.training
        out = [t.detach().clone() for t in step(points(c, 100 + k), order=orders[k])]
        outs.append([t.detach().clone() for t in step_x(points(c, 100 + k), order=orders[k])])
        torch.cuda.synchronize()
        if k == 0:
            rows1 = loss_rows(net._stacked.detach(), True, 0.1)[G * B:].clone()
            assert step.queue.head_valid() == (3, 3) and step.queue.ids.tolist() == [0, 0, 1, -1, -1, -1]
            assert torch.equal(step.queue.buf[:3], rows1)
    loss, loss_c, loss_circle = out
    st = net._stacked.detach().double()
    ck = dict(KW, mask="class", key_classes=ids, queue=rows1.double(), queue_classes=ids)
    rc = float(global_contrast(G, st[G * B:], st[:G * B], None, **ck))
    ro = float(circle_contrast(G, st[:G * B], B, order=orders[1], **ck))
    xk = dict(KW, mask="exclude", queue=rows1.double())
    xc = float(global_contrast(G, st[G * B:], st[:G * B], None, **xk))
    xo = float(circle_contrast(G, st[:G * B], B, order=orders[1], **xk))
    print("step 2: loss_c %.6f (fp64 %.6f, exclude %.6f) loss_circle %.6f (fp64 %.6f, exclude %.6f); the exclude run's: %.6f %.6f"
          % (float(loss_c), rc, xc, float(loss_circle), ro, xo, float(outs[1][1]), float(outs[1][2])))
    assert abs(float(loss_c) - rc) < TOL * abs(rc) and abs(float(loss_circle) - ro) < TOL * abs(ro)
    assert abs(float(loss) - (rc + ro)) < TOL * abs(rc + ro)
    assert abs(rc - xc) > 10 * TOL * abs(xc) and abs(ro - xo) > 10 * TOL * abs(xo)
    assert abs(float(loss_c) - float(outs[1][1])) > 10 * TOL * abs(xc) and abs(float(loss_circle) - float(outs[1][2])) > 10 * TOL * abs(xo)
    assert step.queue.head_valid() == (0, 6) and step.queue.ids.tolist() == [0, 0, 1, 0, 0, 1]
    del net, optim, step, net_x, optim_x, step_x

    net_g, opt_g, step_g = _make_step(c, neg_queue=6)
    g = GraphedStep(step_g, points(c, 99), G, restore=True)
    assert step_g.queue.head_valid() == (0, 0) and int((step_g.queue.buf != 0).sum()) == 0 and step_g.queue.ids.tolist() == [-1] * 6
    net_t, opt_t, step_t = _make_step(c, neg_queue=6)
    vectors = [[0, 0, 1], [1, -1, 1], [2, 2, 2], [-1, 0, 0]]             # [2, 2, 2]: every negative of that step is a queue row
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


# ---- 8: the training entry on a tiny dataset ------------------------------------------------------------------------------------------
def _run_entry(root, folder, *extra):
    mode = ("--loss_normalize", "1", "--loss_temperature", "0.1", "--loss_mask", "class", "--label_fraction", "0.5",
            "--neg_queue", "8", "--save_state_every", "1")
    return run_train_entry(train_argv(root, folder, *extra, before_save=mode, features_first=True))


def test_train_entry_with_class_mask_and_resume(tmp_path):
    from facl_amd import train_state
    root = tmp_path / "d"
    write_tree(str(root))
    state = lambda d, e: train_state.load_state(os.path.join(str(d), "state_%d.pth" % e))
    sd_a, out_a = _run_entry(root, tmp_path / "a", "--nepoch", 2)
    assert "class mask: 8 of 16 train clips labelled, 4 classes" in out_a
    assert len(re.findall(r"class mask:", out_a)) == 1
    losses = re.findall(r"epoch: (\d+) loss mode is : 1 --loss: (\S+)", out_a)
    assert [e for e, _ in losses] == ["0", "1"] and all(np.isfinite(float(v)) for _, v in losses)
    s1 = state(tmp_path / "a", 1)
    q = s1["queue"]
    assert set(q) == {"buf", "state", "ids"} and q["ids"].dtype == torch.int32 and q["ids"].shape == (8,)
    assert q["state"].tolist() == [0, 8] and (q["ids"] >= 0).any() and ((q["ids"] >= -1) & (q["ids"] < 4)).all()
    assert (s1["flags"]["loss_mask"], s1["flags"]["label_fraction"], s1["flags"]["label_seed"]) == ("class", 0.5, 0)
    # two identical runs give identical checkpoints
    sd_b, out_b = _run_entry(root, tmp_path / "b", "--nepoch", 2)
    assert_same_state(sd_a, sd_b, "model")
    assert_same_state(state(tmp_path / "b", 1), s1, "state_1")
    names =[n for n in os.listdir(str(tmp_path / "a")) if n.endswith("_0.pth") and not n.startswith("state_")]
    assert len(names) == 1
    assert_same_state(torch.load(os.path.join(str(tmp_path / "a"), names[0]), map_location="cpu", weights_only=True),
          torch.load(os.path.join(str(tmp_path / "b"), names[0]), map_location="cpu", weights_only=True), names[0])
    # stopped after epoch 0 and continued: the same state_1
    _run_entry(root, tmp_path / "c", "--nepoch", 1)
    assert not os.path.exists(os.path.join(str(tmp_path / "c"), "state_1.pth"))
    sd_c, out_c = _run_entry(root, tmp_path / "c", "--nepoch", 2, "--resume", "auto")
    assert "resumed from %s: epoch 1" % os.path.join(str(tmp_path / "c"), "state_0.pth") in out_c
    assert_same_state(sd_c, sd_a, "model")
    assert_same_state(state(tmp_path / "c", 1), s1, "state_1")
    # a resumed run repeats the labelled fraction
    with pytest.raises(RuntimeError, match="label_fraction"):
        _run_entry(root, tmp_path / "c", "--nepoch", 2, "--resume", "auto", "--label_fraction", "1.0")
