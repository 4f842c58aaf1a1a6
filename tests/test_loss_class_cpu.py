"""Class-aware negative mask of the contrastive losses (--loss_mask class), host side: the fp64 closed forms of facl_amd.utils_my
with ``mask='class'`` against explicitly materialised logits whose masked columns are -inf, the two identities with
``mask='exclude'``, the empty negative set, the C ABI symbols, the flags, the id vector of --label_fraction, the queue's ids and
the saved state."""
import argparse
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("facl_contrast_pair_sum_cls", "facl_contrast_pair_queue_cls", "facl_queue_push_ids")
NINF = float("-inf")


def _inputs(G, B, C, Q, seed=11):
    torch.manual_seed(seed + G * 10 + B)
    x = torch.randn(G * B, C, dtype=torch.float64) * 1.5
    xg = torch.randn(B, C, dtype=torch.float64) * 1.5
    queue = torch.randn(Q, C, dtype=torch.float64) * 1.5
    return x, xg, queue, np.random.RandomState(3).permutation(G)


def _explicit(xg, x, queue, order, G, B, ids, qids):
    """(loss_c, loss_circle) the long way, one clip and one slot at a time: the FULL row of logits [keys | queue] of every
    anchor of the clip, the masked columns set to -inf (the contract of the issue: the clip's own columns, and the columns /
    queue rows whose id is the anchor's known one), log-sum-exp over the clip's rows together; a clip whose rows are all -inf
    contributes 0."""
    xv = x.view(G, B, -1)
    J = G * B
    col_clip = torch.arange(J) % B
    loss = [torch.zeros((), dtype=x.dtype), torch.zeros((), dtype=x.dtype)]
    for n in range(B):
        mine = int(ids[n])
        masked = col_clip == n
        qmasked = torch.zeros(queue.shape[0], dtype=torch.bool)
        if mine >= 0:
            masked = masked | (ids[col_clip] == mine)
            qmasked = qids == mine
        for which, anchors, slots in (
                (0, xg[n:n + 1], [(xg[n], xv[g, n]) for g in range(G)]),
                (1, torch.stack([xv[order[i], n] for i in range(G - 1)]),
                 [(xv[order[i], n], xv[order[i + 1], n]) for i in range(G - 1)])):
            logits = torch.cat((anchors @ x.t(), anchors @ queue.t()), dim=1)
            logits[:, torch.cat((masked, qmasked))] = NINF
            members = logits[logits > NINF]
            for a, k in slots:
                pos = (a * k).sum()
                if members.numel():
                    loss[which] = loss[which] + (torch.logsumexp(torch.cat((pos.reshape(1), members)), 0) - pos) / B
    return loss


IDS = {3: [[0, 1, 0], [2, -1, 2], [-1, -1, 0]], 4: [[0, 1, 0, 2], [1, 1, -1, 1], [-1, 0, -1, 0]]}


@pytest.mark.parametrize("with_queue", [False, True])
@pytest.mark.parametrize("G,B,C", [(4, 3, 8), (3, 4, 8)])
def test_closed_forms_vs_explicit_logits_fp64(G, B, C, with_queue):
    from facl_amd.utils_my import circle_contrast, global_contrast
    x, xg, queue, order = _inputs(G, B, C, 5 if with_queue else 0)
    for k, ids in enumerate(IDS[B]):
        ids = torch.tensor(ids, dtype=torch.int32)
        qids = torch.tensor([0, -1, 1, 2, 0][:queue.shape[0]], dtype=torch.int32)
        for normalize, tau in ((False, 1.0), (True, 0.07)):
            kw = dict(normalize=normalize, temperature=tau, mask="class", key_classes=ids,
                      queue=queue if with_queue else None, queue_classes=qids if with_queue else None)
            lc = global_contrast(G, xg, x, None, **kw)
            lo = circle_contrast(G, x, B, order=order, **kw)
            s = float(np.float32(1.0 / np.sqrt(tau)))
            rows = (lambda t: t / t.norm(dim=1, keepdim=True).clamp_min(1e-12) * s) if normalize else (lambda t: t * s)
            rc, ro = _explicit(rows(xg), rows(x), queue, order, G, B, ids.long(), qids.long())
            assert abs(float(lc) - float(rc)) <= 1e-12 * abs(float(rc)), (k, normalize)
            assert abs(float(lo) - float(ro)) <= 1e-12 * abs(float(ro)), (k, normalize)
            # the mask removes members: never above exclude's value (equal where no id matched or the value is saturated)
            ex = dict(kw, mask="exclude", key_classes=None, queue_classes=None)
            assert float(lc) <= float(global_contrast(G, xg, x, None, **ex))


@pytest.mark.parametrize("with_queue", [False, True])
@pytest.mark.parametrize("G,B,C", [(4, 3, 8), (3, 4, 8)])
def test_identities_with_exclude(G, B, C, with_queue):
    """Every id < 0, and all ids distinct and >= 0 (the queue's distinct from them): the mode IS exclude, bit for bit."""
    from facl_amd.utils_my import circle_contrast, global_contrast
    x, xg, queue, order = _inputs(G, B, C, 5 if with_queue else 0)
    q = queue if with_queue else None
    for normalize, tau in ((False, 1.0), (True, 0.07)):
        kw = dict(normalize=normalize, temperature=tau, queue=q)
        lc = global_contrast(G, xg, x, None, mask="exclude", **kw)
        lo = circle_contrast(G, x, B, order=order, mask="exclude", **kw)
        for ids, qids in ((torch.full((B,), -1), torch.full((5,), -1)), (torch.full((B,), -7), torch.full((5,), -7)),
                          (torch.arange(B), torch.arange(5) + B), (torch.arange(B), torch.full((5,), -1))):
            ck = dict(kw, mask="class", key_classes=ids.int(), queue_classes=qids.int()[:5 if with_queue else 0] if with_queue else None)
            assert torch.equal(global_contrast(G, xg, x, None, **ck), lc)
            assert torch.equal(circle_contrast(G, x, B, order=order, **ck), lo)


def test_one_class_and_an_empty_queue_is_exactly_zero():
    """No negative at all: losses exactly 0, gradients finite and exactly 0 (the closed form treats the empty log-sum-exp
    explicitly; autograd of logsumexp over an all -inf row would give NaN)."""
    from facl_amd.utils_my import circle_contrast, global_contrast
    G, B, C = 4, 3, 8
    x, xg, queue, order = _inputs(G, B, C, 5)
    ids = torch.full((B,), 2, dtype=torch.int32)
    for q, qids in ((None, None), (queue[:0], torch.zeros(0, dtype=torch.int32)), (queue, torch.full((5,), 2, dtype=torch.int32))):
        for normalize, tau in ((False, 1.0), (True, 0.07)):
            xr, xgr = x.clone().requires_grad_(True), xg.clone().requires_grad_(True)
            kw = dict(normalize=normalize, temperature=tau, mask="class", key_classes=ids, queue=q, queue_classes=qids)
            lc = global_contrast(G, xgr, xr, None, **kw)
            lo = circle_contrast(G, xr, B, order=order, **kw)
            assert float(lc.detach()) == 0.0 and float(lo.detach()) == 0.0
            gx, gg = torch.autograd.grad(lc + lo, (xr, xgr))
            assert torch.isfinite(gx).all() and torch.isfinite(gg).all()
            assert not gx.any() and not gg.any()
    # one clip of the batch without a negative, the others with: finite everywhere, the clip's own terms are 0
    ids = torch.tensor([1, 1, 1], dtype=torch.int32)
    qids = torch.tensor([1, 1, 0, 1, 1], dtype=torch.int32)
    xr = x.clone().requires_grad_(True)
    lo = circle_contrast(G, xr, B, order=order, mask="class", key_classes=ids, queue=queue, queue_classes=qids)
    (gx,) = torch.autograd.grad(lo, xr)
    assert torch.isfinite(lo) and float(lo.detach()) > 0 and torch.isfinite(gx).all()


def test_unknown_ids_never_match_each_other():
    from facl_amd.utils_my import circle_contrast, global_contrast
    G, B, C = 3, 4, 8
    x, xg, queue, order = _inputs(G, B, C, 5)
    base = dict(queue=queue)
    want = (global_contrast(G, xg, x, None, mask="exclude", **base), circle_contrast(G, x, B, order=order, mask="exclude", **base))
    for ids, qids in (([-1, -1, -1, -1], [-1] * 5), ([-1, -2, -1, -2], [-2, -1, -2, -1, -1]), ([-5, -5, -5, -5], [-5] * 5)):
        kw = dict(base, mask="class", key_classes=torch.tensor(ids, dtype=torch.int32), queue_classes=torch.tensor(qids, dtype=torch.int32))
        assert torch.equal(global_contrast(G, xg, x, None, **kw), want[0])
        assert torch.equal(circle_contrast(G, x, B, order=order, **kw), want[1])


def test_check_loss_mode_and_the_keyword_refusals():
    from facl_amd.utils_my import MASK_MODES, check_loss_mode, circle_contrast, contrastive_losses_stacked, global_contrast
    assert MASK_MODES == {"zero": 0, "exclude": 1, "class": 2}
    assert check_loss_mode(1.0, "class", 2) == (1.0, 2) and check_loss_mode(0.25, "class") == (2.0, 2)
    with pytest.raises(ValueError, match="negative"):
        check_loss_mode(1.0, "class", 1)
    with pytest.raises(ValueError, match="'exclude' with one key clip leaves no negative"):
        check_loss_mode(1.0, "exclude", 1)
    G, B, C = 4, 3, 8
    x, xg, queue, order = _inputs(G, B, C, 5)
    ids = torch.zeros(B, dtype=torch.int32)
    with pytest.raises(ValueError, match="class ids"):
        global_contrast(G, xg, x, None, mask="class")
    with pytest.raises(ValueError, match="class ids"):
        circle_contrast(G, x, B, order=order, mask="exclude", key_classes=ids)
    with pytest.raises(ValueError, match="one class id per key clip"):
        global_contrast(G, xg, x, None, mask="class", key_classes=ids[:2])
    with pytest.raises(ValueError, match="per queue row"):
        global_contrast(G, xg, x, None, mask="class", key_classes=ids, queue=queue)
    st = torch.cat((x, xg)).float()
    with pytest.raises(ValueError, match="classes"):        # before any launch: no device needed
        contrastive_losses_stacked(G, st, order, mask="class")
    with pytest.raises(ValueError, match="classes"):
        contrastive_losses_stacked(G, st, order, mask="exclude", classes=ids)
    with pytest.raises(ValueError, match="classes"):
        contrastive_losses_stacked(G, st, order, classes=ids)


def test_new_symbols_are_declared_bound_and_exported_and_refuse_without_a_launch():
    from facl_amd import _lib, build
    build.build()
    lib = _lib.load_library()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "facl_hip.h")).read(), flags=re.S)
    for s in ENTRIES:
        m = re.search(r"int\s+%s\s*\(([^)]*)\)" % s, hdr)
        assert m, s
        assert s in _lib.SIGNATURES and hasattr(lib, s), s
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[s]), s
    one = 16                                                # any non-NULL address: nothing is launched
    pair = lambda G_, B_, Bk_, J_, off, cls=one, ws=one: lib.facl_contrast_pair_sum_cls(one, G_, B_, Bk_, J_, one, off, cls, one, one, one, ws, None)
    assert pair(4, 3, 3, 12, 0, cls=None) == -2 and pair(4, 3, 3, 12, 0, ws=None) == -2
    for bad in ((1, 3, 3, 3, 0), (4, 3, 3, 13, 0), (4, 3, 3, 12, 1), (4, 3, 3, 12, -1), (4, 1, 1, 4, 0), (4, 0, 3, 12, 0)):
        assert pair(*bad) == -1, bad
    qu = lambda G_, B_, Bk_, J_, L_, off, cls=one, qcls=one, qs=one: lib.facl_contrast_pair_queue_cls(
        one, one, G_, B_, Bk_, J_, L_, one, off, cls, qcls, qs, one, one, one, one, one, None)
    assert qu(4, 3, 3, 12, 8, 0, cls=None) == -2 and qu(4, 3, 3, 12, 8, 0, qcls=None) == -2 and qu(4, 3, 3, 12, 8, 0, qs=None) == -2
    for bad in ((4, 3, 3, 12, 0, 0), (1, 3, 3, 3, 8, 0), (4, 3, 3, 13, 8, 0), (4, 3, 3, 12, 8, 1), (4, 1, 1, 4, 8, 0),
                (4, 60000, 60000, 240000, 8, 0)):
        assert qu(*bad) == -1, bad
    # the entries with a mask_mode argument know no mode 2
    assert lib.facl_contrast_pair_sum_mask(one, 4, 3, 3, 12, one, 0, 2, one, one, one, one, None) == -1
    assert lib.facl_contrast_pair_queue(one, one, 4, 3, 3, 12, 8, one, 0, 2, one, one, one, one, one, one, None) == -1
    for P, L in ((3, 10), (0, 12), (3, 0), (5, 3)):
        assert lib.facl_queue_push_ids(one, P, one, L, one, None) == -1, (P, L)
    for args in ((None, 3, one, 12, one), (one, 3, None, 12, one), (one, 3, one, 12, None)):
        assert lib.facl_queue_push_ids(*args, None) == -2, args


def test_flags_and_refusals():
    from facl_amd import finetune
    from facl_amd.train_common import build_parser, check_class_mask_flags, check_loss_flags
    p = build_parser('0')
    d = p.parse_args([])
    assert (d.loss_mask, d.label_fraction, d.label_seed) == ("zero", 1.0, 0)
    check_class_mask_flags(d, world=4)                      # off: nothing to refuse
    ok = p.parse_args(["--loss_mask", "class", "--synthetic", "0", "--label_fraction", "0.5", "--label_seed", "3"])
    assert (ok.loss_mask, ok.label_fraction, ok.label_seed) == ("class", 0.5, 3)
    check_class_mask_flags(ok, world=1)
    check_loss_flags(ok, world=1)
    with pytest.raises(RuntimeError, match="runs on one rank only"):
        check_class_mask_flags(ok, world=2)
    for syn in ("1", "2"):
        with pytest.raises(RuntimeError, match="no labelled clips"):
            check_class_mask_flags(p.parse_args(["--loss_mask", "class", "--synthetic", syn]), world=1)
    for bad in ("0", "-0.5", "1.5", "nan"):
        with pytest.raises(RuntimeError, match=r"--label_fraction must be in \(0, 1\]"):
            check_class_mask_flags(p.parse_args(["--loss_mask", "class", "--synthetic", "0", "--label_fraction", bad]), world=1)
    with pytest.raises(RuntimeError, match="negative"):
        check_loss_flags(p.parse_args(["--loss_mask", "class", "--batchSize", "1"]), world=1)
    with pytest.raises(SystemExit):
        p.parse_args(["--loss_mask", "supcon"])
    # fine-tuning: the two flags still parse with their defaults and help, and any non-default mask is refused
    fp = finetune.finetune_parser()
    o = fp.parse_args(["--label_fraction", "0.5", "--label_seed", "3"])
    assert (o.label_fraction, o.label_seed) == (0.5, 3)
    assert (fp.parse_args([]).label_fraction, fp.parse_args([]).label_seed) == (1.0, 0)
    finetune.check_finetune_flags(o, world=1)
    with pytest.raises(RuntimeError, match="contrastive loss"):
        finetune.check_finetune_flags(fp.parse_args(["--loss_mask", "class"]), world=1)


def test_training_entry_refuses_before_the_device(monkeypatch):
    from facl_amd import cn3d_train_motion_GL
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    base = ["--nepoch", "1", "--batchSize", "4", "--loss_mask", "class"]
    with pytest.raises(RuntimeError, match="no labelled clips"):
        cn3d_train_motion_GL.main(base + ["--synthetic", "1"])
    with pytest.raises(RuntimeError, match="label_fraction"):
        cn3d_train_motion_GL.main(base + ["--synthetic", "0", "--view_rng", "philox", "--label_fraction", "0"])
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(RuntimeError, match="runs on one rank only"):
        cn3d_train_motion_GL.main(base + ["--synthetic", "0", "--view_rng", "philox"])


def test_label_fraction_gives_the_nested_stratified_id_vector():
    from facl_amd.finetune import label_subset
    from facl_amd.train_common import split_class_ids
    labels = np.array([i % 5 for i in range(60)] + [5] * 3)
    prev = None
    for f in (0.1, 0.34, 0.5, 1.0):
        ids = split_class_ids(labels, f, 7)
        assert ids.dtype == np.int32 and ids.shape == labels.shape
        keep = label_subset(labels, f, 7)
        assert np.array_equal(np.flatnonzero(ids >= 0), keep)
        assert np.array_equal(ids[keep], labels[keep]) and (np.delete(ids, keep) == -1).all()
        for c in range(6):                                   # stratified: ceil(f n_c) of every class, at least one
            assert (ids == c).sum() == max(1, int(np.ceil(f * (labels == c).sum())))
        if prev is not None:                                 # nested in f
            assert (ids[prev >= 0] == prev[prev >= 0]).all()
        prev = ids
    assert np.array_equal(split_class_ids(labels, 1.0, 0), labels)
    assert not np.array_equal(split_class_ids(labels, 0.34, 7), split_class_ids(labels, 0.34, 8))
    with pytest.raises(ValueError, match="label_fraction"):
        split_class_ids(labels, 0.0, 0)


def test_trajectory_flags_and_a_state_from_before_them(tmp_path):
    from facl_amd import train_state as ts
    from facl_amd.train_common import build_parser
    opt = build_parser('0').parse_args([])
    for k, v in (("label_fraction", 1.0), ("label_seed", 0)):
        assert k in ts.TRAJECTORY_FLAGS and ts.LATER_FLAG_DEFAULTS[k] == v == getattr(opt, k)
    flags = ts.flags_of(opt)
    old = {k: v for k, v in flags.items() if k not in ("label_fraction", "label_seed")}
    state = ts.assemble(0, 3, old, {}, {}, {"queue": None, "key_encoder": None, "swav": None}, ts.capture_rng())
    path = str(tmp_path / "state_0.pth")
    ts.write_atomic(state, path)
    back = ts.load_state(path)
    assert (back["flags"]["label_fraction"], back["flags"]["label_seed"]) == (1.0, 0)
    ts.check_compatible(back["flags"], opt)                  # resumes a default run
    other = build_parser('0').parse_args(["--label_fraction", "0.5"])
    with pytest.raises(RuntimeError, match="label_fraction"):
        ts.check_compatible(back["flags"], other)


def test_queue_snapshot_and_restore_with_and_without_ids():
    from facl_amd.neg_queue import NegativeQueue
    q = NegativeQueue(8, 4, 4, "cpu")
    assert q.ids is None and len(q.snapshot()) == 2
    q.buf.fill_(2.0)
    q.state.copy_(torch.tensor([4, 4], dtype=torch.int32))
    snap = q.snapshot()
    q.restore()
    assert not q.buf.any() and q.head_valid() == (0, 0)
    q.restore(snap)                                          # the 2-tuple, as before
    assert bool((q.buf == 2.0).all()) and q.head_valid() == (4, 4)
    with pytest.raises(ValueError):
        q.restore(snap + (torch.zeros(8, dtype=torch.int32),))
    w = NegativeQueue(8, 4, 4, "cpu", with_ids=True)
    assert w.ids.dtype == torch.int32 and w.ids.tolist() == [-1] * 8 and w.valid_ids().numel() == 0
    w.buf.fill_(3.0)
    w.state.copy_(torch.tensor([4, 8], dtype=torch.int32))
    w.ids.copy_(torch.arange(8, dtype=torch.int32))
    snap = w.snapshot()
    assert len(snap) == 3 and snap[2].data_ptr() != w.ids.data_ptr()
    ptr = w.ids.data_ptr()
    w.restore()
    assert w.ids.tolist() == [-1] * 8 and not w.buf.any() and w.head_valid() == (0, 0)
    w.restore(snap)
    assert w.ids.tolist() == list(range(8)) and w.head_valid() == (4, 8) and w.ids.data_ptr() == ptr      # in place
    assert w.valid_ids().tolist() == list(range(8))
    with pytest.raises(ValueError):
        w.restore(snap[:2])
    w.stage(torch.zeros(4, 4), ids=torch.zeros(4, dtype=torch.int32))
    w.restore(snap)
    with pytest.raises(RuntimeError, match="nothing was staged"):
        w.push()


def _cpu_step(mask, neg_queue=8):
    from facl_amd.train_common import ContrastiveStep
    net = torch.nn.Linear(2, 2)
    opt = argparse.Namespace(SAMPLE_NUM=512, batchSize=4, loss_normalize=1, loss_temperature=0.1, loss_mask=mask, neg_queue=neg_queue)
    return ContrastiveStep(net, None, opt, 4)


def test_step_owns_the_class_ids_and_its_state_carries_the_queue_ids():
    from facl_amd.neg_queue import NegativeQueue
    step = _cpu_step("class")
    assert step.clip_classes.dtype == torch.int32 and step.clip_classes.tolist() == [-1] * 4
    assert _cpu_step("exclude").clip_classes is None
    saved = {"queue": {"buf": torch.ones(8, 16), "state": torch.tensor([4, 4], dtype=torch.int32)}, "key_encoder": None, "swav": None}
    with pytest.raises(RuntimeError, match="ids"):
        step.load_state_dict(saved)                          # a class-mask run needs the ids of the saved rows
    other = _cpu_step("exclude")
    other.load_state_dict(saved)                             # as today for another mask
    assert other.queue.ids is None and other.queue.head_valid() == (4, 4) and set(other.state_dict()["queue"]) == {"buf", "state"}
    saved["queue"]["ids"] = torch.tensor([3, 1, -1, 2, -1, -1, -1, -1], dtype=torch.int32)
    step.load_state_dict(saved)
    assert isinstance(step.queue, NegativeQueue) and step.queue.ids.tolist() == [3, 1, -1, 2, -1, -1, -1, -1]
    sd = step.state_dict()["queue"]
    assert set(sd) == {"buf", "state", "ids"} and sd["ids"] is step.queue.ids
