"""Class-mates as extra positives of the contrastive losses (--class_positives), host side: the fp64 closed forms of
facl_amd.utils_my with ``class_positives`` against a loop over clips, rows and cells, the identities with ``mask='exclude'``, the
empty negative set, the ordering against ``mask='class'``, the refusals, the C ABI symbols, the flags and the saved state."""
import math
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("facl_contrast_pair_sum_sup", "facl_contrast_pair_queue_sup")
MODES = ((False, 1.0), (True, 0.07))                        # the (normalize, tau) pairs of test_loss_class_cpu.py


def _inputs(G, B, C, Q, seed=11):
    torch.manual_seed(seed + G * 10 + B)
    x = torch.randn(G * B, C, dtype=torch.float64) * 1.5
    xg = torch.randn(B, C, dtype=torch.float64) * 1.5
    queue = torch.randn(Q, C, dtype=torch.float64) * 1.5
    return x, xg, queue, np.random.RandomState(3).permutation(G)


def _lae(a, b):
    m = max(a, b)
    return m + math.log(math.exp(a - m) + math.exp(b - m))


def _explicit(xg, x, queue, order, G, B, ids, qids, lam):
    """(loss_c, loss_circle, cells) of the issue's contract, one clip, one anchor row and one cell at a time, in Python floats:
    the negatives are the cells that are neither the clip's own nor of its known class, lse their log-sum-exp over all the clip's
    rows; every own slot adds term(pos), and the class cells C -- other clips' columns and queue rows with the anchor's known id
    -- add (lam nS / |C|) sum term(v).  A clip without a negative adds nothing.  cells: |C| per (loss, clip)."""
    xv = x.view(G, B, -1)
    keys = [(g, b) for g in range(G) for b in range(B)]      # column j = g * B + b belongs to clip b
    loss, cells = [0.0, 0.0], [[0] * B, [0] * B]
    for n in range(B):
        mine = int(ids[n])
        specs = ((0, [xg[n]], [(xg[n], xv[g, n]) for g in range(G)]),
                 (1, [xv[order[i], n] for i in range(G - 1)], [(xv[order[i], n], xv[order[i + 1], n]) for i in range(G - 1)]))
        for which, rows, slots in specs:
            negatives, cell_values = [], []
            for a in rows:
                for g, b in keys:
                    v = float((a * xv[g, b]).sum())
                    if b == n:
                        continue                             # own clip: neither a negative nor a class cell
                    if mine >= 0 and int(ids[b]) == mine:
                        cell_values.append(v)
                    else:
                        negatives.append(v)
                for k in range(queue.shape[0]):
                    v = float((a * queue[k]).sum())
                    if mine >= 0 and int(qids[k]) == mine:
                        cell_values.append(v)
                    else:
                        negatives.append(v)
            cells[which][n] = len(cell_values)
            if not negatives:
                continue
            m = max(negatives)
            lse = m + math.log(sum(math.exp(v - m) for v in negatives))
            total = sum(_lae(float((a * k).sum()), lse) - float((a * k).sum()) for a, k in slots)
            if cell_values:
                total += lam * len(slots) / len(cell_values) * sum(_lae(v, lse) - v for v in cell_values)
            loss[which] += total / B
    return loss[0], loss[1], cells


# per B: in-batch mates (and a queue mate); mates only in the queue; an unknown anchor beside in-batch mates
IDS = {3: [([0, 1, 0], [0, -1, 1, 2, 0]), ([0, 1, 2], [2, -1, 5, 2, 7]), ([-1, 3, 3], [9, -1, 3, 9, 9])],
       4: [([0, 1, 0, 2], [0, -1, 1, 2, 0]), ([0, 1, 2, 3], [3, -1, 5, 3, 7]), ([-1, 0, -1, 0], [9, -1, 0, 9, 9])]}


@pytest.mark.parametrize("lam", [1.0, 0.25])
@pytest.mark.parametrize("with_queue", [False, True])
@pytest.mark.parametrize("G,B,C", [(4, 3, 8), (3, 4, 8)])
def test_closed_forms_vs_explicit_loop_fp64(G, B, C, with_queue, lam):
    from facl_amd.utils_my import circle_contrast, global_contrast
    x, xg, queue, order = _inputs(G, B, C, 5 if with_queue else 0)
    seen_batch = seen_queue_only = seen_unknown = False
    for k, (ids, qids) in enumerate(IDS[B]):
        ids = torch.tensor(ids, dtype=torch.int32)
        qids = torch.tensor(qids[:queue.shape[0]], dtype=torch.int32)
        for normalize, tau in MODES:
            kw = dict(normalize=normalize, temperature=tau, mask="class", key_classes=ids, class_positives=lam,
                      queue=queue if with_queue else None, queue_classes=qids if with_queue else None)
            lc = global_contrast(G, xg, x, None, **kw)
            lo = circle_contrast(G, x, B, order=order, **kw)
            s = float(np.float32(1.0 / np.sqrt(tau)))
            rows = (lambda t: t / t.norm(dim=1, keepdim=True).clamp_min(1e-12) * s) if normalize else (lambda t: t * s)
            rc, ro, cells = _explicit(rows(xg), rows(x), queue, order, G, B, ids.tolist(), qids.tolist(), lam)
            assert abs(float(lc) - rc) <= 1e-12 * abs(rc), (k, normalize)
            assert abs(float(lo) - ro) <= 1e-12 * abs(ro), (k, normalize)
        in_batch = any(ids[a] >= 0 and ids[a] == ids[b] for a in range(B) for b in range(B) if a != b)
        seen_batch |= in_batch
        seen_queue_only |= with_queue and not in_batch and sum(cells[0]) > 0
        seen_unknown |= bool((ids < 0).any()) and sum(cells[0]) > 0
    assert seen_batch and seen_unknown and (seen_queue_only or not with_queue)


@pytest.mark.parametrize("with_queue", [False, True])
@pytest.mark.parametrize("G,B,C", [(4, 3, 8), (3, 4, 8)])
def test_without_class_mates_it_is_exclude(G, B, C, with_queue):
    """Every id < 0, and all ids distinct (the queue's distinct from them): no class cell, the value IS exclude's, bit for bit."""
    from facl_amd.utils_my import circle_contrast, global_contrast
    x, xg, queue, order = _inputs(G, B, C, 5 if with_queue else 0)
    q = queue if with_queue else None
    for normalize, tau in MODES:
        kw = dict(normalize=normalize, temperature=tau, queue=q)
        lc = global_contrast(G, xg, x, None, mask="exclude", **kw)
        lo = circle_contrast(G, x, B, order=order, mask="exclude", **kw)
        for ids, qids in ((torch.full((B,), -1), torch.full((5,), -1)), (torch.full((B,), -7), torch.full((5,), -7)),
                          (torch.arange(B), torch.arange(5) + B), (torch.arange(B), torch.full((5,), -1))):
            for lam in (1.0, 0.25):
                ck = dict(kw, mask="class", key_classes=ids.int(), class_positives=lam,
                          queue_classes=qids.int() if with_queue else None)
                assert torch.equal(global_contrast(G, xg, x, None, **ck), lc)
                assert torch.equal(circle_contrast(G, x, B, order=order, **ck), lo)


def test_one_class_everywhere_is_exactly_zero():
    """No negative at all while every other cell is a class cell: losses exactly 0, gradients finite and exactly 0."""
    from facl_amd.utils_my import circle_contrast, global_contrast
    G, B, C = 4, 3, 8
    x, xg, queue, order = _inputs(G, B, C, 5)
    ids = torch.full((B,), 2, dtype=torch.int32)
    for q, qids in ((None, None), (queue, torch.full((5,), 2, dtype=torch.int32))):
        for normalize, tau in MODES:
            xr, xgr = x.clone().requires_grad_(True), xg.clone().requires_grad_(True)
            kw = dict(normalize=normalize, temperature=tau, mask="class", key_classes=ids, queue=q, queue_classes=qids,
                      class_positives=1.0)
            lc = global_contrast(G, xgr, xr, None, **kw)
            lo = circle_contrast(G, xr, B, order=order, **kw)
            assert float(lc.detach()) == 0.0 and float(lo.detach()) == 0.0
            gx, gg = torch.autograd.grad(lc + lo, (xr, xgr))
            assert torch.isfinite(gx).all() and torch.isfinite(gg).all()
            assert not gx.any() and not gg.any()


def test_value_is_above_the_class_mask_and_the_mates_get_a_gradient():
    from facl_amd.utils_my import circle_contrast, global_contrast
    G, B, C = 4, 3, 8
    x, xg, queue, order = _inputs(G, B, C, 5)
    ids = torch.tensor([0, 1, 0], dtype=torch.int32)
    qids = torch.tensor([1, -1, 2, 2, 1], dtype=torch.int32)
    for normalize, tau in MODES:
        base = dict(normalize=normalize, temperature=tau, mask="class", key_classes=ids, queue=queue, queue_classes=qids)
        for lam in (1.0, 0.25):
            assert float(global_contrast(G, xg, x, None, class_positives=lam, **base)) > float(global_contrast(G, xg, x, None, **base))
            assert float(circle_contrast(G, x, B, order=order, class_positives=lam, **base)) > \
                float(circle_contrast(G, x, B, order=order, **base))
    # one local anchor clip (clip 0 of three key clips, the data-parallel form): the key rows of its mate, clip 2, are masked
    # under the class mask and get no gradient at all; as positives every view of the mate gets one
    xl = x.view(G, B, C)[:, 0].contiguous()
    for lam, moved in ((0.0, False), (1.0, True)):
        keys = x.clone().requires_grad_(True)
        kw = dict(x_keys=keys, clip_offset=0, mask="class", key_classes=ids, class_positives=lam)
        (gk,) = torch.autograd.grad(global_contrast(G, xg[:1], xl, None, **kw) + circle_contrast(G, xl, 1, order=order, **kw), keys)
        mate_rows = gk.view(G, B, C)[:, 2]
        assert bool((mate_rows.abs().sum(dim=1) > 0).all()) == moved and bool(mate_rows.any()) == moved
        assert bool(gk.view(G, B, C)[:, 1].any())            # clip 1 stays a negative


def test_refusals():
    from facl_amd.utils_my import check_class_positives, circle_contrast, contrastive_losses_stacked, global_contrast
    G, B, C = 4, 3, 8
    x, xg, queue, order = _inputs(G, B, C, 5)
    ids = torch.tensor([0, 1, 0], dtype=torch.int32)
    assert check_class_positives(0.0, "zero") == 0.0 and check_class_positives(0.5, "class") == 0.5
    for mask in ("exclude", "zero"):
        with pytest.raises(ValueError, match="mask 'class'"):
            global_contrast(G, xg, x, None, mask=mask, class_positives=1.0)
        with pytest.raises(ValueError, match="mask 'class'"):
            circle_contrast(G, x, B, order=order, mask=mask, class_positives=1.0)
    st = torch.cat((x, xg)).float()
    with pytest.raises(ValueError, match="mask 'class'"):    # before any launch: no device needed
        contrastive_losses_stacked(G, st, order, mask="exclude", class_positives=1.0)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="finite"):
            global_contrast(G, xg, x, None, mask="class", key_classes=ids, class_positives=bad)
        with pytest.raises(ValueError, match="finite"):
            circle_contrast(G, x, B, order=order, mask="class", key_classes=ids, class_positives=bad)
        with pytest.raises(ValueError, match="finite"):
            contrastive_losses_stacked(G, st, order, mask="class", classes=ids, class_positives=bad)


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
    pair = lambda G_, B_, Bk_, J_, off, cls=one, ws=one, pw=1.0: lib.facl_contrast_pair_sum_sup(
        one, G_, B_, Bk_, J_, one, off, cls, pw, one, one, one, ws, None)
    assert pair(4, 3, 3, 12, 0, cls=None) == -2 and pair(4, 3, 3, 12, 0, ws=None) == -2
    for bad in ((1, 3, 3, 3, 0), (4, 3, 3, 13, 0), (4, 3, 3, 12, 1), (4, 3, 3, 12, -1), (4, 1, 1, 4, 0), (4, 0, 3, 12, 0)):
        assert pair(*bad) == -1, bad
    qu = lambda G_, B_, Bk_, J_, L_, off, cls=one, qcls=one, qs=one, ws=one, pw=1.0: lib.facl_contrast_pair_queue_sup(
        one, one, G_, B_, Bk_, J_, L_, one, off, cls, qcls, qs, pw, one, one, one, one, ws, None)
    ok = (4, 3, 3, 12, 8, 0)
    assert qu(*ok, cls=None) == -2 and qu(*ok, qcls=None) == -2 and qu(*ok, qs=None) == -2 and qu(*ok, ws=None) == -2
    for bad in ((4, 3, 3, 12, 0, 0), (1, 3, 3, 3, 8, 0), (4, 3, 3, 13, 8, 0), (4, 3, 3, 12, 8, 1), (4, 1, 1, 4, 8, 0),
                (4, 60000, 60000, 240000, 8, 0)):
        assert qu(*bad) == -1, bad
    for pw in (0.0, -1.0, float("nan"), float("inf")):
        assert pair(4, 3, 3, 12, 0, pw=pw) == -1, pw
        assert qu(*ok, pw=pw) == -1, pw
    # the workspace check covers the new per-chunk arrays: 32 bytes per chunk partial instead of 12
    ws_bytes = int(lib.facl_ws_bytes())
    G_, nch = 4, 119                                         # J = 4 * 60000 columns: 118 chunks, and one of the queue
    B_fit = ws_bytes // ((G_ + 1) * nch * 20)                # fits 12 + 8 bytes per partial and clip pair ...
    assert (2 * B_fit + (G_ + 1) * B_fit * nch) * 8 + (G_ + 1) * B_fit * nch * 4 <= ws_bytes
    assert (2 * B_fit + 3 * (G_ + 1) * B_fit * nch) * 8 + (G_ + 1) * B_fit * nch * 8 > ws_bytes      # ... but not 32
    assert B_fit <= 60000
    assert lib.facl_contrast_pair_queue_sup(one, one, G_, B_fit, 60000, 240000, 8, one, 0, one, one, one, 1.0, one, one, one, one,
                                            one, None) == -1
    # the entries with a mask_mode argument know neither mode 2 nor mode 3
    for mode in (2, 3):
        assert lib.facl_contrast_pair_sum_mask(one, 4, 3, 3, 12, one, 0, mode, one, one, one, one, None) == -1
        assert lib.facl_contrast_pair_queue(one, one, 4, 3, 3, 12, 8, one, 0, mode, one, one, one, one, one, one, None) == -1


def test_flags_and_refusals():
    from facl_amd import finetune
    from facl_amd.train_common import build_parser, check_class_mask_flags
    p = build_parser('0')
    assert p.parse_args([]).class_positives == 0.0
    check_class_mask_flags(p.parse_args([]), world=4)       # off: nothing to refuse
    ok = p.parse_args(["--loss_mask", "class", "--synthetic", "0", "--class_positives", "0.25"])
    assert ok.class_positives == 0.25
    check_class_mask_flags(ok, world=1)
    with pytest.raises(RuntimeError, match="runs on one rank only"):       # inherited from the mask
        check_class_mask_flags(ok, world=2)
    with pytest.raises(RuntimeError, match="no labelled clips"):
        check_class_mask_flags(p.parse_args(["--loss_mask", "class", "--synthetic", "1", "--class_positives", "1"]), world=1)
    for mask in ("zero", "exclude"):
        with pytest.raises(RuntimeError, match="--class_positives.*mask 'class'"):
            check_class_mask_flags(p.parse_args(["--loss_mask", mask, "--class_positives", "1"]), world=1)
    for bad in ("-0.5", "nan", "inf"):
        with pytest.raises(RuntimeError, match="--class_positives.*finite"):
            check_class_mask_flags(p.parse_args(["--loss_mask", "class", "--synthetic", "0", "--class_positives", bad]), world=1)
    assert p.parse_args([]).loss_mask == "zero"              # and the flag is no fourth mask
    fp = finetune.finetune_parser()
    finetune.check_finetune_flags(fp.parse_args([]), world=1)
    with pytest.raises(RuntimeError, match="class_positives"):
        finetune.check_finetune_flags(fp.parse_args(["--class_positives", "1"]), world=1)


def test_training_entry_refuses_before_the_device(monkeypatch):
    from facl_amd import cn3d_train_motion_GL
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    base = ["--nepoch", "1", "--batchSize", "4", "--synthetic", "0", "--view_rng", "philox"]
    with pytest.raises(RuntimeError, match="--class_positives.*mask 'class'"):
        cn3d_train_motion_GL.main(base + ["--class_positives", "1"])
    with pytest.raises(RuntimeError, match="--class_positives.*mask 'class'"):
        cn3d_train_motion_GL.main(base + ["--loss_mask", "exclude", "--class_positives", "1"])
    with pytest.raises(RuntimeError, match="--class_positives.*finite"):
        cn3d_train_motion_GL.main(base + ["--loss_mask", "class", "--class_positives", "-1"])
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(RuntimeError, match="runs on one rank only"):
        cn3d_train_motion_GL.main(base + ["--loss_mask", "class", "--class_positives", "1"])


def test_step_keeps_the_weight_beside_the_loss_mode():
    import argparse
    from facl_amd.train_common import ContrastiveStep
    net = torch.nn.Linear(2, 2)
    mk = lambda **kw: ContrastiveStep(net, None, argparse.Namespace(SAMPLE_NUM=512, batchSize=4, loss_normalize=1, loss_temperature=0.1,
                                                                    neg_queue=8, **kw), 4)
    step = mk(loss_mask="class", class_positives=0.5)
    assert step.class_positives == 0.5
    assert step.loss_mode == dict(normalize=True, temperature=0.1, mask="class")
    assert mk(loss_mask="class").class_positives == 0.0      # a namespace from before the flag
    with pytest.raises(ValueError, match="mask 'class'"):
        mk(loss_mask="exclude", class_positives=0.5)


def test_trajectory_flag_and_a_state_from_before_it(tmp_path):
    from facl_amd import train_state as ts
    from facl_amd.train_common import build_parser
    opt = build_parser('0').parse_args([])
    assert "class_positives" in ts.TRAJECTORY_FLAGS and ts.LATER_FLAG_DEFAULTS["class_positives"] == 0.0 == opt.class_positives
    flags = ts.flags_of(opt)
    assert flags["class_positives"] == 0.0
    old = {k: v for k, v in flags.items() if k != "class_positives"}
    state = ts.assemble(0, 3, old, {}, {}, {"queue": None, "key_encoder": None, "swav": None}, ts.capture_rng())
    path = str(tmp_path / "state_0.pth")
    ts.write_atomic(state, path)
    back = ts.load_state(path)
    assert back["flags"]["class_positives"] == 0.0
    ts.check_compatible(back["flags"], opt)                  # resumes a default run
    other = build_parser('0').parse_args(["--class_positives", "0.5"])
    with pytest.raises(RuntimeError, match="class_positives"):
        ts.check_compatible(back["flags"], other)
