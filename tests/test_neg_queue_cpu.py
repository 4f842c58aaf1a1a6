"""Cross-batch queue of negative keys (--neg_queue), host side: the fp64 closed forms of facl_amd.utils_my with ``queue=``
against materialised logits through F.cross_entropy, the new C ABI symbols, the launcher's constants and the flag refusals."""
import itertools
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G, B, C = 4, 3, 16
MODES = list(itertools.product((False, True), (1.0, 0.07), ("zero", "exclude")))
ENTRIES = ("facl_contrast_pair_queue", "facl_queue_push")


def _rows(x, normalize, tau):
    s = float(np.float32(1.0 / np.sqrt(tau)))
    if normalize:
        x = x / x.norm(dim=1, keepdim=True).clamp_min(1e-12)
    return x * s


def _negatives(sim_rows, clip, Bk, mask):
    """sim_rows (A, G*Bk) of ONE clip -> its shared negative set: same-clip columns zeroed in place, or physically removed."""
    same = (torch.arange(sim_rows.shape[1]) % Bk) == clip
    if mask == "zero":
        return torch.where(same[None, :], torch.zeros((), dtype=sim_rows.dtype), sim_rows).reshape(-1)
    return sim_rows[:, ~same].reshape(-1)


def _materialised(xg, x, keys, queue, order, off, normalize, tau, mask):
    """(loss_c, loss_circle) the long way: per anchor slot the logits [positive | negatives of the clip | queue columns of the
    clip's anchors], label 0, F.cross_entropy with mean over the B clips, summed over the slots.  The queue rows are used as
    they are (not mapped)."""
    xg, x, keys = _rows(xg, normalize, tau), _rows(x, normalize, tau), _rows(keys, normalize, tau)
    Bk = keys.shape[0] // G
    xv = x.view(G, B, C)
    label = torch.zeros(1, dtype=torch.long)
    loss_c = torch.zeros((), dtype=x.dtype)
    loss_o = torch.zeros((), dtype=x.dtype)
    for n in range(B):
        neg_g = torch.cat((_negatives((xg[n:n + 1] @ keys.t()), n + off, Bk, mask), (xg[n:n + 1] @ queue.t()).reshape(-1)))
        for g in range(G):
            pos = (xg[n] * xv[g, n]).sum().reshape(1)
            loss_c = loss_c + F.cross_entropy(torch.cat((pos, neg_g))[None, :], label) / B
        anchors = torch.stack([xv[order[i], n] for i in range(G - 1)])
        neg_o = torch.cat((_negatives(anchors @ keys.t(), n + off, Bk, mask), (anchors @ queue.t()).reshape(-1)))
        for i in range(G - 1):
            pos = (xv[order[i], n] * xv[order[i + 1], n]).sum().reshape(1)
            loss_o = loss_o + F.cross_entropy(torch.cat((pos, neg_o))[None, :], label) / B
    return loss_c, loss_o


def _inputs(world):
    torch.manual_seed(11)
    Bk, off = B * world, B * (world - 1)
    keys3 = torch.randn(G, Bk, C, dtype=torch.float64) * 1.5
    x = keys3[:, off:off + B].reshape(G * B, C).clone()
    xg = torch.randn(B, C, dtype=torch.float64) * 1.5
    queue = torch.randn(12, C, dtype=torch.float64) * 1.5
    return keys3.reshape(G * Bk, C), x, xg, queue, off, np.random.RandomState(3).permutation(G)


@pytest.mark.parametrize("world", [1, 2])
@pytest.mark.parametrize("valid", [0, 3, 12])
@pytest.mark.parametrize("normalize,tau,mask", MODES)
def test_closed_forms_with_queue_vs_materialised_logits_fp64(normalize, tau, mask, valid, world):
    from facl_amd.utils_my import circle_contrast, global_contrast
    keys, x, xg, queue, off, order = _inputs(world)
    kw = dict(normalize=normalize, temperature=tau, mask=mask, queue=queue[:valid])
    x_keys = keys if world > 1 else None
    lc = global_contrast(G, xg, x, None, x_keys=x_keys, clip_offset=off, **kw)
    lo = circle_contrast(G, x, B, order=order, x_keys=x_keys, clip_offset=off, **kw)
    rc, ro = _materialised(xg, x, keys, queue[:valid], order, off, normalize, tau, mask)
    assert abs(float(lc) - float(rc)) <= 1e-12 * abs(float(rc))
    assert abs(float(lo) - float(ro)) <= 1e-12 * abs(float(ro))
    if valid:                                               # more negatives never lower a value (equal where it is saturated)
        kw0 = dict(kw, queue=None)
        assert float(lc) >= float(global_contrast(G, xg, x, None, x_keys=x_keys, clip_offset=off, **kw0))
        assert float(lo) >= float(circle_contrast(G, x, B, order=order, x_keys=x_keys, clip_offset=off, **kw0))


@pytest.mark.parametrize("normalize,tau,mask", [(False, 1.0, "zero"), (True, 0.07, "exclude")])
def test_no_queue_and_empty_queue_are_todays_closed_form(normalize, tau, mask):
    """queue=None and a queue without rows: the same bits as the call without the keyword."""
    from facl_amd.utils_my import circle_contrast, global_contrast
    keys, x, xg, queue, off, order = _inputs(1)
    kw = dict(normalize=normalize, temperature=tau, mask=mask)
    lc, lo = global_contrast(G, xg, x, None, **kw), circle_contrast(G, x, B, order=order, **kw)
    for q in (None, queue[:0]):
        assert torch.equal(global_contrast(G, xg, x, None, queue=q, **kw), lc)
        assert torch.equal(circle_contrast(G, x, B, order=order, queue=q, **kw), lo)


def test_new_symbols_are_declared_bound_and_exported():
    from facl_amd import _lib, build
    build.build()
    lib = _lib.load_library()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "facl_hip.h")).read(), flags=re.S)
    for s in ENTRIES:
        m = re.search(r"int\s+%s\s*\(([^)]*)\)" % s, hdr)
        assert m, s
        assert s in _lib.SIGNATURES and hasattr(lib, s), s
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[s]), s


def test_entries_refuse_without_a_launch():
    """The refusals come before any launch, so they run without a GPU: the push checks its shapes first (FACL_E_SHAPE), then
    its pointers (FACL_E_NULL); the loss entry its pointers first, like facl_contrast_pair_sum_mask."""
    from facl_amd import _lib, build
    build.build()
    lib = _lib.load_library()
    one = 16                                                # any non-NULL address: nothing is launched
    for P, Cc, L in ((3, 8, 10), (3, 6, 12), (3, 2, 12), (0, 8, 12), (3, 8, 0), (5, 8, 3)):
        assert lib.facl_queue_push(one, P, Cc, one, L, one, None) == -1, (P, Cc, L)
    for args in ((None, 3, 8, one, 12, one), (one, 3, 8, None, 12, one), (one, 3, 8, one, 12, None)):
        assert lib.facl_queue_push(*args, None) == -2, args
    assert lib.facl_queue_push(4, 3, 8, one, 12, one, None) == -3          # rows not 16-byte aligned
    call = lambda G_, B_, Bk_, J_, L_, off, mode, ws=one, qs=one: lib.facl_contrast_pair_queue(
        one, one, G_, B_, Bk_, J_, L_, one, off, mode, qs, one, one, one, one, ws, None)
    assert call(4, 3, 3, 12, 8, 0, 0, ws=None) == -2 and call(4, 3, 3, 12, 8, 0, 0, qs=None) == -2
    for bad in ((4, 3, 3, 12, 0, 0, 0), (4, 3, 3, 12, -4, 0, 0), (1, 3, 3, 3, 8, 0, 0), (4, 3, 3, 13, 8, 0, 0), (4, 3, 3, 12, 8, 1, 0),
                (4, 3, 3, 12, 8, 0, 2), (4, 1, 1, 4, 8, 0, 1), (4, 3, 3, 12, 8, -1, 0)):
        assert call(*bad) == -1, bad
    # more chunk partials than the workspace holds
    assert call(4, 60000, 60000, 240000, 8, 0, 0) == -1


def test_path_helpers_follow_the_launcher():
    """neg_queue_paths reads QC and QT out of csrc/loss.hip; the GPU tests' cases sit around 2048 columns per chunk, held as
    8 values in each of 256 threads.  The 16-byte path also needs every matrix on a 16-byte address."""
    import neg_queue_paths as nq
    assert (nq.CHUNK, nq.THREADS) == (2048, 256)
    assert nq.chunks(2048, 2049) == (1, 2) and nq.chunks(2049, 2048) == (2, 1)
    assert nq.vectorised(24, 12) and not nq.vectorised(30, 20) and not nq.vectorised(24, 10)
    m = torch.zeros(64)
    assert m.data_ptr() % 16 == 0
    assert nq.vectorised(24, 12, m, m[4:]) and not nq.vectorised(24, 12, m, m[1:])


def _PlainStep():
    """A step object of the shape GraphedStep wraps, WITHOUT a ``queue`` attribute (dense.DenseStep has none): the base class,
    which carries no state besides model and optimizer."""
    from facl_amd.train_step import TrainStep
    net = torch.nn.Sequential(torch.nn.Linear(3, 2), torch.nn.BatchNorm1d(2))
    return TrainStep(net, torch.optim.SGD(net.parameters(), lr=0.1), 2)


def test_graphed_step_state_of_a_step_without_a_queue_attribute():
    """GraphedStep._snapshot / _restore on a step class that knows no queue (dense.DenseStep: bench.py --config dense) and on
    one whose queue is None: no AttributeError, the snapshot's queue part is None and the parameters come back in place."""
    from facl_amd.dense import DenseStep
    from facl_amd.train_common import GraphedStep
    assert not hasattr(DenseStep(torch.nn.Linear(1, 1), None, 2), "queue")
    for with_none in (False, True):
        step = _PlainStep()
        if with_none:
            step.queue = None
        g = object.__new__(GraphedStep)                          # the state handling alone: a capture needs the device
        g.step = step
        snap = g._snapshot()
        assert snap[3] is None
        want = {k: v.clone() for k, v in step.netR.state_dict().items()}
        ptrs = {k: v.data_ptr() for k, v in step.netR.state_dict().items()}
        with torch.no_grad():
            for p in step.netR.parameters():
                p.add_(1.0)
        g._restore(snap)
        for k, v in step.netR.state_dict().items():
            assert torch.equal(v, want[k]) and v.data_ptr() == ptrs[k], k


def test_timing_tool_keeps_the_blocks_it_does_not_produce(tmp_path):
    """tools/time_neg_queue.py replaces its own keys in the results file and keeps the others: profiles/neg_queue.json also
    holds the recorded bench.py lines and the profiler's kernel times, which a re-run of the tool must not drop."""
    import importlib.util
    import json
    spec = importlib.util.spec_from_file_location("time_neg_queue", os.path.join(ROOT, "tools", "time_neg_queue.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    out = tmp_path / "sub" / "q.json"
    tool.write_results(str(out), {"queue_0_graph_ms": 1.0})                # no file yet
    assert json.loads(out.read_text()) == {"queue_0_graph_ms": 1.0}
    out.write_text(json.dumps({"bench_ab": {"parent": [1]}, "kernel_trace_L4096": {"x": 2}, "queue_0_graph_ms": 1.0}))
    tool.write_results(str(out), {"queue_0_graph_ms": 3.0, "config": {"B": 32}})
    assert json.loads(out.read_text()) == {"bench_ab": {"parent": [1]}, "kernel_trace_L4096": {"x": 2}, "queue_0_graph_ms": 3.0,
                                           "config": {"B": 32}}
    with open(os.path.join(ROOT, "profiles", "neg_queue.json")) as f:
        recorded = json.load(f)
    assert len(recorded["bench_ab"]["parent"]) == len(recorded["bench_ab"]["this"]) == 3 and "kernel_trace_L4096" in recorded


def test_parser_default_and_flag_refusals():
    from facl_amd.train_common import build_parser, check_queue_flags
    p = build_parser('0')
    assert p.parse_args([]).neg_queue == 0
    check_queue_flags(p.parse_args([]), world=1)
    check_queue_flags(p.parse_args([]), world=2)                           # off: nothing to refuse
    check_queue_flags(p.parse_args(["--neg_queue", "4096", "--batchSize", "32"]), world=1)
    with pytest.raises(RuntimeError, match="neg_queue"):
        check_queue_flags(p.parse_args(["--neg_queue", "-1"]), world=1)
    with pytest.raises(RuntimeError, match="multiple of --batchSize"):
        check_queue_flags(p.parse_args(["--neg_queue", "100", "--batchSize", "32"]), world=1)
    with pytest.raises(RuntimeError, match="one rank"):
        check_queue_flags(p.parse_args(["--neg_queue", "64", "--batchSize", "32"]), world=2)


def test_training_entry_refuses_before_the_device(monkeypatch):
    from facl_amd import cn3d_train_motion_GL
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(RuntimeError, match="multiple of --batchSize"):
        cn3d_train_motion_GL.main(["--synthetic", "1", "--nepoch", "1", "--batchSize", "4", "--neg_queue", "6"])
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(RuntimeError, match="one rank"):
        cn3d_train_motion_GL.main(["--synthetic", "1", "--nepoch", "1", "--batchSize", "4", "--neg_queue", "8"])


def test_finetune_refuses_the_queue():
    from facl_amd import finetune
    p = finetune.finetune_parser()
    with pytest.raises(RuntimeError, match="contrastive loss"):
        finetune.check_finetune_flags(p.parse_args(["--neg_queue", "64"]), world=1)


def test_queue_object_refuses_bad_sizes():
    from facl_amd.neg_queue import NegativeQueue
    for L, Cc, P in ((10, 8, 3), (0, 8, 3), (12, 6, 3), (12, 8, 0)):
        with pytest.raises(ValueError):
            NegativeQueue(L, Cc, P, "cpu")
    q = NegativeQueue(12, 8, 3, "cpu")                       # the buffers are plain zeroed tensors; the push is device-only
    assert q.head_valid() == (0, 0) and q.valid_rows().shape == (0, 8) and not q.buf.any()
    with pytest.raises(RuntimeError):
        q.push(torch.zeros(3, 8))
