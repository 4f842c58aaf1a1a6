"""Host side of the clustering feature (facl_amd/cluster.py, cluster_eval.py, --class_ids cluster): the scores on hand-made
tables, the assignment routine against brute force, the flag refusals, the header / bindings and the entries' refusals, which
all come before any launch (no GPU here)."""
import ctypes
import itertools
import math
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- scores -----------------------------------------------------------------------------------------------------------------------
def test_identical_and_permuted_partitions_score_perfectly():
    from facl_amd import cluster as fcl
    true = np.array([0, 0, 0, 1, 1, 2, 2, 2, 2, 3])
    for pred in (true, np.array([7, 5, 9, 2])[true]):             # a relabelling is the same partition
        t = fcl.contingency(pred, true)
        assert t.shape == (4, 4) and t.sum() == 10
        assert fcl.matched_accuracy(t) == 100.0 and fcl.purity(t) == 100.0
        assert abs(fcl.nmi(t) - 1.0) < 1e-12 and abs(fcl.ari(t) - 1.0) < 1e-12
    s = fcl.scores(np.array([7, 5, 9, 2])[true], true)
    assert s["acc"] == 100.0 and s["purity"] == 100.0 and abs(s["nmi"] - 1.0) < 1e-12 and abs(s["ari"] - 1.0) < 1e-12


def test_one_cluster_against_many_classes_scores_zero():
    from facl_amd import cluster as fcl
    true = np.array([0, 0, 1, 1, 2, 2, 2])
    t = fcl.contingency(np.zeros(7, dtype=np.int64), true)
    assert t.tolist() == [[2, 2, 3]]
    assert fcl.nmi(t) == 0.0 and fcl.ari(t) == 0.0
    assert fcl.purity(t) == pytest.approx(100.0 * 3 / 7) and fcl.matched_accuracy(t) == pytest.approx(100.0 * 3 / 7)
    # both partitions a single cluster: 0 / 0 is 1.0
    one = fcl.contingency(np.zeros(5, dtype=np.int64), np.ones(5, dtype=np.int64))
    assert fcl.nmi(one) == 1.0 and fcl.ari(one) == 1.0


def test_three_by_three_table_with_worked_out_values():
    from facl_amd import cluster as fcl
    t = np.array([[5, 1, 0], [1, 4, 1], [0, 2, 6]])
    pred = np.repeat(np.arange(3), t.sum(axis=1))
    true = np.concatenate([np.repeat(np.arange(3), row) for row in t])
    assert fcl.contingency(pred, true).tolist() == t.tolist()
    # ARI by hand: n = 20; sum C(nij, 2) = 10 + 6 + 15 + 1 = 32; rows 6, 6, 8 -> 15 + 15 + 28 = 58; columns 6, 7, 7 -> 15 + 21 + 21 = 57;
    # C(20, 2) = 190; expected = 58 * 57 / 190 = 17.4; max = 57.5
    want_ari = (32 - 17.4) / (57.5 - 17.4)
    assert abs(fcl.ari(t) - want_ari) < 1e-12
    # NMI by hand from the definitions
    n = 20.0
    a, b = [6, 6, 8], [6, 7, 7]
    mi = sum(v / n * math.log(v * n / (a[i] * b[j])) for i, row in enumerate(t.tolist()) for j, v in enumerate(row) if v)
    h = lambda c: -sum(v / n * math.log(v / n) for v in c)
    assert abs(fcl.nmi(t) - mi / (0.5 * (h(a) + h(b)))) < 1e-12
    assert fcl.purity(t) == 75.0 and fcl.matched_accuracy(t) == 75.0


def _brute(table):
    r, c = table.shape
    m = max(r, c)
    sq = np.zeros((m, m), dtype=np.int64)
    sq[:r, :c] = table
    return max(int(sq[np.arange(m), list(p)].sum()) for p in itertools.permutations(range(m)))


def test_matched_accuracy_against_brute_force():
    from facl_amd import cluster as fcl
    rng = np.random.RandomState(5)
    shapes = [(1, 1), (2, 2), (3, 5), (5, 3), (4, 4), (6, 6), (6, 2), (1, 6), (5, 6), (6, 5)]
    try:
        from scipy.optimize import linear_sum_assignment
    except ImportError:
        linear_sum_assignment = None
    for r, c in shapes:
        for trial in range(6):
            t = rng.randint(0, 9 if trial % 2 else 3, size=(r, c))             # few distinct values: many equal sums
            if t.sum() == 0:
                t[0, 0] = 1
            want = 100.0 * _brute(t) / t.sum()
            assert abs(fcl.matched_accuracy(t) - want) < 1e-9, (t.tolist(), want)
            if linear_sum_assignment is not None:                               # an additional assertion, never the only one
                i, j = linear_sum_assignment(-t)
                assert abs(fcl.matched_accuracy(t) - 100.0 * t[i, j].sum() / t.sum()) < 1e-9
    # the assignment itself is one-to-one and optimal on a float matrix
    cost = rng.rand(7, 7)
    col = fcl.assign_min(cost)
    assert sorted(col.tolist()) == list(range(7))
    best = min(sum(cost[i, p[i]] for i in range(7)) for p in itertools.permutations(range(7)))
    assert abs(cost[np.arange(7), col].sum() - best) < 1e-12


def test_scores_against_sklearn_where_it_imports():
    from facl_amd import cluster as fcl
    rng = np.random.RandomState(11)
    pred, true = rng.randint(0, 7, size=300), rng.randint(0, 5, size=300)
    t = fcl.contingency(pred, true)
    assert t.sum() == 300 and (t.sum(axis=1) == np.bincount(pred)).all() and (t.sum(axis=0) == np.bincount(true)).all()
    # symmetric in the two labellings, invariant under relabelling
    assert abs(fcl.nmi(t) - fcl.nmi(t.T)) < 1e-12 and abs(fcl.ari(t) - fcl.ari(t.T)) < 1e-12
    assert 0.0 <= fcl.nmi(t) < 0.2 and abs(fcl.ari(t)) < 0.05                  # independent labellings
    try:
        from sklearn.metrics import adjusted_rand_score, normalized_mutual_info_score
    except ImportError:
        return
    assert abs(fcl.nmi(t) - normalized_mutual_info_score(true, pred)) < 1e-10
    assert abs(fcl.ari(t) - adjusted_rand_score(true, pred)) < 1e-10


def test_no_scipy_or_sklearn_in_the_package():
    for dirpath, _, files in os.walk(os.path.join(ROOT, "facl_amd")):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+(scipy|sklearn)\b", src, flags=re.M), f


# ---- flags ------------------------------------------------------------------------------------------------------------------------
CLUSTER = ["--loss_mask", "class", "--synthetic", "0", "--class_ids", "cluster", "--clusters", "3", "--cluster_every", "1"]


def _without(args, flag):
    i = args.index(flag)
    return args[:i] + args[i + 2:]


def test_cluster_id_flags_default_off_and_refusals():
    from facl_amd.train_common import build_parser, check_class_mask_flags
    p = build_parser('0')
    d = p.parse_args([])
    assert (d.class_ids, d.clusters, d.cluster_every, d.cluster_iters, d.cluster_restarts, d.cluster_seed) == ("labels", 0, 0, 50, 1, 0)
    check_class_mask_flags(d, world=4)                                          # off: nothing to refuse
    check_class_mask_flags(p.parse_args(CLUSTER), world=1)
    check_class_mask_flags(p.parse_args(CLUSTER + ["--class_positives", "0.5", "--neg_queue", "8", "--batchSize", "4"]), world=1)
    refusals = [
        (_without(CLUSTER, "--loss_mask"), 1, "--class_ids cluster supplies the ids of --loss_mask class"),
        (_without(CLUSTER, "--loss_mask") + ["--loss_mask", "exclude"], 1, "got --loss_mask exclude"),
        (_without(CLUSTER, "--synthetic") + ["--synthetic", "1"], 1, "--class_ids cluster extracts and clusters the train split"),
        (_without(CLUSTER, "--synthetic") + ["--synthetic", "2"], 1, "it needs --synthetic 0"),
        (CLUSTER, 2, "--class_ids cluster runs on one rank only \\(got 2 ranks\\)"),
        (_without(CLUSTER, "--clusters"), 1, "--clusters K in 2..1024 \\(got 0\\)"),
        (_without(CLUSTER, "--clusters") + ["--clusters", "1"], 1, "--clusters K in 2..1024 \\(got 1\\)"),
        (_without(CLUSTER, "--clusters") + ["--clusters", "1025"], 1, "--clusters K in 2..1024 \\(got 1025\\)"),
        (_without(CLUSTER, "--cluster_every"), 1, "--cluster_every E >= 1 \\(got 0\\)"),
        (CLUSTER + ["--cluster_iters", "0"], 1, "--cluster_iters and --cluster_restarts must be >= 1"),
        (CLUSTER + ["--cluster_restarts", "0"], 1, "--cluster_iters and --cluster_restarts must be >= 1"),
        (CLUSTER + ["--label_fraction", "0.5"], 1, "--class_ids cluster reads no label"),
        (CLUSTER + ["--label_seed", "3"], 1, "--class_ids cluster reads no label"),
        (CLUSTER + ["--save_state_every", "1"], 1, "--save_state_every / --resume"),
        (CLUSTER + ["--resume", "auto"], 1, "--save_state_every / --resume"),
    ]
    for args, world, msg in refusals:
        with pytest.raises(RuntimeError, match=msg):
            check_class_mask_flags(p.parse_args(args), world=world)


def test_label_id_refusals_keep_their_messages():
    from facl_amd.train_common import build_parser, check_class_mask_flags
    p = build_parser('0')
    with pytest.raises(RuntimeError, match="--loss_mask class runs on one rank only \\(got 2 ranks\\): gathered class ids are not implemented"):
        check_class_mask_flags(p.parse_args(["--loss_mask", "class", "--synthetic", "0"]), world=2)
    with pytest.raises(RuntimeError, match="--loss_mask class masks the keys of clips with the anchor's action label: it needs --synthetic 0"):
        check_class_mask_flags(p.parse_args(["--loss_mask", "class", "--synthetic", "1"]), world=1)
    with pytest.raises(RuntimeError, match="--label_fraction must be in \\(0, 1\\] \\(got 0.0\\)"):
        check_class_mask_flags(p.parse_args(["--loss_mask", "class", "--synthetic", "0", "--label_fraction", "0"]), world=1)
    with pytest.raises(RuntimeError, match="--class_positives"):
        check_class_mask_flags(p.parse_args(["--loss_mask", "exclude", "--class_positives", "1"]), world=1)


def test_entries_refuse_before_the_device(tmp_path, monkeypatch):
    """The training entry raises on the flags before it creates its output folder; fine-tuning refuses the flag outright."""
    from facl_amd import cn3d_train_motion_GL as train
    from facl_amd.finetune import check_finetune_flags, finetune_parser
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(RuntimeError, match="--clusters K in 2..1024"):
        train.main(_without(CLUSTER, "--clusters") + ["--save_root_dir", str(tmp_path / "ck")])
    assert not os.path.exists(str(tmp_path / "ck"))
    with pytest.raises(RuntimeError, match="--class_ids supplies the class ids of the contrastive loss's mask"):
        check_finetune_flags(finetune_parser().parse_args(["--class_ids", "cluster"]), world=1)


def test_cluster_eval_parser():
    from facl_amd import cluster_eval
    o = cluster_eval.build_parser().parse_args(["--motion_feature_dir", "m"])
    assert (o.subset, o.clusters, o.iters, o.restarts, o.seed, o.columns, o.appearance_feature_dir) == ("test", 0, 50, 3, 0, "all", None)
    with pytest.raises(SystemExit):
        cluster_eval.build_parser().parse_args(["--motion_feature_dir", "m", "--columns", "views"])


# ---- header, bindings, refusals of the entries ------------------------------------------------------------------------------------
def test_header_declares_and_lib_binds_the_entries():
    from facl_amd import _lib
    txt = open(os.path.join(ROOT, "include", "facl_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name, nargs in (("facl_cluster_ws_bytes", 3), ("facl_cluster_row_inv", 6), ("facl_cluster_sums", 12)):
        m = re.search(r"(?:int|int64_t)\s+%s\s*\(([^)]*)\)" % name, txt)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name]), name
    assert "facl_cluster_ws_bytes" in _lib.RESTYPE_I64


E_SHAPE, E_NULL, E_ALIGN = -1, -2, -3


def test_entries_refuse_bad_arguments_before_any_launch():
    """Host buffers stand in for device memory: every call below is refused by the argument checks, which come before the
    first launch, so nothing is ever read through these pointers."""
    from facl_amd import _lib, build
    build.build()
    lib = _lib.load_library()
    raw = (ctypes.c_char * 4096)()
    base = (ctypes.addressof(raw) + 63) & ~63                                   # 64-byte aligned
    x, inv, order, offs, cent, err, ws = (base + 256 * i for i in range(7))
    sums = lambda **kw: lib.facl_cluster_sums(*[{**dict(x=x, n=8, ldx=64, C=64, inv=inv, order=order, offs=offs, K=2, cent=cent,
                                                        err=err, ws=ws, stream=None), **kw}[k]
                                                for k in ("x", "n", "ldx", "C", "inv", "order", "offs", "K", "cent", "err", "ws", "stream")])
    rinv = lambda **kw: lib.facl_cluster_row_inv(*[{**dict(x=x, n=8, ldx=64, C=64, inv=inv, stream=None), **kw}[k]
                                                   for k in ("x", "n", "ldx", "C", "inv", "stream")])
    shape_cases = [dict(n=0), dict(n=-3), dict(C=0), dict(C=32), dict(C=96, ldx=96), dict(ldx=60), dict(ldx=66, C=64), dict(ldx=32)]
    for kw in shape_cases:
        assert sums(**kw) == E_SHAPE, kw
        assert rinv(**kw) == E_SHAPE, kw
    for K in (0, -1, 1025):
        assert sums(K=K) == E_SHAPE, K
    for name in ("x", "inv", "order", "offs", "cent", "err", "ws"):
        assert sums(**{name: None}) == E_NULL, name
    for name in ("x", "inv"):
        assert rinv(**{name: None}) == E_NULL, name
    for name in ("x", "cent", "ws"):
        assert sums(**{name: locals()[name] + 4}) == E_ALIGN, name
    assert rinv(x=x + 8) == E_ALIGN
    # precedence: shape, then NULL, then alignment
    assert sums(n=0, x=None) == E_SHAPE and sums(x=None, cent=cent + 4) == E_NULL
    assert rinv(C=32, x=None) == E_SHAPE and rinv(inv=None, x=x + 4) == E_NULL
    # the workspace size: offsets rounded up to 256 bytes + 8 C (n / 128 + K) bytes of partial sums
    assert lib.facl_cluster_ws_bytes(37920, 60, 5632) == 256 + 8 * 5632 * (37920 // 128 + 60)
    assert lib.facl_cluster_ws_bytes(1, 1, 64) == 256 + 8 * 64
    assert lib.facl_cluster_ws_bytes(8, 1024, 64) == 4352 + 8 * 64 * 1024
    for bad in ((0, 1, 64), (1, 0, 64), (1, 1025, 64), (1, 1, 32), (1, 1, 100)):
        assert lib.facl_cluster_ws_bytes(*bad) == E_SHAPE, bad


def test_wrappers_refuse_cpu_tensors():
    import torch
    from facl_amd import cluster as fcl
    with pytest.raises(RuntimeError, match="GPU only"):
        fcl.kmeans(torch.zeros(8, 64), 2)
    with pytest.raises(RuntimeError, match="GPU only"):
        fcl.row_inv(torch.zeros(8, 64))
