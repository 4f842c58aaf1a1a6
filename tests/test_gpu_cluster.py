"""Spherical k-means on the device (csrc/cluster.hip, facl_amd/cluster.py), the clustering entry and --class_ids cluster of the
training entries.  References are fp64 NumPy restatements of the algorithm as facl_amd.cluster.kmeans documents it."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from poison import poisoned_scratch  # noqa: F401
from synth_tree import epoch_loss_text, run_train_entry, train_argv, write_tree

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS24 = 2.0 ** -24
GAP = 2e-6                                                   # REL_TOL of tests/test_gpu_knn.py x the largest |cosine| = 1


def _dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def _ulp32(v):
    return np.spacing(np.abs(v).astype(np.float32)).astype(np.float64)


# ---- 1: the row pass --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,C,ld", [(1, 64, 64), (77, 192, 192), (130, 512, 5632)])
def test_row_inv_vs_fp64(n, C, ld):
    from facl_amd import cluster as fcl
    rng = np.random.RandomState(n)
    full = (rng.randn(n, ld) * np.exp(rng.uniform(-8, 8, size=(n, 1)))).astype(np.float32)
    if n > 2:
        full[1, ld - C:] = 0.0                               # a row of zeros (inside the slice)
    x = _dev(full)[:, ld - C:]                               # the LAST C columns: a strided view, read in place
    assert x.stride(0) == ld
    inv = fcl.row_inv(x).cpu().numpy()
    want = 1.0 / np.maximum(np.sqrt((full[:, ld - C:].astype(np.float64) ** 2).sum(axis=1)), 1e-12)
    ulps = np.abs(inv.astype(np.float64) - want) / _ulp32(want)
    print("row_inv n=%d C=%d: worst %.3f ulp" % (n, C, ulps.max()))
    assert inv.dtype == np.float32 and ulps.max() <= 2.0     # DESIGN 3.13's bound for the same row body
    if n > 2:
        assert inv[1] == np.float32(1e12)


# ---- 2: the sums ------------------------------------------------------------------------------------------------------------------
def _labels_for(case, n, K, rng):
    if case == "skewed":                                     # 700 of 777 rows in cluster 0, cluster 3 empty
        lab = np.zeros(n, dtype=np.int64)
        lab[700:] = rng.choice([1, 2, 4], size=n - 700)
        return lab[rng.permutation(n)]
    return rng.randint(0, K, size=n)


def _order_offs(lab, K):
    order = np.argsort(lab, kind="stable").astype(np.int32)
    offs = np.concatenate([[0], np.cumsum(np.bincount(lab, minlength=K))]).astype(np.int32)
    return order, offs


SUM_CASES = [("one", 1, 64, 64, 1), ("skewed", 777, 64, 64, 5), ("wide", 300, 5632, 5632, 60), ("slice", 300, 512, 5632, 60)]
MARK = lambda K, C: (-123.0 + 0.25 * np.arange(K * C, dtype=np.float32).reshape(K, C) % 17.0).astype(np.float32)


def _sums_setup(case, n, C, ld, K):
    from facl_amd import cluster as fcl
    rng = np.random.RandomState(n + C + K)
    full = (rng.randn(n, ld) * np.exp(rng.uniform(-3, 3, size=(n, 1)))).astype(np.float32)
    x = _dev(full)[:, ld - C:]
    xs = full[:, ld - C:].astype(np.float64)
    lab = _labels_for(case, n, K, rng)
    inv = fcl.row_inv(x)
    return x, xs, lab, inv


def _sums_ref(xs, inv64, order, offs, K, keep):
    """fp64 sums of double(x) * double(inv) and the bound's sum of magnitudes; clusters without rows keep `keep`."""
    want, mag = keep.astype(np.float64).copy(), np.zeros_like(keep, dtype=np.float64)
    for c in range(K):
        rows = [int(i) for i in order[offs[c]:offs[c + 1]] if 0 <= i < xs.shape[0]]
        if offs[c + 1] > offs[c]:
            want[c] = (xs[rows] * inv64[rows, None]).sum(axis=0)
            mag[c] = (np.abs(xs[rows]) * inv64[rows, None]).sum(axis=0)
    return want, mag


@pytest.mark.parametrize("case,n,C,ld,K", SUM_CASES)
def test_cluster_sums_vs_fp64(case, n, C, ld, K):
    from facl_amd import cluster as fcl
    x, xs, lab, inv = _sums_setup(case, n, C, ld, K)
    order, offs = _order_offs(lab, K)
    d_order, d_offs = fcl.label_order(_dev(lab), K)
    assert d_order.cpu().numpy().tolist() == order.tolist() and d_offs.cpu().numpy().tolist() == offs.tolist()
    cent = _dev(MARK(K, C))
    assert fcl.cluster_sums(x, inv, d_order, d_offs, cent) is cent
    got = cent.cpu().numpy()
    # each term carries the fp32 rounding of inv_i, the result one final rounding; fp64 accumulation is below both
    inv64 = 1.0 / np.maximum(np.sqrt((xs ** 2).sum(axis=1)), 1e-12)
    want, mag = _sums_ref(xs, inv64, order, offs, K, MARK(K, C))
    live = np.repeat((offs[1:] > offs[:-1])[:, None], C, axis=1)
    ratio = np.abs(got.astype(np.float64) - want)[live] / (3.0 * EPS24 * mag[live])
    print("cluster_sums %s: worst |error| / bound = %.4f" % (case, ratio.max()))
    assert ratio.max() <= 1.0
    # against the inv the entry was given, only the final rounding (and fp64 accumulation) remains
    want_g, mag_g = _sums_ref(xs, inv.cpu().numpy().astype(np.float64), order, offs, K, MARK(K, C))
    assert (np.abs(got.astype(np.float64) - want_g)[live] <= EPS24 * np.abs(want_g)[live] + 1e-12 * mag_g[live]).all()
    # clusters without rows come back bit-identical
    empty = np.flatnonzero(offs[1:] == offs[:-1])
    if case == "skewed":
        assert empty.tolist() == [3] and offs[1] == 700
    assert (got[empty].view(np.int32) == MARK(K, C)[empty].view(np.int32)).all()
    # the same bits again
    again = _dev(MARK(K, C))
    fcl.cluster_sums(x, inv, d_order, d_offs, again)
    assert torch.equal(again.view(torch.int32), cent.view(torch.int32))


def test_cluster_sums_skips_indices_out_of_range():
    """The guard: an entry of `order` outside [0, n) is never dereferenced -- the row is skipped, the wrapper raises, and every
    other row is summed as before."""
    from facl_amd import cluster as fcl
    case, n, C, ld, K = SUM_CASES[1]
    x, xs, lab, inv = _sums_setup(case, n, C, ld, K)
    order, offs = _order_offs(lab, K)
    bad = order.copy()
    bad[5], bad[offs[2]] = -1, n                             # one in cluster 0 (first segment), one at the start of cluster 2
    cent = _dev(MARK(K, C))
    with pytest.raises(RuntimeError, match="outside \\[0, n\\)"):
        fcl.cluster_sums(x, inv, _dev(bad), _dev(offs), cent)
    got = cent.cpu().numpy()
    want, mag = _sums_ref(xs, inv.cpu().numpy().astype(np.float64), bad, offs, K, MARK(K, C))      # without the two rows
    for c in (0, 1, 2, 4):
        assert (np.abs(got[c].astype(np.float64) - want[c]) <= EPS24 * np.abs(want[c]) + 1e-12 * mag[c]).all(), c
    assert (got[3].view(np.int32) == MARK(K, C)[3].view(np.int32)).all()
    # boundaries that are no partition of the rows: nothing is read, nothing is written
    for wrong in (offs[::-1].copy(), offs + 1, np.where(np.arange(K + 1) == K, n + 5, offs).astype(np.int32)):
        cent = _dev(MARK(K, C))
        with pytest.raises(RuntimeError, match="offs is not"):
            fcl.cluster_sums(x, inv, _dev(order), _dev(wrong.astype(np.int32)), cent)
        assert (cent.cpu().numpy().view(np.int32) == MARK(K, C).view(np.int32)).all()


# ---- 3: the algorithm, restated in fp64 -------------------------------------------------------------------------------------------
def _assign64(xn, cent):
    cn = cent / np.maximum(np.sqrt((cent ** 2).sum(axis=1, keepdims=True)), 1e-12)
    sim = xn @ cn.T
    top = np.sort(sim, axis=1)
    gap = top[:, -1] - top[:, -2] if sim.shape[1] > 1 else np.full(sim.shape[0], np.inf)
    return np.argmax(sim, axis=1), gap


def _update64(xn, lab, cent):
    new = cent.copy()
    for c in range(cent.shape[0]):
        if (lab == c).any():
            new[c] = xn[lab == c].sum(axis=0)
    return new


@pytest.mark.parametrize("n,C,K", [(600, 64, 6), (512, 512, 60)])
def test_one_lloyd_step_vs_fp64(n, C, K):
    from facl_amd import cluster as fcl
    rng = np.random.RandomState(C + K)
    xh = rng.randn(n, C).astype(np.float32)
    idx = rng.choice(n, K, replace=False)
    xs = xh.astype(np.float64)
    xn = xs / np.maximum(np.sqrt((xs ** 2).sum(axis=1, keepdims=True)), 1e-12)
    lab0, gap0 = _assign64(xn, xs[idx])
    cent1 = _update64(xn, lab0, xs[idx])
    lab1, gap1 = _assign64(xn, cent1)
    # on the reference alone, before the device is used: the first assignment has no near tie at all (a row that changed
    # sides there would move a centroid), and at most 1 % of the rows are exempt from the second
    assert gap0.min() > GAP
    exempt = gap1 <= GAP
    assert exempt.mean() <= 0.01
    labels, cent, info = fcl.kmeans(_dev(xh), K, iters=1, init=idx)
    got = labels.cpu().numpy()
    assert labels.dtype == torch.int32 and got.shape == (n,) and tuple(cent.shape) == (K, C) and cent.dtype == torch.float32
    assert (got[~exempt] == lab1[~exempt]).all()
    assert info["n_iter"] == 1 and len(info["history"]) == 2 and info["restart"] == 0
    if (lab0 != lab1)[~exempt].any():
        assert not info["converged"]
    # the centroids returned are the ones that produced the labels: the sums under the first assignment
    c64 = cent.cpu().numpy().astype(np.float64)
    assert np.abs(c64 - cent1).max() <= 3.0 * EPS24 * np.abs(xn).sum(axis=0).max()
    mean1 = np.take_along_axis(xn @ (cent1 / np.sqrt((cent1 ** 2).sum(axis=1, keepdims=True))).T, lab1[:, None], 1).mean()
    assert abs(info["objective"] - mean1) <= GAP
    assert info["sizes"].tolist() == np.bincount(got, minlength=K).tolist()


def test_trajectory_properties():
    from facl_amd import cluster as fcl
    from facl_amd.knn_eval import knn_topk
    n, C, K = 1000, 64, 8
    x = _dev(np.random.RandomState(3).randn(n, C).astype(np.float32))
    labels, cent, info = fcl.kmeans(x, K, iters=50, restarts=3, seed=4)
    h = np.asarray(info["history"])
    assert len(h) == info["n_iter"] + 1 and (np.diff(h) >= -GAP).all() and info["objective"] == h[-1]
    got = labels.cpu().numpy()
    assert got.min() >= 0 and got.max() < K and info["sizes"].sum() == n
    assert info["sizes"].tolist() == np.bincount(got, minlength=K).tolist() and 0 <= info["empty"] <= K
    if info["converged"]:                                    # one more assignment changes no label
        assert torch.equal(knn_topk(x, cent, 1)[1][:, 0], labels)
    else:
        assert info["n_iter"] == 50
    singles = [fcl.kmeans(x, K, iters=50, restarts=1, seed=4 + r) for r in range(3)]
    objs = [s[2]["objective"] for s in singles]
    assert info["restart"] == int(np.argmax(objs)) and info["objective"] == max(objs)          # equal: the lower r (argmax's first)
    assert torch.equal(singles[info["restart"]][0], labels)
    labels2, cent2, info2 = fcl.kmeans(x, K, iters=50, restarts=3, seed=4)
    assert torch.equal(labels2, labels) and torch.equal(cent2.view(torch.int32), cent.view(torch.int32))
    assert info2["history"] == info["history"] and info2["restart"] == info["restart"]
    with pytest.raises(ValueError, match="n >= K"):
        fcl.kmeans(x[:5], K)


def test_planted_partition_ignores_row_length():
    from facl_amd import cluster as fcl
    rng = np.random.RandomState(8)
    K, C, per = 8, 64, 125
    dirs = np.linalg.qr(rng.randn(C, C))[0][:K]              # K orthogonal unit directions
    ids = np.repeat(np.arange(K), per)
    rows = dirs[ids] + 0.05 * rng.randn(K * per, C)
    rows *= 10.0 ** rng.uniform(-3, 3, size=(K * per, 1))    # positive row scales over six decades
    perm = rng.permutation(K * per)
    rows, ids = rows[perm].astype(np.float32), ids[perm]
    init = [int(np.flatnonzero(ids == c)[0]) for c in range(K)]
    labels, _, info = fcl.kmeans(_dev(rows), K, iters=50, init=init)
    assert info["converged"] and info["n_iter"] <= 3 and info["empty"] == 0
    t = fcl.contingency(labels.cpu().numpy(), ids)
    assert fcl.ari(t) == 1.0 and fcl.matched_accuracy(t) == 100.0
    assert info["sizes"].tolist() == [per] * K


# ---- 4: the clustering entry ------------------------------------------------------------------------------------------------------
def _feature_tree(root, n=24, width=11 * 512):
    """The probe's layout: the clip list under reslution/Resolution60/raw (cameras 2 / 3 train: 16, camera 1 test: 8, four
    actions) and two folders of <v_name>.npy vectors, every 512-chunk = the action's direction + noise."""
    rng = np.random.RandomState(21)
    names = ["S%03dC%03dP%03dR001A%03d" % (1 + i % 4, (2, 3, 1)[i % 3], 1 + i, 1 + (i // 3) % 4) for i in range(n)]
    lst = os.path.join(str(root), "reslution", "Resolution60", "raw")
    os.makedirs(lst, exist_ok=True)
    dirs = np.linalg.qr(rng.randn(512, 512))[0][:8]
    for stream, folder in enumerate(("motion", "appearance")):
        os.makedirs(os.path.join(str(root), folder), exist_ok=True)
        for i, nm in enumerate(names):
            a = (i // 3) % 4
            v = np.tile(dirs[a + 4 * stream], width // 512) + 0.02 * rng.randn(width)
            np.save(os.path.join(str(root), folder, nm + ".npy"), v.astype(np.float32))
    for nm in names:
        np.save(os.path.join(lst, nm + ".npy"), np.zeros((1, 8)))
    return names


def _seed_of_a_spread_draw(root, test):
    """The smallest seed whose first restart draws one initial row per action of the split (host arithmetic on the clip list
    alone): from there the planted actions are found whatever the later restarts do, so 100 % is what the entry must print."""
    from facl_amd.dataset import PROBE_LIST_DIR, ClipIndex
    index = ClipIndex.from_dir(os.path.join(str(root), PROBE_LIST_DIR), "ntu120")
    y = np.asarray([index.label(v) for v in index.select("view", test=test)])
    K = len(np.unique(y))
    for seed in range(1000):
        if len(np.unique(y[np.random.RandomState(seed).choice(len(y), K, replace=False)])) == K:
            return str(seed)
    raise AssertionError("no seed below 1000 draws one row per action")


def test_cluster_eval_entry(tmp_path, capsys):
    from facl_amd import cluster_eval
    _feature_tree(tmp_path)
    base = ["--data_root", str(tmp_path), "--dataset", "ntu120", "--motion_feature_dir", str(tmp_path / "motion")]
    both = base + ["--appearance_feature_dir", str(tmp_path / "appearance")]
    seed_test, seed_train = _seed_of_a_spread_draw(tmp_path, True), _seed_of_a_spread_draw(tmp_path, False)
    capsys.readouterr()
    res = cluster_eval.main(both + ["--seed", seed_test])    # the default three restarts
    out = capsys.readouterr().out
    assert "cluster acc: 100.0" in out and "nmi: " in out and "ari: " in out and "purity: 100.0" in out
    assert re.search(r"objective: \S+ iters: \d+ restart: \d+ sizes min/max: 2/2", out)
    assert res["acc"] == 100.0 and abs(res["nmi"] - 1.0) < 1e-12 and res["ari"] == 1.0 and res["sizes"].tolist() == [2, 2, 2, 2]
    res = cluster_eval.main(both + ["--seed", seed_train, "--columns", "global", "--subset", "train"])
    assert res["acc"] == 100.0 and res["sizes"].tolist() == [4, 4, 4, 4]
    res = cluster_eval.main(base + ["--seed", seed_test, "--columns", "global"])               # one stream: the slice is read in place
    assert res["acc"] == 100.0
    res = cluster_eval.main(base + ["--clusters", "2", "--restarts", "1"])
    assert res["sizes"].sum() == 8 and 0.0 < res["acc"] <= 100.0 and "cluster acc: " in capsys.readouterr().out


# ---- 5: --class_ids cluster of the training entry ---------------------------------------------------------------------------------
CLUSTER = ("--loss_mask", "class", "--class_ids", "cluster", "--clusters", "3", "--cluster_every", "1")


def _run_entry(root, folder, *extra):
    mode = ("--loss_normalize", "1", "--loss_temperature", "0.1", "--neg_queue", "8", "--nepoch", "2")
    return run_train_entry(train_argv(root, folder, *extra, before_save=mode, features_first=True))


def test_train_entry_with_cluster_ids(tmp_path):
    root = tmp_path / "d"
    write_tree(str(root))
    sd_a, out_a = _run_entry(root, tmp_path / "a", *CLUSTER)
    lines = re.findall(r"epoch: (\d+) clusters: 3 objective: (\S+) iters: (\d+) sizes min/median/max: (\d+)/(\S+)/(\d+) \| acc: (\S+) nmi: (\S+)",
                       out_a)
    assert [l[0] for l in lines] == ["0", "1"], out_a
    for l in lines:                                          # K = 3: min, median and max are the three sizes
        assert int(l[3]) + float(l[4]) + int(l[5]) == 16 and np.isfinite(float(l[1])) and 0 <= int(l[2]) <= 50
        assert 0.0 <= float(l[6]) <= 100.0 and 0.0 <= float(l[7]) <= 1.0 + 1e-9
    assert "class mask: cluster ids, 3 clusters" in out_a and "labelled" not in out_a
    # epoch 0: every id is unknown, the class mask is the exclude mask bit for bit
    sd_x, out_x = _run_entry(root, tmp_path / "x", "--loss_mask", "exclude")
    assert "clusters:" not in out_x
    assert epoch_loss_text(out_a, 0) == epoch_loss_text(out_x, 0)
    # epoch 1: sixteen clips in three clusters put two cluster-mates into every batch of four, so the mask acts
    assert sd_a.keys() == sd_x.keys()
    assert any(not torch.equal(sd_a[k], sd_x[k]) for k in sd_a)
    # two identical runs give bit-identical weights and checkpoints
    sd_b, out_b = _run_entry(root, tmp_path / "b", *CLUSTER)
    assert [epoch_loss_text(out_b, e) for e in (0, 1)] == [epoch_loss_text(out_a, e) for e in (0, 1)]
    assert re.findall(r"clusters: .*", out_b) == re.findall(r"clusters: .*", out_a)
    for k in sd_a:
        assert torch.equal(sd_a[k], sd_b[k]), k
    names = sorted(n for n in os.listdir(str(tmp_path / "a")) if n.endswith(".pth"))
    assert names and names == sorted(n for n in os.listdir(str(tmp_path / "b")) if n.endswith(".pth"))
    for nm in names:
        fa = torch.load(os.path.join(str(tmp_path / "a"), nm), map_location="cpu", weights_only=True)
        fb = torch.load(os.path.join(str(tmp_path / "b"), nm), map_location="cpu", weights_only=True)
        assert fa.keys() == fb.keys() and all(torch.equal(fa[k], fb[k]) for k in fa), nm


def test_recluster_resets_the_queue_ids_only():
    from facl_amd.neg_queue import NegativeQueue
    from facl_amd.train_common import recluster
    rng = np.random.RandomState(2)
    queue = NegativeQueue(8, 64, 4, DEV, with_ids=True)
    for p in range(3):                                       # three pushes: the ring has wrapped, every slot holds an id
        queue.push(_dev(rng.randn(4, 64).astype(np.float32)), _dev(np.arange(4) % 3, dtype=torch.int32))
    assert (queue.ids >= 0).all() and queue.head_valid() == (4, 8)
    buf, state = queue.buf.clone(), queue.state.clone()
    names = ["clip%02d" % i for i in range(40)]
    class_of = {n: 7 for n in names + ["not_extracted"]}
    feats = _dev(rng.randn(40, 11 * 512).astype(np.float32))
    ids, info = recluster(SimpleNamespace(queue=queue), class_of, feats, names, 3, iters=5, restarts=1, seed=1)
    assert queue.ids.tolist() == [-1] * 8
    assert torch.equal(queue.buf, buf) and torch.equal(queue.state, state)
    assert [class_of[n] for n in names] == ids.tolist() and set(ids.tolist()) <= {0, 1, 2} and class_of["not_extracted"] == -1
    assert info["sizes"].sum() == 40
    recluster(SimpleNamespace(queue=None), class_of, feats, names, 3, iters=1)                 # a step without a queue yet
