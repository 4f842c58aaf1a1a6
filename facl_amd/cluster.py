"""Spherical k-means of frozen features on the device, and the label-free clustering scores.  The reference has no
counterpart: clustering accuracy / NMI / ARI / purity are the standard label-free complement of its linear probe
(linear_classify/linercls.py), and the cluster ids stand in for action labels in the class-aware loss modes (--class_ids cluster).

A Lloyd iteration is two passes over the (n, C) features: the assignment is ``knn_topk`` with the centroids as the bank and
k = 1 (csrc/knn.hip: the fused cosine GEMM with selection, deterministic, the lower index on equal similarities), the update is
``cluster_sums`` (csrc/cluster.hip: fp64 sums of the unit rows in a fixed order, no floating-point atomic).  The stable order by
label that the update reads comes from ``torch.sort(labels, stable=True)`` and ``bincount`` / ``cumsum``: 4 bytes per row beside
the 4 C of the sums.  The kernels are GPU only: there is no CPU path.  The scores are plain NumPy on the host."""
import numpy as np
import torch

from . import _lib
from .knn_eval import _rows, knn_topk

K_MAX = 1024


# ---- device: the centroid update ------------------------------------------------------------------------------------------------
def row_inv(x):
    """(n,) float32: 1 / max(||x_i||, 1e-12) of every row, the sum of squares in fp64."""
    x = _rows(x, "features")
    n, C = x.shape
    with torch.cuda.device(x.device):
        inv = _lib.empty((n,), dtype=torch.float32, device=x.device)
        _lib.call("facl_cluster_row_inv", x, n, x.stride(0), C, inv, detail="n=%d, C=%d" % (n, C))
    return inv


def label_order(labels, K):
    """(order (n) int32, offs (K+1) int32) of int labels in [0, K): the row indices sorted by label, ascending inside a label,
    and the label boundaries."""
    lab = labels.long()
    order = torch.sort(lab, stable=True)[1].to(torch.int32)
    offs = torch.zeros((K + 1,), dtype=torch.int32, device=labels.device)
    offs[1:] = torch.cumsum(torch.bincount(lab, minlength=K)[:K], 0)
    return order, offs


def cluster_sums(x, inv, order, offs, cent):
    """cent[c] = the sum of x_i * inv_i over the rows order[offs[c] : offs[c+1]], in that order, IN PLACE; a cluster without rows
    keeps its row of `cent` (K, C).  Raises when `order` or `offs` are not a sorted labelling of the n rows: an index outside
    [0, n) is skipped by the kernel, never read."""
    x = _rows(x, "features")
    _lib.require_cuda(inv, order, offs, cent)
    n, C = x.shape
    K = cent.shape[0]
    if cent.dtype != torch.float32 or cent.dim() != 2 or cent.shape[1] != C or not cent.is_contiguous():
        raise ValueError("centroids must be a contiguous float32 (K, %d) matrix (got %s %s)" % (C, cent.dtype, tuple(cent.shape)))
    if inv.dtype != torch.float32 or tuple(inv.shape) != (n,) or not inv.is_contiguous():
        raise ValueError("inv must be contiguous float32 (%d,) (got %s %s)" % (n, inv.dtype, tuple(inv.shape)))
    for t, m, what in ((order, n, "order"), (offs, K + 1, "offs")):
        if t.dtype != torch.int32 or tuple(t.shape) != (m,) or not t.is_contiguous():
            raise ValueError("%s must be contiguous int32 (%d,) (got %s %s)" % (what, m, t.dtype, tuple(t.shape)))
    dev = x.device
    with torch.cuda.device(dev):
        nbytes = _lib.call_size("facl_cluster_ws_bytes", n, K, C, detail="n=%d, K=%d, C=%d" % (n, K, C))
        ws = _lib.empty(((nbytes + 7) // 8,), dtype=torch.float64, device=dev)
        err = torch.zeros((1,), dtype=torch.int32, device=dev)
        _lib.call("facl_cluster_sums", x, n, x.stride(0), C, inv, order, offs, K, cent, err, ws,
                  detail="n=%d, C=%d, K=%d" % (n, C, K))
        e = int(err.item())
    if e:
        raise RuntimeError("facl_cluster_sums: %s (err %d)" % (" and ".join(
            m for b, m in ((1, "an entry of order lies outside [0, n): the row was skipped"),
                           (2, "offs is not 0 = offs[0] <= ... <= offs[K] = n: nothing was summed")) if e & b), e))
    return cent


# ---- device: Lloyd iterations ---------------------------------------------------------------------------------------------------
def _lloyd(x, inv, idx, K, iters):
    dev = x.device
    cent = x[torch.as_tensor(idx, dtype=torch.long, device=dev)].contiguous()
    prev, history, updates, converged = None, [], 0, False
    ever_empty = torch.zeros((K,), dtype=torch.bool, device=dev)
    while True:
        val, ix = knn_topk(x, cent, 1)
        labels = ix[:, 0].contiguous()
        history.append(float(val.double().mean().item()))
        if prev is not None and torch.equal(labels, prev):
            converged = True
            break
        if updates >= iters:
            break
        order, offs = label_order(labels, K)
        ever_empty |= offs[1:] == offs[:-1]
        cluster_sums(x, inv, order, offs, cent)
        updates += 1
        prev = labels
    sizes = torch.bincount(labels.long(), minlength=K)[:K]
    ever_empty |= sizes == 0
    info = dict(objective=history[-1], history=history, n_iter=updates, converged=converged,
                sizes=sizes.cpu().numpy().astype(np.int64), empty=int(ever_empty.sum().item()))
    return labels, cent, info


def kmeans(features, K, iters=50, restarts=1, seed=0, init=None):
    """Deterministic spherical k-means of (n, C) float32 CUDA rows (C a multiple of 64; a column slice is clustered in place).
    Returns (labels int32 (n), centroids float32 (K, C), info).

    Restart r starts from the rows np.random.RandomState(seed + r).choice(n, K, replace=False); `init`, K row indices, replaces
    the draw and implies one restart.  Iteration t: labels_t = argmax cosine against the current centroids, objective_t = the
    mean of those cosines; t > 0 and labels_t == labels_{t-1}: converged, stop; otherwise, while fewer than `iters` updates
    were made, centroids = the sums of the unit rows under labels_t (a cluster without rows keeps its centroid) and go on.
    The result is the restart of largest final objective (equal: the lower r), with the centroids that produced the labels.
    info: objective, history (per iteration), n_iter (updates made), converged, restart, sizes (K,), empty (clusters that
    were ever without rows).  The centroids are un-normalised sums; only their direction matters."""
    x = _rows(features, "features")
    n, C = x.shape
    K, iters, restarts = int(K), int(iters), int(restarts)
    if not 1 <= K <= K_MAX:
        raise ValueError("K must be in 1..%d (got %d)" % (K_MAX, K))
    if n < K:
        raise ValueError("k-means of %d rows into %d clusters: it needs n >= K" % (n, K))
    if iters < 0 or restarts < 1:
        raise ValueError("iters must be >= 0 and restarts >= 1 (got %d, %d)" % (iters, restarts))
    if init is not None:
        init = np.asarray(init, dtype=np.int64).reshape(-1)
        if init.shape != (K,) or init.min() < 0 or init.max() >= n:
            raise ValueError("init must hold K = %d row indices in [0, %d)" % (K, n))
        restarts = 1
    inv = row_inv(x)
    best = None
    for r in range(restarts):
        idx = init if init is not None else np.random.RandomState(seed + r).choice(n, K, replace=False)
        labels, cent, info = _lloyd(x, inv, idx, K, iters)
        info["restart"] = r
        if best is None or info["objective"] > best[2]["objective"]:
            best = (labels, cent, info)
    return best


# ---- host: scores of a clustering against labels (plain NumPy) ------------------------------------------------------------------
def contingency(pred, true):
    """(clusters, classes) int64 table of counts; the distinct values of each labelling in ascending order."""
    pred, true = np.asarray(pred).reshape(-1), np.asarray(true).reshape(-1)
    if pred.shape != true.shape:
        raise ValueError("pred and true differ in length (%d, %d)" % (pred.shape[0], true.shape[0]))
    up, ip = np.unique(pred, return_inverse=True)
    ut, it = np.unique(true, return_inverse=True)
    table = np.zeros((len(up), len(ut)), dtype=np.int64)
    np.add.at(table, (ip.reshape(-1), it.reshape(-1)), 1)
    return table


def purity(table):
    """Percent of the rows that carry the majority class of their cluster."""
    table = np.asarray(table, dtype=np.int64)
    return 100.0 * float(table.max(axis=1).sum()) / max(int(table.sum()), 1)


def _entropy(counts, n):
    p = counts[counts > 0].astype(np.float64) / n
    return float(-(p * np.log(p)).sum())


def nmi(table):
    """Normalised mutual information: I(U; V) / ((H(U) + H(V)) / 2), natural logarithm; 1.0 when both partitions are a single
    cluster (0 / 0), as scikit-learn defines it."""
    table = np.asarray(table, dtype=np.int64)
    n = float(table.sum())
    a, b = table.sum(axis=1), table.sum(axis=0)
    if (a > 0).sum() <= 1 and (b > 0).sum() <= 1:
        return 1.0
    i, j = np.nonzero(table)
    nij = table[i, j].astype(np.float64)
    mi = float((nij / n * (np.log(nij) + np.log(n) - np.log(a[i].astype(np.float64)) - np.log(b[j].astype(np.float64)))).sum())
    mi = max(mi, 0.0)
    norm = 0.5 * (_entropy(a, n) + _entropy(b, n))
    return mi / norm if norm > 0 else 0.0


def ari(table):
    """Adjusted Rand index (Hubert & Arabie); 1.0 when the expected and the maximal index coincide (both partitions trivial)."""
    table = np.asarray(table, dtype=np.int64)
    pairs = lambda v: float((v.astype(np.float64) * (v.astype(np.float64) - 1.0) / 2.0).sum())
    n = float(table.sum())
    s, sa, sb = pairs(table), pairs(table.sum(axis=1)), pairs(table.sum(axis=0))
    total = n * (n - 1.0) / 2.0
    expected = sa * sb / total if total > 0 else 0.0
    mx = 0.5 * (sa + sb)
    return 1.0 if mx == expected else (s - expected) / (mx - expected)


def assign_min(cost):
    """Row -> column of a minimum-cost one-to-one assignment of a square cost matrix (the Hungarian method with potentials,
    shortest augmenting paths; O(n^3), the inner loop vectorised)."""
    cost = np.asarray(cost, dtype=np.float64)
    n = cost.shape[0]
    if cost.ndim != 2 or cost.shape[1] != n:
        raise ValueError("assign_min takes a square matrix (got %s)" % (cost.shape,))
    u, v = np.zeros(n + 1), np.zeros(n + 1)
    p, way = np.zeros(n + 1, dtype=np.int64), np.zeros(n + 1, dtype=np.int64)       # p[j]: the row of column j (1-based, 0: free)
    for i in range(1, n + 1):
        p[0], j0 = i, 0
        minv = np.full(n + 1, np.inf)
        used = np.zeros(n + 1, dtype=bool)
        while True:
            used[j0] = True
            i0 = p[j0]
            free = ~used[1:]
            cur = cost[i0 - 1] - u[i0] - v[1:]
            upd = free & (cur < minv[1:])
            minv[1:][upd] = cur[upd]
            way[1:][upd] = j0
            masked = np.where(free, minv[1:], np.inf)
            j1 = int(np.argmin(masked)) + 1
            delta = masked[j1 - 1]
            u[p[used]] += delta                                                         # distinct rows: p is one-to-one on `used`
            v[used] -= delta
            minv[1:][free] -= delta
            j0 = j1
            if p[j0] == 0:
                break
        while j0:
            j1 = way[j0]
            p[j0] = p[j1]
            j0 = j1
    out = np.zeros(n, dtype=np.int64)
    out[p[1:] - 1] = np.arange(n)
    return out


def matched_accuracy(table):
    """Percent of the rows that agree under the best one-to-one assignment of clusters to classes (a rectangular table is
    padded with zeros: a surplus cluster or class matches nothing)."""
    table = np.asarray(table, dtype=np.int64)
    m = max(table.shape)
    sq = np.zeros((m, m), dtype=np.int64)
    sq[:table.shape[0], :table.shape[1]] = table
    col = assign_min(sq.max() - sq)
    return 100.0 * float(sq[np.arange(m), col].sum()) / max(int(table.sum()), 1)


def scores(pred, true):
    """dict(acc, nmi, ari, purity) of a clustering against labels; acc and purity in percent."""
    t = contingency(pred, true)
    return dict(acc=matched_accuracy(t), nmi=nmi(t), ari=ari(t), purity=purity(t))
