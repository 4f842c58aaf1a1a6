"""Weighted k-nearest-neighbour evaluation of frozen features: the cheap complement of the linear probe
(``facl_amd.linear_classify``).  Cosine similarity between L2-normalised feature rows, the k nearest rows of a labelled bank,
an exp(s / T)-weighted vote over their labels.  The similarity GEMM and the selection are one fused kernel
(csrc/knn.hip: fp16x3 exact split, running top-k per query in the epilogue), so the (queries, bank) similarity matrix is
never written.  GPU only: there is no CPU path."""
import argparse

import torch

from . import _lib

K_MAX = 64


def _rows(t, what):
    _lib.require_cuda(t)
    if t.dim() != 2 or t.dtype != torch.float32:
        raise ValueError("%s must be a 2-D float32 tensor (got %s %s)" % (what, tuple(t.shape), t.dtype))
    if t.stride(1) != 1 or t.stride(0) % 4 != 0 or t.stride(0) < t.shape[1] or t.data_ptr() % 16 != 0:
        t = t.contiguous()
    return t


def _int32(t, n, what, device):
    if t is None:
        return None
    t = torch.as_tensor(t)
    _lib.require_cuda(t)
    if t.shape != (n,):
        raise ValueError("%s must have shape (%d,) (got %s)" % (what, n, tuple(t.shape)))
    return t.to(device=device, dtype=torch.int32).contiguous()


def knn_topk(queries, bank, k, self_idx=None):
    """(values, indices), each (nq, k): the k bank rows of largest cosine similarity per query row, values non-increasing,
    equal values by lower bank index; the same bits every run.  `self_idx` (nq) int: the bank row a query must not return
    (-1: none) -- leave-one-out of a split against itself.  Features are (n, C) float32 with C a multiple of 64."""
    queries, bank = _rows(queries, "queries"), _rows(bank, "bank")
    if bank.device != queries.device:
        raise ValueError("queries and bank are on different devices")
    nq, C = queries.shape
    nb = bank.shape[0]
    if bank.shape[1] != C:
        raise ValueError("queries are %d wide, the bank %d" % (C, bank.shape[1]))
    k = int(k)
    dev = queries.device
    sidx = _int32(self_idx, nq, "self_idx", dev)
    with torch.cuda.device(dev):
        nbytes = _lib.call_size("facl_knn_ws_bytes", nq, nb, k, detail="nq=%d, nb=%d, k=%d" % (nq, nb, k))
        ws = _lib.empty((nbytes + 3) // 4, dtype=torch.int32, device=dev)
        val = _lib.empty((nq, k), dtype=torch.float32, device=dev)
        idx = _lib.empty((nq, k), dtype=torch.int32, device=dev)
        _lib.call("facl_knn_topk", queries, nq, queries.stride(0), bank, nb, bank.stride(0), C, k, sidx, val, idx, ws,
                  detail="nq=%d, nb=%d, C=%d, k=%d" % (nq, nb, C, k))
    return val, idx


def knn_vote(values, indices, bank_labels, num_class, T=0.1):
    """(pred (nq) int32, scores (nq, num_class) float32) from the neighbours `knn_topk` returned: scores[c] = the sum of
    exp(s / T) over the neighbours labelled c, pred = argmax (the lower class on equal scores)."""
    _lib.require_cuda(values, indices, bank_labels)
    nq, k = values.shape
    dev = values.device
    values = values.float().contiguous()
    indices = indices.to(torch.int32).contiguous()
    labels = bank_labels.to(device=dev, dtype=torch.int32).contiguous()
    num_class = int(num_class)
    with torch.cuda.device(dev):
        pred = _lib.empty((nq,), dtype=torch.int32, device=dev)
        scores = _lib.empty((nq, max(num_class, 0)), dtype=torch.float32, device=dev)
        _lib.call("facl_knn_vote", values, indices, labels, nq, labels.shape[0], k, num_class, 1.0 / T, pred, scores,
                  detail="nq=%d, k=%d, num_class=%d" % (nq, k, num_class))
    return pred, scores


def knn_predict(queries, bank, bank_labels, k=20, T=0.1, num_class=None, self_idx=None):
    """(pred, scores) of the weighted kNN classifier; `num_class` defaults to max(bank_labels) + 1."""
    _lib.require_cuda(queries, bank, bank_labels)
    if num_class is None:
        num_class = int(bank_labels.max().item()) + 1
    val, idx = knn_topk(queries, bank, k, self_idx)
    return knn_vote(val, idx, bank_labels, num_class, T)


def knn_top1(queries, query_labels, bank, bank_labels, k=20, T=0.1, num_class=None, self_idx=None):
    """Top-1 accuracy in percent of `knn_predict` against `query_labels`."""
    _lib.require_cuda(queries, query_labels, bank, bank_labels)
    if num_class is None:
        num_class = int(max(bank_labels.max().item(), query_labels.max().item())) + 1
    pred, _ = knn_predict(queries, bank, bank_labels, k, T, num_class, self_idx)
    hit = int((pred.long() == query_labels.to(pred.device).long()).sum().item())
    return 100.0 * hit / max(queries.shape[0], 1)


def build_parser():
    from . import dataset as fds
    p = argparse.ArgumentParser(description="Weighted kNN evaluation of extracted features")
    p.add_argument('--dataset', type=str, default='ntu120', help='ntu120 | ntu60')
    p.add_argument('--main_gpu', type=int, default=0, help='main GPU id')
    p.add_argument('--data_root', type=str, default='../ntu/3DV_ntu60', help='the dataset root (as the linear probe)')
    p.add_argument('--split', type=str, default='view', choices=fds.SPLIT_MODES, help='view | subject | set')
    p.add_argument('--full_train', type=int, default=1, help='(--split subject): 0 = without the validation performers')
    p.add_argument('--motion_feature_dir', type=str, required=True, help='folder of <v_name>.npy motion features')
    p.add_argument('--appearance_feature_dir', type=str, default=None,
                   help='folder of <v_name>.npy appearance features (optional: one stream alone is accepted)')
    p.add_argument('--k', type=int, default=20, help='neighbours per query (1..64)')
    p.add_argument('--temperature', type=float, default=0.1, help='T of the exp(s / T) vote')
    return p


def main(args=None):
    """The test split classified against the train split as bank; prints and returns the top-1 (%)."""
    from .linear_classify import load_splits
    opt = build_parser().parse_args(args)
    print(opt)
    (ftr, ytr), (fte, yte) = load_splits(opt)
    top1 = knn_top1(fte, yte, ftr, ytr, k=opt.k, T=opt.temperature)
    print('knn top1:', top1)
    return top1


if __name__ == '__main__':
    main()
