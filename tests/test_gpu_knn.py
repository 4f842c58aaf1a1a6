"""The fused similarity-GEMM + top-k kernel and the weighted vote (csrc/knn.hip, facl_amd/knn_eval.py) against fp64
references computed here with torch.float64 on the device."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REL_TOL = 2e-6                # of the largest |similarity|: the bound tests/test_gpu_gemm.py holds facl_gemm_fwd to
NOISE = 5.0                   # test 5: isotropic noise around the class centres (see _end_to_end_data)


def _gauss(seed, *shape):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float32).to(DEV)


def _sims64(q, x):
    qn = q.double() / q.double().norm(dim=1, keepdim=True).clamp_min(1e-12)
    xn = x.double() / x.double().norm(dim=1, keepdim=True).clamp_min(1e-12)
    return qn @ xn.t()


def _check_topk(val, idx, S, k, tol):
    """The criterion of the kernel's contract: S (nq, nb) fp64 similarities with excluded entries at -inf."""
    nq = S.shape[0]
    assert val.shape == (nq, k) and idx.shape == (nq, k) and val.dtype == torch.float32 and idx.dtype == torch.int32
    idx = idx.long()
    assert int(idx.min()) >= 0 and int(idx.max()) < S.shape[1]
    vk = S.topk(k, dim=1).values[:, -1:]                                   # fp64 k-th largest per query
    own = S.gather(1, idx)                                                 # fp64 similarity of every returned index
    worst = float((vk - own).max())
    print("returned below the k-th by at most %.3e (tol %.3e)" % (worst, tol))
    assert bool((own >= vk - tol).all())
    must = S > vk + tol                                                    # rows that have to be returned
    got = torch.zeros_like(must)
    got.scatter_(1, idx, True)
    assert bool((got | ~must).all()), "a bank row clearly above the k-th similarity is missing"
    err = float((val.double() - own).abs().max())
    print("value error %.3e (tol %.3e)" % (err, tol))
    assert err <= tol
    assert bool((val[:, 1:] <= val[:, :-1]).all()), "values must be non-increasing"
    assert int(got.sum()) == nq * k, "an index repeats within a row"


@pytest.mark.parametrize("nq,nb,C,k", [(1, 64, 64, 64), (65, 129, 64, 64), (130, 1000, 512, 20), (200, 3000, 1536, 1),
                                       (3, 4100, 512, 5)])
def test_topk_against_fp64(nq, nb, C, k):
    from facl_amd.knn_eval import knn_topk
    q, x = _gauss(11 + nq, nq, C), _gauss(23 + nb, nb, C)
    S = _sims64(q, x)
    val, idx = knn_topk(q, x, k)
    _check_topk(val, idx, S, k, REL_TOL * float(S.abs().max()))


def test_topk_rows_with_a_leading_dimension_and_scales():
    """Rows of very different magnitude (each row has its own power-of-two scale) inside a wider buffer."""
    from facl_amd.knn_eval import knn_topk
    nq, nb, C, k = 70, 300, 128, 7
    qb, xb = _gauss(5, nq, C + 64), _gauss(6, nb, C + 64)
    xb *= torch.logspace(-6, 12, nb, device=DEV).unsqueeze(1)
    qb *= torch.logspace(8, -5, nq, device=DEV).unsqueeze(1)
    q, x = qb[:, :C], xb[:, :C]
    S = _sims64(q, x)
    val, idx = knn_topk(q, x, k)
    _check_topk(val, idx, S, k, REL_TOL * float(S.abs().max()))


def test_exact_ties_lower_index_first_and_bitwise_repeatable():
    from facl_amd.knn_eval import knn_topk
    nb, C, k = 1000, 64, 5
    x = _gauss(3, nb, C)
    x[300] = x[7]
    x[901] = x[7]
    q = x[7].unsqueeze(0) + 0.01 * _gauss(4, 4, C)                         # four queries that rank the copies first
    val, idx = knn_topk(q, x, k)                                           # 4 queries: the bank is split across workgroups
    assert idx[:, :3].tolist() == [[7, 300, 901]] * 4
    assert bool((val[:, 0] == val[:, 1]).all()) and bool((val[:, 1] == val[:, 2]).all())
    val2, idx2 = knn_topk(q, x, k)
    assert torch.equal(val.view(torch.int32), val2.view(torch.int32)) and torch.equal(idx, idx2)
    # enough query tiles that no workgroup splits the bank: the same rows, the same bits
    reps = 128 * 512 // 4 + 1
    vb, ib = knn_topk(q.repeat(reps, 1), x, k)
    assert torch.equal(vb.view(torch.int32), val.view(torch.int32).repeat(reps, 1)) and torch.equal(ib, idx.repeat(reps, 1))
    vb2, ib2 = knn_topk(q.repeat(reps, 1), x, k)
    assert torch.equal(vb.view(torch.int32), vb2.view(torch.int32)) and torch.equal(ib, ib2)


def test_self_idx_leaves_the_own_row_out():
    from facl_amd.knn_eval import knn_topk
    nb, C, k = 1000, 512, 20
    x = _gauss(8, nb, C)
    rows = torch.tensor([0, 17, nb - 1], device=DEV)
    q = x[rows].clone()
    S = _sims64(q, x)
    tol = REL_TOL * float(S.abs().max())
    val, idx = knn_topk(q, x, k, self_idx=rows)
    assert not bool((idx.long() == rows.unsqueeze(1)).any())
    Sx = S.clone()
    Sx[torch.arange(3, device=DEV), rows] = float("-inf")
    _check_topk(val, idx, Sx, k, tol)
    val, idx = knn_topk(q, x, k, self_idx=torch.full((3,), -1, device=DEV))
    assert idx[:, 0].tolist() == rows.tolist()
    assert float((val[:, 0].double() - 1.0).abs().max()) <= tol
    _check_topk(val, idx, S, k, tol)


def _vote64(val, idx, labels, num_class, T):
    w = torch.exp(val.double() * (1.0 / T))
    s = torch.zeros(val.shape[0], num_class, dtype=torch.float64, device=val.device)
    s.scatter_add_(1, labels.long()[idx.long()], w)
    return s


@pytest.mark.parametrize("k", [1, 20, 64])
@pytest.mark.parametrize("num_class", [1, 12, 120])
def test_vote_against_fp64(k, num_class):
    from facl_amd.knn_eval import knn_vote
    nq, nb, T = 67, 500, 0.07
    g = torch.Generator().manual_seed(100 * k + num_class)
    val = (torch.rand(nq, k, generator=g) * 2 - 1).sort(dim=1, descending=True).values.to(DEV)
    idx = torch.randint(0, nb, (nq, k), generator=g, dtype=torch.int32).to(DEV)
    labels = torch.randint(0, num_class, (nb,), generator=g, dtype=torch.int32).to(DEV)
    pred, scores = knn_vote(val, idx, labels, num_class, T)
    ref = _vote64(val, idx, labels, num_class, T)
    rel = float(((scores.double() - ref).abs() / ref.clamp_min(1e-300)).max())
    print("scores: max relative error %.3e" % rel)
    assert bool((scores.double() - ref).abs().le(1e-5 * ref).all())
    assert torch.equal(pred.long(), ref.argmax(dim=1))


def test_vote_equal_scores_pick_the_lower_class():
    from facl_amd.knn_eval import knn_vote
    val = torch.tensor([[0.5, 0.5], [0.75, 0.25]], device=DEV)
    idx = torch.tensor([[0, 1], [0, 1]], dtype=torch.int32, device=DEV)
    labels = torch.tensor([5, 3], dtype=torch.int32, device=DEV)
    pred, scores = knn_vote(val, idx, labels, 8, 0.07)
    assert float(scores[0, 5]) == float(scores[0, 3]) > 0                  # bit-equal class scores
    assert pred.tolist() == [3, 5]


def _end_to_end_data():
    g = torch.Generator().manual_seed(2024)
    centres = torch.randn(12, 512, generator=g)
    yb, yq = torch.arange(600) % 12, torch.arange(130) % 12
    bank = centres[yb] + NOISE * torch.randn(600, 512, generator=g)
    query = centres[yq] + NOISE * torch.randn(130, 512, generator=g)
    return [t.to(DEV) for t in (query, yq, bank, yb)]


def test_end_to_end_prediction_against_fp64():
    from facl_amd.knn_eval import knn_predict, knn_top1
    q, yq, x, yb = _end_to_end_data()
    k, T = 20, 0.1
    S = _sims64(q, x)
    tv, ti = S.topk(k, dim=1)
    ref = _vote64(tv, ti, yb, 12, T)
    ref_pred = ref.argmax(dim=1)
    ref_acc = 100.0 * float((ref_pred == yq).double().mean())
    print("fp64 kNN accuracy %.2f %%" % ref_acc)
    assert 50.0 < ref_acc < 95.0
    top2 = ref.topk(2, dim=1).values
    clear = (top2[:, 0] - top2[:, 1]) > 1e-3 * top2[:, 0]
    assert int((~clear).sum()) <= 0.02 * q.shape[0]
    pred, scores = knn_predict(q, x, yb, k=k, T=T, num_class=12)
    assert scores.shape == (130, 12)
    assert torch.equal(pred.long()[clear], ref_pred[clear])
    acc = 100.0 * int((pred.long() == yq).sum()) / 130
    assert knn_top1(q, yq, x, yb, k=k, T=T, num_class=12) == acc
    assert knn_top1(q, yq, x, yb, k=k, T=T) == acc                         # num_class from the labels


def test_domain_edges_return_codes_without_launching():
    from facl_amd import _lib
    lib = _lib.load_library()
    nq, nb, C = 4, 40, 64
    q, x = _gauss(1, nq, 128), _gauss(2, nb, 128)
    val = torch.full((nq, 64), 7.0, device=DEV)
    idx = torch.full((nq, 64), 7, dtype=torch.int32, device=DEV)
    ws = torch.zeros(1 << 16, dtype=torch.int32, device=DEV)
    sidx = torch.full((nq,), -1, dtype=torch.int32, device=DEV)
    p, st = _lib.ptr, _lib.stream()

    def topk(k, C=C, nb=nb, out=val, self_idx=None, q=q):
        return lib.facl_knn_topk(p(q), nq, 128, p(x), nb, 128, C, k, p(self_idx), p(out), p(idx), p(ws), st)

    assert topk(0) == -1 and topk(65) == -1                               # FACL_E_SHAPE
    assert topk(41) == -1 and topk(40, self_idx=sidx) == -1               # nb < k; nb - 1 < k with rows excluded
    assert topk(5, C=96) == -1 and topk(5, C=0) == -1
    assert topk(5, nb=0) == -1
    assert topk(5, out=None) == -2                                        # FACL_E_NULL
    assert lib.facl_knn_topk(p(q), nq, 128, p(x), nb, 128, C, 5, None, p(val), None, p(ws), st) == -2
    assert lib.facl_knn_topk(None, nq, 128, p(x), nb, 128, C, 5, None, p(val), p(idx), p(ws), st) == -2
    assert lib.facl_knn_topk(p(q) + 4, nq, 128, p(x), nb, 128, C, 5, None, p(val), p(idx), p(ws), st) == -3   # FACL_E_ALIGN
    labels = torch.zeros(nb, dtype=torch.int32, device=DEV)
    pred = torch.full((nq,), 7, dtype=torch.int32, device=DEV)

    def vote(k, num_class, pred=pred):
        return lib.facl_knn_vote(p(val), p(idx), p(labels), nq, nb, k, num_class, 10.0, p(pred), None, st)

    assert vote(0, 3) == -1 and vote(65, 3) == -1 and vote(5, 0) == -1 and vote(5, 1025) == -1
    assert vote(5, 3, pred=None) == -2
    torch.cuda.synchronize()
    assert bool((val == 7.0).all()) and bool((idx == 7).all()) and bool((pred == 7).all())   # nothing was launched
    assert topk(40) == 0 and vote(40, 3) == 0                             # the edge of the domain itself runs
    torch.cuda.synchronize()
    got = idx.view(-1)[:nq * 40].view(nq, 40).long().sort(dim=1).values
    assert bool((got == torch.arange(40, device=DEV)).all())                # k = nb: every bank row, once
