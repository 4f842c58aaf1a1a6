"""The prototype contrastive term (csrc/proto.hip, facl_amd/proto.py, --proto_weight of the training entries)
against an fp64 NumPy restatement of the formula, and its invariants: unknown and out-of-range ids, run-to-run and replayed
bits, exact row scaling, and the training entry."""
import functools
import os
import re

import numpy as np
import pytest
import torch

from poison import poisoned_scratch  # noqa: F401
from synth_tree import epoch_loss_text, run_train_entry, train_argv, write_tree

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu().numpy()


def _poison_buffers(M, C, K):
    """NaN into the op's static outputs (not the err word), so that an element the launch leaves unwritten shows."""
    from facl_amd import proto
    d, loss, ws, _ = proto.buffers(torch.device(DEV), M, C, K)
    d.fill_(float("nan"))
    loss.fill_(float("nan"))
    ws.fill_(float("nan"))
    return d


# ---- inputs and the two references --------------------------------------------------------------------------------------------------
SHAPES = [(1, 1, 64, 1), (2, 3, 64, 5), (3, 5, 192, 17), (10, 4, 512, 65), (24, 32, 512, 60), (24, 32, 512, 1024)]


def _inputs(G, B, C, K, seed=None):
    from facl_amd import cluster as fcl
    rng = np.random.RandomState(G * 1000 + B * 100 + C + K if seed is None else seed)
    M = (G + 1) * B
    x = (rng.randn(M, C) * 10.0 ** rng.uniform(-3, 3, size=(M, 1))).astype(np.float32)      # row norms over six decades
    if M > 2:
        x[1] = 0.0                                           # one all-zero row
    protos = (rng.randn(K, C) * rng.uniform(0.5, 40.0, size=(K, 1))).astype(np.float32)     # un-normalised sums
    if K > 1:
        protos[K // 2] = 0.0                                 # one all-zero prototype
    scale = rng.uniform(1.0, 50.0, size=K).astype(np.float32)
    classes = rng.randint(0, K, size=B).astype(np.int32)
    if B > 1:
        classes[rng.rand(B) < 0.3] = -1                      # -1 mixed with valid ids
        classes[0], classes[B - 1] = -1, K - 1               # at least one of each
    d_protos = _dev(protos)
    proto_inv = fcl.row_inv(d_protos)
    return dict(G=G, B=B, C=C, K=K, M=M, x=x, protos=protos, scale=scale, classes=classes, d_x=_dev(x), d_protos=d_protos,
                d_inv=proto_inv, d_scale=_dev(scale), d_classes=_dev(classes), proto_inv=proto_inv.cpu().numpy())


def _ref64(x, classes, protos, proto_inv, scale):
    """The issue's formula in fp64 on the float32 inputs -> (loss, dx (M, C), inv (M))."""
    x, c, a = x.astype(np.float64), protos.astype(np.float64), scale.astype(np.float64)
    M, K = x.shape[0], c.shape[0]
    inv = 1.0 / np.maximum(np.sqrt((x * x).sum(axis=1)), 1e-12)
    z = x * inv[:, None]
    p = c * proto_inv.astype(np.float64)[:, None]
    l = (z @ p.T) * a[None, :]
    s = classes[np.arange(M) % classes.shape[0]].astype(np.int64)
    known = (s >= 0) & (s < K)
    m = l.max(axis=1, keepdims=True)
    lse = m[:, 0] + np.log(np.exp(l - m).sum(axis=1))
    sc = np.where(known, s, 0)
    loss = ((lse - l[np.arange(M), sc]) * known).sum() / M
    dl = np.exp(l - lse[:, None])
    dl[np.arange(M), sc] -= 1.0
    dl *= known[:, None] / M
    dz = (dl * a[None, :]) @ p
    dx = inv[:, None] * (dz - z * (dz * z).sum(axis=1, keepdims=True))
    return loss, dx, inv


def _torch32(d_x, d_classes, d_protos, d_inv, d_scale):
    """The same formula with torch in fp32 on the device: F.normalize, mm, log_softmax, autograd -> (loss, dx) as fp64 arrays."""
    x = d_x.clone().requires_grad_(True)
    M, K = x.shape[0], d_protos.shape[0]
    z = torch.nn.functional.normalize(x, dim=1)
    l = torch.mm(z, (d_protos * d_inv[:, None]).t()) * d_scale[None, :]
    s = d_classes.long()[torch.arange(M, device=x.device) % d_classes.shape[0]]
    known = (s >= 0) & (s < K)
    logp = torch.log_softmax(l, dim=1)
    loss = -(logp[torch.arange(M, device=x.device), torch.where(known, s, torch.zeros_like(s))] * known).sum() / M
    loss.backward()
    return float(loss.double().item()), x.grad.double().cpu().numpy()


@functools.lru_cache(maxsize=None)
def _measured(shape):
    """One evaluation per shape, shared by the tests below: the kernel (through autograd), torch-fp32 and fp64."""
    from facl_amd import proto
    G, B, C, K = shape
    t = _inputs(G, B, C, K)
    _poison_buffers(t["M"], C, K)
    x = t["d_x"].clone().requires_grad_(True)
    loss = proto.proto_nce(x, t["d_classes"], t["d_protos"], t["d_inv"], t["d_scale"])
    loss.backward()
    torch.cuda.synchronize()
    got_loss, got_dx = float(loss.double().item()), x.grad.double().cpu().numpy()
    # grad_out = 1: the gradient autograd hands back is the kernel's dstacked, bit for bit
    assert (_bits(x.grad) == _bits(proto.buffers(torch.device(DEV), t["M"], C, K)[0])).all()
    loss64, dx64, inv = _ref64(t["x"], t["classes"], t["protos"], t["proto_inv"], t["scale"])
    t32_loss, t32_dx = _torch32(t["d_x"], t["d_classes"], t["d_protos"], t["d_inv"], t["d_scale"])
    a_max = float(t["scale"].max())
    delta = a_max * (C + 8) * 2.0 ** -24
    bound = 2.0 * delta + 2.0 ** -23 * abs(loss64)
    unit = inv * a_max / t["M"]                              # a row's natural gradient magnitude
    e_dx = (np.abs(got_dx - dx64).max(axis=1) / unit).max()
    e_dx32 = (np.abs(t32_dx - dx64).max(axis=1) / unit).max()
    return dict(t=t, loss=got_loss, loss64=loss64, bound=bound, e_loss=abs(got_loss - loss64), e_loss32=abs(t32_loss - loss64),
                e_dx=e_dx, e_dx32=e_dx32, dx=got_dx, dx64=dx64)


# ---- 1: the op against fp64 -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_op_vs_fp64(shape):
    """Hard bound (derived): every logit carries at most delta = a_max (C + 8) 2^-24 of fp32 summation error on unit vectors and
    logsumexp is 1-Lipschitz in the sup norm, so |loss - loss64| <= 2 delta + 2^-23 |loss64|.  Tighter bar for dx, against a
    reference and not against the code under test: the worst row error, in units of inv_r a_max / M, is at most 4 x that of the
    same formula evaluated by torch in fp32 on the device (the 4 is for differing summation orders); the same holds for the loss.
    Measured on an MI355X, kernel / torch-fp32: loss |err| 0 / 0, 9.3e-8 / 1.5e-7, 1.3e-7 / 1.3e-7, 9.4e-9 / 2.3e-7, 1.6e-8 / 1.6e-8,
    9.6e-8 / 8.6e-7; dx worst (units) 0 / 0, 3.0e-8 / 4.9e-8, 4.4e-8 / 1.1e-7, 9.2e-8 / 1.1e-7, 7.6e-8 / 1.8e-7, 2.8e-7 / 2.8e-7."""
    G, B, C, K = shape
    r = _measured(shape)
    print("proto_nce %s: loss %.9g |err| %.3e (bound %.3e, torch-fp32 %.3e); dx worst %.4e units (torch-fp32 %.4e)"
          % (shape, r["loss"], r["e_loss"], r["bound"], r["e_loss32"], r["e_dx"], r["e_dx32"]))
    assert np.isfinite(r["loss"]) and np.isfinite(r["dx"]).all()
    assert r["e_loss"] <= r["bound"]
    assert r["e_dx"] <= 4.0 * r["e_dx32"] and r["e_loss"] <= 4.0 * r["e_loss32"]
    if K == 1:                                               # one prototype: softmax = onehot
        assert abs(r["loss"]) <= r["bound"] and r["e_dx"] <= 2.0 ** -20                # the loss is 0, dx ~ 0 in its natural unit
    # the rows of unknown clips are zero bits (the mixed case)
    t = r["t"]
    unknown = np.flatnonzero(t["classes"][np.arange(t["M"]) % B] < 0)
    assert (r["dx"][unknown].view(np.int64) == 0).all()
    if B > 1:
        assert len(unknown) == (G + 1) * int((t["classes"] < 0).sum()) > 0


def test_loss_error_against_torch_fp32():
    """The tighter bar once more over the six shapes together (test_op_vs_fp64 holds it shape by shape): the kernel's worst loss
    error, each in units of its shape's hard bound, is at most 4 x torch-fp32's worst in the same units.  Prints both worst values."""
    rs = [_measured(s) for s in SHAPES]
    worst = max(r["e_loss"] / r["bound"] for r in rs)
    worst32 = max(r["e_loss32"] / r["bound"] for r in rs)
    print("proto_nce loss, worst |err| / bound over the shapes: kernel %.4e, torch-fp32 %.4e" % (worst, worst32))
    print("proto_nce dx, worst over the shapes: kernel %.4e units, torch-fp32 %.4e units"
          % (max(r["e_dx"] for r in rs), max(r["e_dx32"] for r in rs)))
    assert worst <= 4.0 * worst32


# ---- 2: unknown ids ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 3, 64, 5), (24, 32, 512, 60)])
def test_all_unknown_is_positive_zero(shape):
    from facl_amd import proto
    G, B, C, K = shape
    t = _inputs(G, B, C, K)
    d = _poison_buffers(t["M"], C, K)
    loss = proto.proto_nce(t["d_x"], _dev(np.full(B, -1, dtype=np.int32)), t["d_protos"], t["d_inv"], t["d_scale"])
    assert _bits(loss.reshape(1)).tolist() == [0]            # +0.0
    assert (_bits(d) == 0).all()


# ---- 3: an id out of range --------------------------------------------------------------------------------------------------------
def test_id_out_of_range_raises_and_reads_nothing():
    from facl_amd import proto
    G, B, C, K = 3, 5, 192, 17
    t = _inputs(G, B, C, K)
    for bad_id in (K, 2 ** 31 - 1):
        bad = t["classes"].copy()
        bad[2] = bad_id
        d = _poison_buffers(t["M"], C, K)
        with pytest.raises(RuntimeError, match=r"outside the range \[0, %d\)" % K):
            proto.proto_nce(t["d_x"], _dev(bad), t["d_protos"], t["d_inv"], t["d_scale"])
        got, loss_bad = _bits(d).copy(), _bits(proto.buffers(torch.device(DEV), t["M"], C, K)[1]).copy()
        bad[2] = -1
        _poison_buffers(t["M"], C, K)
        loss = proto.proto_nce(t["d_x"], _dev(bad), t["d_protos"], t["d_inv"], t["d_scale"])      # the word was cleared: no raise
        assert (got == _bits(d)).all() and loss_bad.tolist() == _bits(loss.reshape(1)).tolist()
        assert (got[2::B] == 0).all() and (got[B - 1::B] != 0).any()  # classes[B - 1] is valid by construction


# ---- 4: run to run, and replayed --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 5, 192, 17), (24, 32, 512, 60)])
def test_same_bits_again_and_replayed(shape):
    from facl_amd import proto
    G, B, C, K = shape
    t = _inputs(G, B, C, K)
    args = (t["d_x"], t["d_classes"], t["d_protos"], t["d_inv"], t["d_scale"])
    runs = []
    for _ in range(2):
        d = _poison_buffers(t["M"], C, K)
        loss = proto.proto_nce(*args)
        runs.append((_bits(loss.reshape(1)).copy(), _bits(d).copy()))
    assert (runs[0][0] == runs[1][0]).all() and (runs[0][1] == runs[1][1]).all()
    assert np.isfinite(runs[0][1].view(np.float32)).all()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        loss_g, _ = proto.proto_nce_raw(*args)
        d_g = proto.buffers(torch.device(DEV), t["M"], C, K)[0]                  # the capture stream's own static buffers
    for _ in range(2):
        d_g.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert (_bits(loss_g.reshape(1)) == runs[0][0]).all() and (_bits(d_g) == runs[0][1]).all()


# ---- 5: row scaling ---------------------------------------------------------------------------------------------------------------
def test_scaling_a_row_by_a_power_of_two():
    from facl_amd import proto
    G, B, C, K = 2, 3, 64, 5
    t = _inputs(G, B, C, K)
    M = t["M"]
    x = (np.random.RandomState(5).randn(M, C)).astype(np.float32)              # norms near 8: no power below reaches a subnormal
    cls = _dev(np.array([1, 4, 0], dtype=np.int32))
    d = _poison_buffers(M, C, K)
    loss = proto.proto_nce(_dev(x), cls, t["d_protos"], t["d_inv"], t["d_scale"])
    base_loss, base = _bits(loss.reshape(1)).copy(), d.cpu().numpy().copy()
    for row, k in ((4, 7), (0, -5), (M - 1, 20)):
        y = x.copy()
        y[row] *= np.float32(2.0 ** k)
        _poison_buffers(M, C, K)
        loss = proto.proto_nce(_dev(y), cls, t["d_protos"], t["d_inv"], t["d_scale"])
        got = d.cpu().numpy()
        assert (_bits(loss.reshape(1)) == base_loss).all()
        want = base.copy()
        want[row] *= np.float32(2.0 ** -k)
        assert np.abs(want[row]).max() > 0 and (got.view(np.int32) == want.view(np.int32)).all(), (row, k)


# ---- 6: the training entry --------------------------------------------------------------------------------------------------------
CLUSTER = ("--loss_mask", "class", "--class_ids", "cluster", "--clusters", "3", "--cluster_every", "1")


def _run_entry(root, folder, *extra):
    mode = ("--loss_normalize", "1", "--loss_temperature", "0.1", "--neg_queue", "8", "--nepoch", "2")
    return run_train_entry(train_argv(root, folder, *extra, before_save=mode, features_first=True))


def _checkpoints(folder):
    names = sorted(n for n in os.listdir(str(folder)) if n.endswith(".pth"))
    return {n: torch.load(os.path.join(str(folder), n), map_location="cpu", weights_only=True) for n in names}


def test_train_entry_with_prototypes(tmp_path):
    root = tmp_path / "d"
    write_tree(str(root))
    sd_p, out_p = _run_entry(root, tmp_path / "p", *CLUSTER, "--proto_weight", "1.0")
    lines = re.findall(r"epoch: (\d+) prototypes: 3 concentration min/mean/max: (\S+)/(\S+)/(\S+)", out_p)
    assert [l[0] for l in lines] == ["0", "1"], out_p
    for l in lines:
        lo, mean, hi = (float(v) for v in l[1:])
        assert 0.0 < lo <= mean <= hi and np.isfinite(hi)
    sd_n, out_n = _run_entry(root, tmp_path / "n", *CLUSTER)
    assert "prototypes:" not in out_n
    # epoch 0: every id is unknown, the term is +0.0 and its gradient zero
    assert epoch_loss_text(out_p, 0) == epoch_loss_text(out_n, 0)
    # epoch 1 trains against the prototypes of the first clustering
    assert sd_p.keys() == sd_n.keys()
    assert any(not torch.equal(sd_p[k], sd_n[k]) for k in sd_p)
    # two identical runs give bit-identical weights and checkpoint files
    sd_q, out_q = _run_entry(root, tmp_path / "q", *CLUSTER, "--proto_weight", "1.0")
    assert [epoch_loss_text(out_q, e) for e in (0, 1)] == [epoch_loss_text(out_p, e) for e in (0, 1)]
    assert re.findall(r"prototypes: .*", out_q) == re.findall(r"prototypes: .*", out_p)
    for k in sd_p:
        assert torch.equal(sd_p[k], sd_q[k]), k
    ck_p, ck_q = _checkpoints(tmp_path / "p"), _checkpoints(tmp_path / "q")
    assert ck_p and ck_p.keys() == ck_q.keys()
    for nm in ck_p:
        assert ck_p[nm].keys() == ck_q[nm].keys() and all(torch.equal(ck_p[nm][k], ck_q[nm][k]) for k in ck_p[nm]), nm
    # weight 0 is the run without the flag: every printed loss, every weight
    sd_0, out_0 = _run_entry(root, tmp_path / "z", *CLUSTER, "--proto_weight", "0")
    assert "prototypes:" not in out_0
    assert [epoch_loss_text(out_0, e) for e in (0, 1)] == [epoch_loss_text(out_n, e) for e in (0, 1)]
    for k in sd_n:
        assert torch.equal(sd_n[k], sd_0[k]), k
    # the term is part of the captured step: the graphed run replays it against the static prototypes and walks the eager trajectory
    sd_g, out_g = _run_entry(root, tmp_path / "g", *CLUSTER, "--proto_weight", "1.0", "--graph", "1")
    assert "graph capture failed" not in out_g
    assert [epoch_loss_text(out_g, e) for e in (0, 1)] == [epoch_loss_text(out_p, e) for e in (0, 1)]
    assert re.findall(r"prototypes: .*", out_g) == re.findall(r"prototypes: .*", out_p)
    for k in sd_p:
        assert torch.equal(sd_p[k], sd_g[k]), k
