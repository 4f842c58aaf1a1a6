"""The kernels of csrc/cls.hip against torch fp64 on the same inputs: the gathered F.normalize of the stacked, view-major
encoder output (forward and backward) and the softmax cross-entropy with its gradient and counters.  NaN-poisoned scratch."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from poison import poisoned_scratch  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _gather64(stacked, G, B):
    """(G*B + B, C) view-major rows -> (B, (G+1)*C) fp64 clip-major vectors [view0 .. view(G-1), global]."""
    C = stacked.shape[1]
    return stacked.double().view(G + 1, B, C).permute(1, 0, 2).reshape(B, (G + 1) * C)


def _scatter(clip_major, G, B, C):
    """the inverse layout map: (B, (G+1)*C) -> (G*B + B, C)."""
    return clip_major.view(B, G + 1, C).permute(1, 0, 2).reshape((G + 1) * B, C)


def _gn_fwd(stacked, G, B):
    from facl_amd import _lib
    lib = _lib.load_library()
    C = stacked.shape[1]
    out = torch.full((B, (G + 1) * C), float("nan"), device=DEV)
    inv = torch.full((B,), float("nan"), device=DEV)
    _lib.check(lib.facl_cls_gather_norm_fwd(_lib.ptr(stacked), G, B, C, _lib.ptr(out), _lib.ptr(inv), _lib.stream()), "fwd")
    return out, inv


def _gn_bwd(dout, out, inv, G, B, C):
    from facl_amd import _lib
    lib = _lib.load_library()
    ds = torch.full(((G + 1) * B, C), float("nan"), device=DEV)
    _lib.check(lib.facl_cls_gather_norm_bwd(_lib.ptr(dout), _lib.ptr(out), _lib.ptr(inv), G, B, C, _lib.ptr(ds), _lib.stream()), "bwd")
    return ds


GN_CASES = [(1, 1, 512), (2, 3, 512), (24, 32, 512), (64, 2, 512), (3, 5, 64)]


@pytest.mark.parametrize("G,B,C", GN_CASES)
def test_gather_norm_forward_and_backward_vs_fp64(G, B, C):
    gen = torch.Generator(device=DEV)
    gen.manual_seed(G * 1000 + B)
    stacked = torch.randn((G + 1) * B, C, device=DEV, generator=gen) * (0.5 + torch.rand((G + 1) * B, 1, device=DEV, generator=gen) * 4)
    if B > 1:
        stacked[torch.arange(G + 1, device=DEV) * B + 1] = 0.0                    # clip 1: all G + 1 rows zero
    out, inv = _gn_fwd(stacked, G, B)
    out2, inv2 = _gn_fwd(stacked, G, B)
    assert torch.equal(out, out2) and torch.equal(inv, inv2)                       # the same bits every run
    x64 = _gather64(stacked, G, B)
    inv64 = 1.0 / x64.norm(dim=1).clamp_min(1e-12)
    ref = (x64 * inv64[:, None]).cpu().numpy()
    got = out.cpu().numpy()
    assert np.isfinite(got).all()
    # 2 fp32 ulp of the fp64 result: one rounding of inv, one of the product
    ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    worst = float((np.abs(got.astype(np.float64) - ref) / ulp).max())
    i64 = inv64.cpu().numpy()
    worst_inv = float((np.abs(inv.cpu().numpy().astype(np.float64) - i64) / np.spacing(i64.astype(np.float32)).astype(np.float64)).max())
    print("gather_norm fwd G=%d B=%d C=%d: %.2f ulp, inv %.2f ulp" % (G, B, C, worst, worst_inv))
    assert worst <= 2.0 and worst_inv <= 1.0
    if B > 1:
        assert (got[1] == 0).all() and float(inv[1]) == float(np.float32(1e12))   # zeros, not NaN

    # backward against fp64 autograd of F.normalize on the gathered vector
    dout = torch.randn(B, (G + 1) * C, device=DEV, generator=gen)
    ds = _gn_bwd(dout, out, inv, G, B, C)
    assert torch.equal(ds, _gn_bwd(dout, out, inv, G, B, C))
    assert torch.isfinite(ds).all()                                               # every row of dstacked was written

    def autograd(dtype):
        x = _gather64(stacked, G, B).to(dtype).requires_grad_(True)
        F.normalize(x, p=2, dim=1).backward(dout.to(dtype))
        return x.grad.double()
    g64, g32 = autograd(torch.float64), autograd(torch.float32)
    mine = _gather64(ds, G, B)
    scale = g64.abs().amax(dim=1).clamp_min(1e-300)
    e_mine = ((mine - g64).abs().amax(dim=1) / scale).cpu().numpy()
    e_32 = ((g32 - g64).abs().amax(dim=1) / scale).cpu().numpy()
    print("gather_norm bwd: kernel %.2e, torch fp32 %.2e" % (e_mine.max(), e_32.max()))
    assert (e_mine <= np.maximum(4 * e_32, 1e-7)).all(), (e_mine, e_32)


def test_gather_norm_autograd_function_matches_the_entries():
    from facl_amd.cls_head import gather_norm
    G, B, C = 2, 3, 512
    torch.manual_seed(0)
    stacked = torch.randn((G + 1) * B, C, device=DEV, requires_grad=True)
    out = gather_norm(stacked, G, B)
    dout = torch.randn_like(out)
    out.backward(dout)
    o, inv = _gn_fwd(stacked.detach(), G, B)
    assert torch.equal(out.detach(), o) and torch.equal(stacked.grad, _gn_bwd(dout, o, inv, G, B, C))


# ---- softmax cross-entropy ---------------------------------------------------------------------------------------------------
def _ce(logits, labels, ncls, want_grad=True):
    """facl_softmax_ce on a (R, ld) buffer whose first ncls columns are the logits -> (loss, dlogits, stats)."""
    from facl_amd import _lib
    from facl_amd.sa_mlp import _Workspace
    lib = _lib.load_library()
    R, ld = logits.shape
    loss = torch.full((1,), float("nan"), device=DEV)
    d = torch.full((R, ncls), float("nan"), device=DEV) if want_grad else None
    stats = torch.full((2,), -7, dtype=torch.int32, device=DEV)
    ws = _Workspace.get(torch.device(DEV))
    _lib.check(lib.facl_softmax_ce(_lib.ptr(logits), ld, _lib.ptr(labels), R, ncls, _lib.ptr(loss), _lib.ptr(d), _lib.ptr(stats),
                                   _lib.ptr(ws), _lib.stream()), "facl_softmax_ce")
    return loss, d, stats


def _torch_ce(x, y, dtype):
    z = x.to(dtype).requires_grad_(True)
    loss = F.cross_entropy(z, y.long())
    loss.backward()
    return loss.detach().double(), z.grad.double()


@pytest.mark.parametrize("ncls", [2, 60, 64, 65, 120, 1024])
@pytest.mark.parametrize("R", [1, 3, 64, 65])
def test_softmax_ce_vs_fp64(R, ncls):
    gen = torch.Generator(device=DEV)
    gen.manual_seed(R * 2000 + ncls)
    for scale in (1.0, 1e4):
        x = torch.randn(R, ncls, device=DEV, generator=gen) * scale
        top = x.argmax(dim=1, keepdim=True)
        x.scatter_add_(1, top, torch.full((R, 1), scale, device=DEV))              # the maximum leads by >= 1e-3: no near-tie
        y = torch.randint(0, ncls, (R,), device=DEV, generator=gen).to(torch.int32)
        y[0] = int(top[0])                                                        # at least one hit
        l64, g64 = _torch_ce(x, y, torch.float64)
        l32, g32 = _torch_ce(x, y, torch.float32)
        hits = int((x.double().argmax(dim=1) == y.long()).sum())
        for pad in (0, 3):
            buf = torch.full((R, ncls + pad), float("nan"), device=DEV)
            buf[:, :ncls] = x
            loss, d, stats = _ce(buf, y, ncls)
            loss2, d2, stats2 = _ce(buf, y, ncls)
            assert torch.equal(loss, loss2) and torch.equal(d, d2) and torch.equal(stats, stats2)
            assert torch.isfinite(loss).all() and torch.isfinite(d).all()         # 1e4-scaled logits must not overflow
            e_l, e_l32 = abs(float(loss) - float(l64)), abs(float(l32) - float(l64))
            e_g, e_g32 = float((d.double() - g64).abs().max()), float((g32 - g64).abs().max())
            gmax = float(g64.abs().max())
            print("softmax_ce R=%d ncls=%d scale=%g ld=+%d: loss %.2e (torch fp32 %.2e) of %.3e, dlogits %.2e (%.2e) of %.3e"
                  % (R, ncls, scale, pad, e_l, e_l32, float(l64), e_g, e_g32, gmax))
            assert e_l <= max(4 * e_l32, 1e-6 * abs(float(l64)))
            assert e_g <= max(4 * e_g32, 1e-6 * gmax)
            assert stats.tolist() == [hits, 0]
            # without a gradient buffer: the same loss and counters
            loss3, _, stats3 = _ce(buf, y, ncls, want_grad=False)
            assert torch.equal(loss3, loss) and torch.equal(stats3, stats)


@pytest.mark.parametrize("ncls", [2, 60, 65, 1024])
def test_softmax_ce_equal_logits_and_ties(ncls):
    # row 0: all logits equal -> loss log(ncls), argmax 0 (its label is the last class: no hit);
    # row 1: the two largest logits equal, the label the higher class -> argmax is the lower one: no hit;
    # row 2: the same row, the label the lower class -> a hit
    x = torch.zeros(3, ncls, device=DEV)
    x[0] = 0.75
    lo, hi = (0, 1) if ncls == 2 else (ncls // 3, ncls - 2)
    x[1:, :] = torch.linspace(-2.0, -1.0, ncls, device=DEV)
    x[1:, lo] = x[1:, hi] = 3.0
    y = torch.tensor([ncls - 1, hi, lo], dtype=torch.int32, device=DEV)
    loss, d, stats = _ce(x, y, ncls)
    assert stats.tolist() == [1, 0]
    l64, g64 = _torch_ce(x, y, torch.float64)
    assert abs(float(loss) - float(l64)) <= 1e-6 * float(l64)
    one = _ce(x[:1].contiguous(), y[:1].contiguous(), ncls)
    assert abs(float(one[0]) - math.log(ncls)) <= 1e-6 * math.log(ncls) and one[2].tolist() == [0, 0]
    y0 = torch.zeros(1, dtype=torch.int32, device=DEV)
    assert _ce(x[:1].contiguous(), y0, ncls)[2].tolist() == [1, 0]                  # argmax of equal logits is class 0
    assert float((d.double() - g64).abs().max()) <= 1e-6 * float(g64.abs().max())


@pytest.mark.parametrize("R,ncls", [(5, 60), (65, 7)])
def test_softmax_ce_labels_outside_the_range(R, ncls):
    gen = torch.Generator(device=DEV)
    gen.manual_seed(5)
    x = torch.randn(R, ncls, device=DEV, generator=gen)
    y = torch.randint(0, ncls, (R,), device=DEV, generator=gen).to(torch.int32)
    y[1], y[R - 2] = -1, ncls
    ok = torch.ones(R, dtype=torch.bool, device=DEV)
    ok[1] = ok[R - 2] = False
    loss, d, stats = _ce(x, y, ncls)
    z = x[ok].double().requires_grad_(True)
    ref = F.cross_entropy(z, y[ok].long(), reduction="sum") / R                  # such a row still counts in R
    ref.backward()
    assert stats.tolist() == [int((x[ok].argmax(dim=1) == y[ok].long()).sum()), 2]
    assert abs(float(loss) - float(ref)) <= 1e-6 * float(ref)
    assert (d[~ok] == 0).all()
    assert float((d[ok].double() - z.grad).abs().max()) <= 1e-6 * float(z.grad.abs().max())


def test_classifier_head_matches_final_fc():
    """ClipClassifier on the stacked output == linear_classify.Final_FC on extract_batch's layout, same keys and weights."""
    from facl_amd.cls_head import ClipClassifier
    from facl_amd.linear_classify import Final_FC
    G, B, ncls = 3, 5, 12
    torch.manual_seed(3)
    head = ClipClassifier(G, ncls).to(DEV)
    probe = Final_FC(input_dim=512, gost=G + 1, num_class=ncls).to(DEV)
    probe.load_state_dict(head.state_dict(), strict=True)
    assert abs(float(head.fc.weight.std()) - 0.01) < 1e-3 and float(head.fc.bias.abs().max()) == 0.0
    stacked = torch.randn((G + 1) * B, 512, device=DEV, requires_grad=True)
    logits = head(stacked, G, B)
    feat = stacked.detach().reshape(G + 1, B, 512).permute(1, 0, 2).reshape(B, (G + 1) * 512)
    want = probe(feat)
    assert float((logits - want).abs().max()) <= 1e-5 * float(want.abs().max())
    y = torch.randint(0, ncls, (B,), device=DEV).to(torch.int32)
    loss, stats = head.loss(logits, y)
    loss.backward()
    assert abs(float(loss) - float(F.cross_entropy(want.double(), y.long()))) <= 1e-5 * float(loss)
    assert stacked.grad is not None and torch.isfinite(stacked.grad).all() and head.fc.weight.grad is not None
    assert int(stats[0]) == int((want.argmax(dim=1) == y.long()).sum()) and int(stats[1]) == 0
