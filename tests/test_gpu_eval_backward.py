"""Eval-mode backward of the encoder (BatchNorm frozen at its running statistics): every conv/linear -> BN -> ReLU
site alone, the whole FineTuneNet in eval(), a frozen FineTuneStep, and the --freeze_bn entry, against torch fp64 with eval-mode
BatchNorm (tests/eval_grad_ref.py) routed through the kernel's own max-pool and ReLU decisions.

In every test the running statistics sit AWAY from the batch's own (mean + 0.1 standard deviations, 1.3 x the variance, from a
train-mode fp64 evaluation of the same batch): a backward that used batch statistics, or kept a batch-statistic term, fails.
The bar is the fine-tuning step's own, TOL = 1e-4 (tests/test_gpu_finetune.py); the same routed graph in plain torch fp32 is
evaluated next to it and both errors are printed.  Eager launches on NaN-poisoned scratch; nothing here captures a graph."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from eval_grad_ref import BN_EPS, bn_eval, forward64_eval, routed_pool, routed_relu, shifted_running_stats
from helpers import FUSED_ADAM_BETAS, adam64, forward64, max_rel_rows, routing_taps, snapshot
from poison import poisoned_scratch  # noqa: F401
from step_factory import class_labels, grouped, make_finetune_step, points, step_opt
from synth_tree import write_tree
from test_gpu_finetune import ADAM_TOL, CONFIGS, NCLS, TOL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
S = K = 64


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _randn(shape, seed, scale=1.0):
    return torch.randn(shape, device=DEV, generator=_gen(seed)) * scale


def _away(y64):
    """Running statistics away from those of the batch y64 (rows, C): (mean + 0.1 std, 1.3 var), fp32."""
    mean, var = y64.mean(0), y64.var(0, unbiased=False)
    return (mean + 0.1 * var.sqrt()).float(), (1.3 * var).float()


def _check_grads(tag, mine, g64, g32):
    """Every gradient of `mine` against fp64: ||mine - g64|| / max(||g64||, 1e-2 gmax) <= TOL (the rule of
    tests/test_gpu_finetune.py); the plain-fp32 twin's error by the same measure is printed beside it."""
    assert set(mine) == set(g64), (tag, sorted(set(mine) ^ set(g64)))
    gmax = max(float(g64[n].norm()) for n in mine)
    worst, worst32, bad = 0.0, 0.0, []
    for n, m in mine.items():
        r = g64[n].reshape(m.shape)
        den = max(float(r.norm()), 1e-2 * gmax)
        err = float((m.double() - r).norm()) / den
        e32 = float((g32[n].double().reshape(m.shape) - r).norm()) / den
        worst, worst32 = max(worst, err), max(worst32, e32)
        if not err <= TOL:
            bad.append((n, err, e32))
    print("[%s] gradients: mine-vs-fp64 %.2e   torch-fp32-vs-fp64 %.2e" % (tag, worst, worst32))
    assert not bad, (tag, bad)


def _ties(tag, ties):
    worst = max([v for n, v in ties.items() if not n.endswith("_flips")] + [0.0])
    assert worst < 1e-5, (tag, ties)


def _bn_module(C, seed, y64):
    """A BatchNorm holder with gamma of both signs, a non-zero beta and running statistics away from the batch's."""
    from facl_amd.cn3d_model_conbag import _BatchNormState
    bn = _BatchNormState(C).to(DEV)
    with torch.no_grad():
        bn.weight.copy_(1.0 + 0.6 * torch.rand(C, device=DEV, generator=_gen(seed)))
        bn.weight[::5] *= -1.0
        bn.bias.copy_(_randn(C, seed + 1, 0.2))
        rm, rv = _away(y64)
        bn.running_mean.copy_(rm)
        bn.running_var.copy_(rv)
    bn.steps = 3
    return bn


def _affine(cout, cin, seed):
    from facl_amd.cn3d_model_conbag import _Affine
    a = _Affine((cout, cin), cin).to(DEV)
    with torch.no_grad():
        a.weight.copy_(_randn((cout, cin), seed, 1.0 / np.sqrt(cin)))
        a.bias.copy_(_randn(cout, seed + 1, 0.1))
    return a


def _bn_untouched(bn, before):
    rm, rv, steps = before
    assert torch.equal(bn.running_mean, rm) and torch.equal(bn.running_var, rv) and bn.steps == steps


def _bn_state(bn):
    return bn.running_mean.clone(), bn.running_var.clone(), bn.steps


def _leaf(t, dtype):
    return t.detach().to(dtype).requires_grad_(True)


# ---- 1. every site alone -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_centers", [True, False])
def test_linear_bn_relu_site(with_centers):
    """192 rows, 67 -> 128 columns (the centroid xyz as the first three) and 64 -> 128."""
    from facl_amd import tail
    R, Cin, C = 192, 64, 128
    h = _randn((R, Cin), 1).requires_grad_(True)
    centers = (_randn((R, 3), 2, 0.3)) if with_centers else None
    lin = _affine(C, Cin + (3 if with_centers else 0), 3)
    full = h.detach() if centers is None else torch.cat((centers, h.detach()), 1)
    bn = _bn_module(C, 5, full.double() @ lin.weight.double().t() + lin.bias.double())
    up = _randn((R, C), 7)
    kept = _bn_state(bn)
    with routing_taps() as taps:
        a = tail.linear_bn_relu(h, lin, bn, False, centers=centers)
    (a * up).sum().backward()
    _bn_untouched(bn, kept)
    mine = {"h": h.grad, "W": lin.weight.grad, "b": lin.bias.grad, "gamma": bn.weight.grad, "beta": bn.bias.grad}
    mask = taps["relu_t1" if with_centers else "relu_t2"]

    def ref(dtype):
        q = {"h": _leaf(h, dtype), "W": _leaf(lin.weight, dtype), "b": _leaf(lin.bias, dtype), "gamma": _leaf(bn.weight, dtype),
             "beta": _leaf(bn.bias, dtype)}
        x = q["h"] if centers is None else torch.cat((centers.to(dtype), q["h"]), 1)
        ties = {}
        z = bn_eval(x @ q["W"].t() + q["b"], q["gamma"], q["beta"], bn.running_mean.to(dtype), bn.running_var.to(dtype))
        out = routed_relu(z, mask, ties, "relu")
        (out * up.to(dtype)).sum().backward()
        return out.detach(), {k: v.grad for k, v in q.items()}, ties
    a64, g64, ties = ref(torch.float64)
    _, g32, _ = ref(torch.float32)
    _ties("linear_bn_relu", ties)
    assert max_rel_rows(a.detach().cpu().numpy(), a64.cpu().numpy()) < TOL
    assert float(g64["b"].abs().max()) > 0
    _check_grads("linear_bn_relu centers=%s" % with_centers, mine, g64, g32)


def _segmax_smallest_fused_rows(C):
    """The fused GEMM + max kernel (facl_gemm_fwd_segmax) lives in the 128x128 tiles, which are chosen when they alone fill the
    chip: ceil(C / 128) * ceil(R / 128) >= 256 (csrc/gemm.hip: choose_tile; FACL_E_CONFIG below).  The smallest such R that
    is a multiple of 64."""
    row_tiles = -(-256 // (-(-C // 128)))
    return 64 * -(-(128 * (row_tiles - 1) + 1) // 64)


@pytest.mark.parametrize("S_,fused", [(8, False), (64, True)])
def test_linear_bn_segmax_site(S_, fused):
    """S = 8: the row pass (facl_rows_segmax).  S = 64 at the smallest row count the fused GEMM accepts (one cloud fewer gets
    FACL_E_CONFIG and would take the row pass)."""
    from facl_amd import _lib, tail
    Cin, C = 64, 1024 if fused else 128
    R = _segmax_smallest_fused_rows(C) if fused else 5 * S_
    M = R // S_
    h = _randn((R, Cin), 11).requires_grad_(True)
    lin = _affine(C, Cin, 12)
    bn = _bn_module(C, 14, h.detach().double() @ lin.weight.double().t() + lin.bias.double())
    if fused:
        assert R == 4032
        lib = _lib.load_library()
        from facl_amd.sa_mlp import _Workspace
        for rows, want in ((R - 64, -4), (R, 0)):
            y = torch.empty((rows, C), device=DEV)
            ym, ag = torch.empty((rows // 64, C), device=DEV), torch.empty((rows // 64, C), dtype=torch.int32, device=DEV)
            rc = lib.facl_gemm_fwd_segmax(h.data_ptr(), rows, Cin, lin.weight.data_ptr(), Cin, C, lin.bias.data_ptr(),
                                          bn.weight.data_ptr(), y.data_ptr(), None, ym.data_ptr(), ag.data_ptr(),
                                          _Workspace.get(h.device).data_ptr(), _lib.stream())
            assert rc == want, (rows, rc)
    up = _randn((M, C), 16)
    kept = _bn_state(bn)
    with routing_taps() as taps:
        xpre = tail.linear_bn_relu_segmax(h, lin, bn, False, S_)
    (xpre * up).sum().backward()
    _bn_untouched(bn, kept)
    mine = {"h": h.grad, "W": lin.weight.grad, "b": lin.bias.grad, "gamma": bn.weight.grad, "beta": bn.bias.grad}

    def ref(dtype):
        q = {"h": _leaf(h, dtype), "W": _leaf(lin.weight, dtype), "b": _leaf(lin.bias, dtype), "gamma": _leaf(bn.weight, dtype),
             "beta": _leaf(bn.bias, dtype)}
        ties = {}
        z = bn_eval(q["h"] @ q["W"].t() + q["b"], q["gamma"], q["beta"], bn.running_mean.to(dtype), bn.running_var.to(dtype))
        out = routed_relu(routed_pool(z.view(M, S_, C), taps["seg_arg"], ties, "seg"), taps["relu_t3"], ties, "relu")
        (out * up.to(dtype)).sum().backward()
        return out.detach(), {k: v.grad for k, v in q.items()}, ties
    x64, g64, ties = ref(torch.float64)
    _, g32, _ = ref(torch.float32)
    _ties("segmax", ties)
    assert max_rel_rows(xpre.detach().cpu().numpy(), x64.cpu().numpy()) < TOL
    _check_grads("linear_bn_segmax S=%d" % S_, mine, g64, g32)


@pytest.mark.parametrize("G,B", [(2, 4), (5, 3)])
def test_fc_head_site(G, B):
    from facl_amd import tail
    Cin, C, dim = 256, 128, 64
    x_pre = _randn((G * B, Cin), 21).abs().requires_grad_(True)
    lin1, lin2 = _affine(C, Cin, 22), _affine(dim, C, 24)
    bn = _bn_module(C, 26, x_pre.detach().double() @ lin1.weight.double().t() + lin1.bias.double())
    up = _randn((G * B + B, dim), 28)
    kept = _bn_state(bn)
    with routing_taps() as taps:
        out = tail.fc_head(x_pre, G, lin1, bn, lin2, False)
    (out * up).sum().backward()
    _bn_untouched(bn, kept)
    mine = {"x_pre": x_pre.grad, "W1": lin1.weight.grad, "b1": lin1.bias.grad, "gamma": bn.weight.grad, "beta": bn.bias.grad,
            "W2": lin2.weight.grad, "b2": lin2.bias.grad}

    def ref(dtype):
        q = {"x_pre": _leaf(x_pre, dtype), "W1": _leaf(lin1.weight, dtype), "b1": _leaf(lin1.bias, dtype),
             "gamma": _leaf(bn.weight, dtype), "beta": _leaf(bn.bias, dtype), "W2": _leaf(lin2.weight, dtype), "b2": _leaf(lin2.bias, dtype)}
        ties = {}
        xg = routed_pool(q["x_pre"].view(G, B, Cin).transpose(0, 1), taps["view_arg"], ties, "view")
        st = torch.cat((q["x_pre"], xg), 0)
        z = bn_eval(st @ q["W1"].t() + q["b1"], q["gamma"], q["beta"], bn.running_mean.to(dtype), bn.running_var.to(dtype))
        o = routed_relu(z, taps["relu_fc"], ties, "relu_fc") @ q["W2"].t() + q["b2"]
        (o * up.to(dtype)).sum().backward()
        return o.detach(), {k: v.grad for k, v in q.items()}, ties
    o64, g64, ties = ref(torch.float64)
    _, g32, _ = ref(torch.float32)
    _ties("fc_head", ties)
    assert max_rel_rows(out.detach().cpu().numpy(), o64.cpu().numpy()) < TOL
    assert float(g64["b1"].abs().max()) > 0
    _check_grads("fc_head G=%d B=%d" % (G, B), mine, g64, g32)


_SA_KEYS = {"W1": "net3DV_1.0.weight", "b1": "net3DV_1.0.bias", "g1": "net3DV_1.1.weight", "be1": "net3DV_1.1.bias",
            "W2": "net3DV_1.3.weight", "b2": "net3DV_1.3.bias", "g2": "net3DV_1.4.weight", "be2": "net3DV_1.4.bias",
            "W3": "net3DV_1.6.weight", "b3": "net3DV_1.6.bias", "g3": "net3DV_1.7.weight", "be3": "net3DV_1.7.bias"}


def _sa_setup(D, K_, groups, seed, neg):
    """The SA block's parameters (formula weights), rows of `groups` groups of K_ neighbours, and running statistics away from
    the batch's own, layer by layer from a train-mode fp64 pass."""
    from oracle.weights import formula_state_dict
    sd = formula_state_dict(D, neg_gamma=neg)
    p = {k: torch.as_tensor(sd[v]).to(DEV).float().contiguous() for k, v in _SA_KEYS.items()}
    x_rows = ((torch.rand(groups * K_, D, device=DEV, generator=_gen(seed)) - 0.5) * 0.8).contiguous()
    h, buffers = x_rows.double(), {}
    for i in (1, 2, 3):
        W = p["W%d" % i].double()
        y = h @ W.reshape(W.shape[0], -1).t() + p["b%d" % i].double()
        mean, var = y.mean(0), y.var(0, unbiased=False)
        h = torch.relu((y - mean) / torch.sqrt(var + BN_EPS) * p["g%d" % i].double() + p["be%d" % i].double())
        buffers["rm%d" % i], buffers["rv%d" % i] = _away(y)
    return p, x_rows, buffers


def _sa_reference(p, buffers, x_rows, K_, up, taps, dtype):
    q = {k: _leaf(v, dtype) for k, v in p.items()}
    ties, h = {}, x_rows.to(dtype)
    for i in (1, 2, 3):
        W = q["W%d" % i]
        z = bn_eval(h @ W.reshape(W.shape[0], -1).t() + q["b%d" % i], q["g%d" % i], q["be%d" % i],
                    buffers["rm%d" % i].to(dtype), buffers["rv%d" % i].to(dtype))
        h = routed_relu(z, taps.get("relu_sa%d" % i), ties, "relu_sa%d" % i) if i < 3 else z
    pooled = routed_relu(routed_pool(h.view(-1, K_, 256), taps.get("sa_arg"), ties, "sa"), taps.get("relu_sa3"), ties, "relu_sa3")
    (pooled * up.to(dtype)).sum().backward()
    return pooled.detach(), {k: v.grad for k, v in q.items()}, ties


@pytest.mark.parametrize("D,K_,groups,neg", [(3, 64, 7, True), (4, 64, 7, False), (8, 64, 7, False), (4, 128, 5, False),
                                               (4, 8, 21, False)])
def test_sa_block_site(D, K_, groups, neg):
    """7 units (ragged against every tile of the heavy passes) at D = 3, 4, 8; K = 128 (two units per group) and K = 8 (eight
    groups replicated into one unit) at D = 4.  All twelve gradients, b1 / b2 / b3 among them.  K = 64 is routed through the
    kernel's decisions; the other K have no per-group taps and compare against the plain fp64 graph."""
    from facl_amd import sa_mlp
    p, x_rows, buffers = _sa_setup(D, K_, groups, 30 + D + K_, neg)
    params = {k: p[k].clone().requires_grad_(True) for k in sa_mlp._PARAM_ORDER}
    kept = {k: v.clone() for k, v in buffers.items()}
    state = {"buffers": buffers, "training": False, "K": K_}
    with routing_taps() as taps:
        pooled = sa_mlp.SAMLPFunction.apply(x_rows, state, *[params[k] for k in sa_mlp._PARAM_ORDER])
    assert pooled.shape == (groups, 256) and "y2f" in pooled.grad_fn.c            # the storing passes ran
    up = _randn(pooled.shape, 40)
    (pooled * up).sum().backward()
    for k in kept:
        assert torch.equal(kept[k], buffers[k]), k
    if K_ != 64:
        taps = {}
    mine = {k: v.grad for k, v in params.items()}
    p64, g64, ties = _sa_reference(p, buffers, x_rows, K_, up, taps, torch.float64)
    _, g32, _ = _sa_reference(p, buffers, x_rows, K_, up, taps, torch.float32)
    _ties("sa", ties)
    assert max_rel_rows(pooled.detach().cpu().numpy(), p64.cpu().numpy()) < TOL
    for b in ("b1", "b2", "b3"):
        assert float(g64[b].abs().max()) > 0
    _check_grads("sa D=%d K=%d" % (D, K_), mine, g64, g32)


# ---- 4. eval forward with grad enabled (storing passes) vs under no_grad (the one-kernel path) ---------------------------------
@pytest.mark.parametrize("D,K_,groups", [(4, 64, 7), (3, 128, 5), (4, 16, 12)])
def test_eval_forward_with_grad_vs_no_grad(D, K_, groups):
    """The bound of test_sa_eval_one_kernel_vs_training_kernels_and_fp64 for the two paths: each within 2e-5 of fp64, the one
    kernel within 3x the storing passes' error + 2e-6.  Under no_grad the Function still gives the one-kernel result, bit for bit."""
    from facl_amd import sa_mlp
    p, x_rows, buffers = _sa_setup(D, K_, groups, 50 + D + K_, False)
    state = {"buffers": buffers, "training": False, "K": K_}
    params = [p[k].clone().requires_grad_(True) for k in sa_mlp._PARAM_ORDER]
    stored = sa_mlp.SAMLPFunction.apply(x_rows, dict(state), *params)
    with torch.no_grad():
        fused = sa_mlp.SAMLPFunction.apply(x_rows, dict(state), *params)
    direct, ctx = sa_mlp.sa_mlp_forward(x_rows, {**p, **buffers}, False, K=K_)
    assert stored.grad_fn is not None and "y2f" in stored.grad_fn.c and "y2f" not in ctx
    assert torch.equal(fused, direct)
    ref, _, _ = _sa_reference(p, buffers, x_rows, K_, torch.zeros_like(stored), {}, torch.float64)
    e_f, e_s = max_rel_rows(fused.cpu().numpy(), ref.cpu().numpy()), max_rel_rows(stored.detach().cpu().numpy(), ref.cpu().numpy())
    print("one kernel vs fp64 %.2e   storing passes (grad enabled) vs fp64 %.2e" % (e_f, e_s))
    assert e_s < 2e-5 and e_f < 2e-5 and e_f < 3 * e_s + 2e-6


# ---- 2 + 3. the whole model in eval(), one frozen FineTuneStep ------------------------------------------------------------------
def _reference_eval(c, sd, pts, labels, routing, dtype):
    B, G = c["B"], c["G"]
    x_rows, centers = grouped(c, pts)
    x, xg, _, q, ties = forward64_eval(x_rows, centers, sd, G, S, K, DEV, routing=routing, grad=True, dtype=dtype)
    feat = torch.cat((x, xg), dim=0).view(G + 1, B, 512).permute(1, 0, 2).reshape(B, (G + 1) * 512)
    logits = F.normalize(feat, p=2, dim=1) @ q["head.fc.weight"].t() + q["head.fc.bias"]
    loss = F.cross_entropy(logits, labels.long())
    loss.backward()
    return {"logits": logits.detach(), "loss": float(loss.detach()), "ties": ties,
            "g": {k: v.grad.detach() for k, v in q.items() if v.grad is not None},
            "hits": int((logits.detach().argmax(dim=1) == labels.long()).sum())}


@pytest.mark.parametrize("cfg", ["ragged", "view_major"])
def test_frozen_step_vs_fp64(cfg):
    """FineTuneNet in eval() through FineTuneStep(freeze_bn=True): logits, loss and the gradient of every parameter torch gives
    one (the seven pre-BN biases included) against fp64; running statistics and counters bit-identical afterwards; FusedAdam
    against fp64 Adam on the kernel's gradients; a second step from the restored state bit-identical to the first."""
    from facl_amd.finetune import FineTuneStep
    c = CONFIGS[cfg]
    net, optim, _ = make_finetune_step(c, NCLS)
    pts, labels = points(c, 100), class_labels(c, 1, NCLS)
    x_rows, centers = grouped(c, pts)
    sd0 = {k: v.detach().cpu() for k, v in net.state_dict().items()}
    with torch.no_grad():
        stats = forward64(x_rows, centers, sd0, c["G"], S, K, DEV)[2]
    net.load_state_dict(shifted_running_stats(sd0, stats))
    del stats, x_rows, centers
    step = FineTuneStep(net, optim, step_opt(c["D"], c["B"], c["N"]), c["G"], freeze_bn=True)
    step.labels.copy_(labels)
    before = snapshot(net, optim)
    with routing_taps() as routing:
        loss, logits, stats_k = step(pts)
    torch.cuda.synchronize()
    assert not net.training
    grads = {n: p.grad.detach().clone() for n, p in net.named_parameters() if p.grad is not None}
    params = {n: p.detach().clone() for n, p in net.named_parameters()}
    after = snapshot(net, optim)
    loss, logits = loss.detach().clone(), logits.detach().clone()

    # the frozen statistics: bit-identical, counters included
    for k, v in before["net"].items():
        if "running" in k or "num_batches" in k:
            assert torch.equal(v, after["net"][k]), k
    ref = _reference_eval(c, before["net"], pts, labels, routing, torch.float64)
    ref32 = _reference_eval(c, before["net"], pts, labels, routing, torch.float32)
    e_lg = max_rel_rows(logits.cpu().numpy(), ref["logits"].cpu().numpy())
    e_l = abs(float(loss) - ref["loss"]) / abs(ref["loss"])
    e_lg32 = max_rel_rows(ref32["logits"].cpu().numpy(), ref["logits"].cpu().numpy())
    print("[%s] logits %.2e (fp32 twin %.2e)  loss %.2e  stats %s" % (cfg, e_lg, e_lg32, e_l, stats_k.tolist()))
    assert e_lg < TOL and e_l < TOL, (cfg, e_lg, e_l)
    _ties(cfg, ref["ties"])
    assert len(grads) == 30 + 2 and "netR_FC.0.bias" in grads and "net3DV_1.0.bias" in grads
    _check_grads(cfg, grads, ref["g"], ref32["g"])
    assert stats_k.tolist() == [ref["hits"], 0]

    # FusedAdam on the kernel's own gradients
    ak, akf = adam64(before, grads), adam64(before, grads, FUSED_ADAM_BETAS)
    bad_adam = []
    for n, (p64, _, _) in ak.items():
        _, m64, v64 = akf[n]
        for what, got, want in (("param", params[n], p64), ("exp_avg", after["adam"][n]["exp_avg"], m64),
                                ("exp_avg_sq", after["adam"][n]["exp_avg_sq"], v64)):
            d = float((got.to(DEV).double().reshape(want.shape) - want).abs().max()) / max(float(want.abs().max()), 1e-30)
            if not d <= ADAM_TOL:
                bad_adam.append((n, what, d))
    assert not bad_adam, (cfg, bad_adam)
    assert after["step"] == 1
    for b in ("net3DV_3.3.bias", "netR_FC.0.bias"):
        assert not torch.equal(before["net"][b], after["net"][b]), b           # the pre-BN biases train

    # a second step from the restored state: bit-identical
    net.load_state_dict(before["net"])
    optim.load_state_dict(before["optim"])
    loss2, logits2, _ = step(pts)
    torch.cuda.synchronize()
    assert torch.equal(loss2.detach(), loss) and torch.equal(logits2.detach(), logits)
    for n, p in net.named_parameters():
        assert torch.equal(p.detach(), params[n]), n
        if n in grads:
            assert torch.equal(p.grad, grads[n]), n


# ---- 5. the entry ------------------------------------------------------------------------------------------------------------
def test_entry_freeze_bn(tmp_path, capsys):
    from facl_amd import finetune
    write_tree(str(tmp_path / "d"))
    common = ["--synthetic", "0", "--data_root", str(tmp_path / "d"), "--dataset", "ntu120", "--batchSize", "4",
              "--num_crop", "10", "--SAMPLE_NUM", "512", "--INPUT_FEATURE_NUM", "4", "--label_fraction", "0.5", "--num_class", "4"]
    finetune.main(common + ["--nepoch", "1", "--graph", "0", "--eval_every", "0", "--save_root_dir", str(tmp_path / "pre")])
    capsys.readouterr()
    ck = str(tmp_path / "pre" / "finetune_enc_0.pth")
    top1 = finetune.main(common + ["--nepoch", "2", "--eval_every", "1", "--save_root_dir", str(tmp_path / "ft"),
                                   "--freeze_bn", "1", "--checkpoint", ck])
    text = capsys.readouterr().out
    assert text.count("BatchNorm frozen: running statistics of %s kept; step runs eager" % ck) == 1
    assert "graph capture" not in text
    assert isinstance(top1, float) and "epoch: 1 test top1: %s" % top1 in text and "epoch: 0 test top1:" in text
    loaded = torch.load(ck, map_location="cpu", weights_only=True)
    saved = torch.load(str(tmp_path / "ft" / "finetune_enc_1.pth"), map_location="cpu", weights_only=True)
    assert loaded.keys() == saved.keys() and os.path.exists(str(tmp_path / "ft" / "finetune_fc_1.pth"))
    frozen = [k for k in loaded if "running" in k or "num_batches" in k]
    assert len(frozen) == 7 * 3
    for k in frozen:
        assert torch.equal(loaded[k], saved[k]), k
    moved = [k for k in loaded if k not in frozen and k != "mapping.weight" and not torch.equal(loaded[k], saved[k])]
    assert len(moved) == 30, sorted(set(loaded) - set(frozen) - set(moved))
