"""GPU tests of the momentum key encoder (--key_encoder): the averaging kernel facl_ema_apply against fp64 with guard bands,
the training step with a key encoder (eager and graph-replayed) and the training entry.  The step tests run at the `ragged`
size of test_gpu_neg_queue.py with its mode and its bound TOL.  The whole module runs on NaN-poisoned scratch."""
import os
import re

import numpy as np
import pytest
import torch

from chunk_cases import DEV, _banded, _bands_intact, _case, _ints, _ptrs
from helpers import snapshot
from poison import poisoned_scratch  # noqa: F401
from step_factory import make_contrastive_step, make_net, points

pytestmark = pytest.mark.gpu
TOL = 1e-4                           # test_gpu_neg_queue.py / test_gpu_trajectory.py: losses of one step
U = 2.0 ** -24                       # unit roundoff of fp32


# ---- 1: the kernel ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [0.0, 0.5, 0.999, 1.0])
@pytest.mark.parametrize("nt", [14, 64])
def test_ema_apply_vs_fp64_with_guard_bands(nt, m):
    """pk = m pk + (1-m) p against fp64 on the same fp32 inputs, all tensors in ONE launch.  Bound (derived, not measured):
    three roundings -- the two products and the sum -- plus the rounding of 1 - m give |pk - ref| <= 3u (m|pk| + (1-m)|p|)
    to first order; 4u with the second-order terms.  m = 0: the bits of p; m = 1: the bits pk had.  The guard bands around
    every tensor stay as they were and p is not written."""
    from facl_amd import _lib
    lib = _lib.load_library()
    gen = torch.Generator(device=DEV)
    gen.manual_seed(nt)
    case = _case(nt)
    assert len(case) == nt
    ks = [_banded(torch.randn(n, device=DEV, generator=gen), s) for n, s in case]
    ps = [_banded(torch.randn(n, device=DEV, generator=gen), s) for n, s in case]
    k_old = [d.clone() for _, d in ks]
    p_buf_old = [b.clone() for b, _ in ps]
    PK, P, N = _ptrs([d for _, d in ks]), _ptrs([d for _, d in ps]), _ints([n for n, _ in case])
    _lib.check(lib.facl_ema_apply(nt, PK, P, N, m, _lib.stream()), "facl_ema_apply")
    torch.cuda.synchronize()
    m32 = float(np.float32(m))                              # the launch constant the kernel got
    worst = 0.0
    for i, (n, s) in enumerate(case):
        buf, got = ks[i]
        assert _bands_intact(buf, s, n), (i, n, s)
        assert torch.equal(ps[i][0], p_buf_old[i]), (i, n, s)                      # p and its bands: not written
        p = ps[i][1]
        assert torch.isfinite(got).all()
        if m == 0.0:
            assert torch.equal(got.view(torch.int32), p.view(torch.int32)), (i, n, s)
        elif m == 1.0:
            assert torch.equal(got.view(torch.int32), k_old[i].view(torch.int32)), (i, n, s)
        else:
            ref = m32 * k_old[i].double() + (1.0 - m32) * p.double()
            bound = 4 * U * (m32 * k_old[i].double().abs() + (1.0 - m32) * p.double().abs())
            err = (got.double() - ref).abs()
            worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
            assert bool((err <= bound).all()), (i, n, s, float((err / bound).max()))
    print("facl_ema_apply nt=%d m=%g: max error / bound %.3f" % (nt, m, worst))


# ---- 2: the training step (helpers as in test_gpu_neg_queue.py) ------------------------------------------------------------------
RAGGED = dict(B=3, G=5, N=1000, D=3)
STEP_MODE = dict(loss_normalize=1, loss_temperature=0.1, loss_mask="exclude")
KW = dict(normalize=True, temperature=0.1, mask="exclude")


def _mapped(x_global):
    from facl_amd.utils_my import loss_rows
    return loss_rows(x_global.detach().contiguous(), KW["normalize"], KW["temperature"]).clone()


def _query_rows(net, G, B):
    """The rows a step WITHOUT a key encoder stores: x_global of the step's stacked output after the row map."""
    from facl_amd.utils_my import loss_rows
    return loss_rows(net._stacked.detach(), KW["normalize"], KW["temperature"])[G * B:].clone()


def _sd(net):
    return {k: v.detach().clone() for k, v in net.state_dict().items()}


def test_key_encoder_at_m0_is_the_plain_queue():
    """(a) Four steps with key_encoder=1, key_momentum=0 and four steps with the queue alone, from the same state, points and
    orders: losses, every entry of the model's state_dict, queue contents and (head, valid) bit-identical.  At m = 0 the copy
    equals the model at every forward and the no-grad forward makes the same launches; this also shows that the key forward
    overwrites nothing the query forward leaves for its backward."""
    c = RAGGED
    G = c["G"]
    r = np.random.RandomState(7)
    orders = [r.permutation(G) for _ in range(4)]
    res = []
    for flags in (dict(key_encoder=1, key_momentum=0.0), {}):
        net, optim, step = make_contrastive_step(c, neg_queue=6, **STEP_MODE, **flags)
        per_step = []
        for k, order in enumerate(orders):
            out = [t.detach().clone() for t in step(points(c, 100 + k), order=order)]
            torch.cuda.synchronize()
            per_step.append((out, _sd(net), step.queue.buf.clone(), step.queue.head_valid()))
            if flags:                                       # m = 0: the copy's parameters are the model's after every step
                for a, b in zip(step.key_encoder.key.parameters(), net.parameters()):
                    assert torch.equal(a, b) and not a.requires_grad
        assert (step.key_encoder is not None) == bool(flags)
        res.append(per_step)
    for k, ((out_a, sd_a, buf_a, hv_a), (out_b, sd_b, buf_b, hv_b)) in enumerate(zip(*res)):
        for a, b in zip(out_a, out_b):
            assert torch.isfinite(a).all() and torch.equal(a, b), (k, float(a), float(b))
        assert sd_a.keys() == sd_b.keys()
        for name in sd_a:
            assert torch.equal(sd_a[name], sd_b[name]), (k, name)
        assert torch.equal(buf_a, buf_b) and hv_a == hv_b == ((3 * (k + 1)) % 6, min(3 * (k + 1), 6)), k


def test_key_encoder_three_eager_steps_at_m_half():
    """(b) key_momentum = 0.5, three eager steps; see the assertions."""
    from facl_amd.utils_my import circle_contrast, global_contrast
    c = RAGGED
    B, G = c["B"], c["G"]
    r = np.random.RandomState(7)
    orders = [r.permutation(G) for _ in range(3)]
    net, optim, step = make_contrastive_step(c, neg_queue=6, key_encoder=1, key_momentum=0.5, **STEP_MODE)
    net0, optim0, step0 = make_contrastive_step(c, neg_queue=6, **STEP_MODE)        # the run without a key encoder (step 1 only)
    third = make_net(c["D"], c["G"], c["B"], c["N"]).train()
    init = _sd(net)
    k64 = [p.detach().double().clone() for p in net.parameters()]
    for k in range(3):
        pts = points(c, 100 + k)
        held = None if step.queue is None else step.queue.valid_rows().double()
        want_rows = None
        if step.key_encoder is not None:
            third.load_state_dict(step.key_encoder.state_dict(), strict=True)
        # before step 1 the key encoder does not exist yet: it starts as the model, which `third` already is
        third.train()
        xt, yt = step.group(pts)
        with torch.no_grad():
            want_rows = _mapped(third(xt, yt, 1)[3])
        loss, loss_c, loss_circle = [t.detach().clone() for t in step(pts, order=orders[k])]
        torch.cuda.synchronize()
        if k == 0:                                          # empty queue: the step without a key encoder, bit for bit
            out0 = [t.detach().clone() for t in step0(pts, order=orders[0])]
            torch.cuda.synchronize()
            for a, b in zip((loss, loss_c, loss_circle), out0):
                assert torch.equal(a, b)
            for (name, a), b in zip(net.named_parameters(), net0.parameters()):
                assert torch.equal(a, b), name
        # the key parameters follow k <- 0.5 k + 0.5 q_after_step: per step the kernel's 4u (m|k| + (1-m)|q|) <= 4u max(|k|, |q|),
        # halved by every later step: 4u (1 + 1/2 + 1/4) < 8u after three; asserted with margin at 16u
        worst = 0.0
        for i, (kp, q) in enumerate(zip(step.key_encoder.key.parameters(), net.parameters())):
            k64[i] = 0.5 * k64[i] + 0.5 * q.detach().double()
            bound = 16 * U * torch.maximum(k64[i].abs(), q.detach().double().abs())
            err = (kp.double() - k64[i]).abs()
            assert bool((err <= bound).all()), (k, i)
            worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
        # the rows the step wrote are the key encoder's, bit for bit, and from step 2 on not the query's own
        wrote = step.queue.buf[(3 * k) % 6:(3 * k) % 6 + 3]
        assert step.queue.head_valid() == ((3 * (k + 1)) % 6, min(3 * (k + 1), 6))
        assert torch.equal(wrote, want_rows), k
        own = _query_rows(net, G, B)
        diff = float((wrote - own).abs().max())
        print("step %d: key recursion error / bound %.3f; max |key rows - query rows| %.3e" % (k + 1, worst, diff))
        if k >= 1:
            assert not torch.equal(wrote, own), k
        st = net._stacked.detach().double()
        rc = float(global_contrast(G, st[G * B:], st[:G * B], None, queue=held, **KW))
        ro = float(circle_contrast(G, st[:G * B], B, order=orders[k], queue=held, **KW))
        print("step %d: loss_c %.6f (fp64 %.6f) loss_circle %.6f (fp64 %.6f)" % (k + 1, float(loss_c), rc, float(loss_circle), ro))
        assert abs(float(loss_c) - rc) < TOL * abs(rc) and abs(float(loss_circle) - ro) < TOL * abs(ro)
        assert abs(float(loss) - (rc + ro)) < TOL * abs(rc + ro)
    # the copy's BatchNorm ran in train mode on its own buffers
    ksd = step.key_encoder.state_dict()
    for name in ("net3DV_1.1.running_mean", "net3DV_3.7.running_mean", "netR_FC.1.running_mean"):
        assert not torch.equal(ksd[name], init[name]), name
    assert step.key_encoder.key.training
    assert int(ksd["net3DV_1.1.num_batches_tracked"]) == int(init["net3DV_1.1.num_batches_tracked"]) + 3
    assert int(ksd["netR_FC.1.num_batches_tracked"]) == int(init["netR_FC.1.num_batches_tracked"]) + 6     # two calls per forward


def _assert_key_equals(key_encoder, sd, steps, where):
    ksd = key_encoder.state_dict()
    assert ksd.keys() == sd.keys()
    for name in ksd:
        assert torch.equal(ksd[name], sd[name]), (where, name)
    assert [m.steps for m in key_encoder._bn_modules()] == steps, where


def test_key_encoder_graph_replay():
    """(c) GraphedStep(restore=True) with key_momentum = 0.9: after construction the key encoder equals the model and the
    queue is empty; four replayed steps against eager steps of a twin restored from the same state are bit-identical in losses,
    model state, key-encoder state (parameters, buffers, steps), queue contents and (head, valid)."""
    from facl_amd.train_common import GraphedStep
    c = RAGGED
    G = c["G"]
    r = np.random.RandomState(7)
    orders = [r.permutation(G) for _ in range(4)]
    flags = dict(neg_queue=6, key_encoder=1, key_momentum=0.9, **STEP_MODE)
    net_g, opt_g, step_g = make_contrastive_step(c, **flags)
    g = GraphedStep(step_g, points(c, 99), G, restore=True)
    assert step_g.queue is not None and step_g.queue.head_valid() == (0, 0) and int((step_g.queue.buf != 0).sum()) == 0
    assert step_g.key_encoder is not None
    _assert_key_equals(step_g.key_encoder, _sd(net_g), [m.steps for m in net_g.modules() if hasattr(m, "count_batch")], "start")
    net_t, opt_t, step_t = make_contrastive_step(c, **flags)
    for k, order in enumerate(orders):
        pts = points(c, 100 + k)
        before = snapshot(net_g, opt_g)
        qsnap, ksnap = step_g.queue.snapshot(), step_g.key_encoder.snapshot()
        out_g = [t.detach().clone() for t in g(pts, order=order)]
        net_t.load_state_dict(before["net"])
        opt_t.load_state_dict(before["optim"])
        if step_t.queue is not None:
            step_t.queue.restore(qsnap)
        if step_t.key_encoder is not None:                  # k = 0: the twin creates its copy from the model it just loaded
            step_t.key_encoder.restore(ksnap)
        out_t = [t.detach().clone() for t in step_t(pts, order=order)]
        torch.cuda.synchronize()
        for a, b in zip(out_g, out_t):
            assert torch.isfinite(a).all() and torch.equal(a, b), (k, float(a), float(b))
        sd_g, sd_t = net_g.state_dict(), net_t.state_dict()
        for name in sd_g:
            assert torch.equal(sd_g[name], sd_t[name]), (k, name)
        _assert_key_equals(step_g.key_encoder, _sd(step_t.key_encoder.key), [m.steps for m in step_t.key_encoder._bn_modules()], k)
        assert not torch.equal(step_g.key_encoder.key.net3DV_3[6].weight, net_g.net3DV_3[6].weight), k     # m = 0.9: it lags
        assert torch.equal(step_g.queue.buf, step_t.queue.buf), k
        assert step_g.queue.head_valid() == step_t.queue.head_valid() == ((3 * (k + 1)) % 6, min(3 * (k + 1), 6)), k


# ---- 3: the training entry ----------------------------------------------------------------------------------------------------------
def test_train_entry_with_key_encoder(tmp_path, capsys):
    """(d)"""
    from facl_amd import cn3d_train_motion_GL as train
    from facl_amd.cn3d_model_conbag import PointNet_Plus
    from facl_amd.train_common import build_parser
    args = ["--synthetic", "1", "--nepoch", "1", "--steps_per_epoch", "3", "--batchSize", "4", "--num_crop", "4", "--SAMPLE_NUM", "512",
            "--neg_queue", "8", "--key_encoder", "1", "--key_momentum", "0.5", "--save_root_dir", str(tmp_path)]
    train.main(args)
    out = capsys.readouterr().out
    m = re.search(r"--loss: (\S+)", out)
    assert m, out
    assert np.isfinite(float(m.group(1)))
    q_path, k_path = os.path.join(str(tmp_path), "corr_GL_0.pth"), os.path.join(str(tmp_path), "corr_GL_0_key.pth")
    assert os.path.exists(q_path) and os.path.exists(k_path)
    q_sd, k_sd = torch.load(q_path, map_location="cpu"), torch.load(k_path, map_location="cpu")
    fresh = PointNet_Plus(build_parser('0').parse_args(args), gost=4)
    fresh.load_state_dict(k_sd, strict=True)
    assert q_sd.keys() == k_sd.keys()
    assert any(not torch.equal(q_sd[name], k_sd[name]) for name, _ in fresh.named_parameters())
    assert all(torch.isfinite(v).all() for v in k_sd.values())
    with pytest.raises(RuntimeError, match="neg_queue"):
        train.main(["--synthetic", "1", "--nepoch", "1", "--batchSize", "4", "--key_encoder", "1"])
