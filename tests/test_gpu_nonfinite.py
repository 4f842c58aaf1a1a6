"""A NaN or an inf in the data or in a parameter must stay loud on the GPU: the HIP path is held to what the torch fp64
reference does at every site of tests/nonfinite_sites.py (tests/test_nonfinite_cpu.py evaluates and records those reference
results on the CPU; nothing here is hard-coded).  Where the reference is non-finite the kernels' result must be; where the
reference stays finite the kernels must agree with its value.  The whole module runs on NaN-poisoned scratch."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import nonfinite_sites as NS
from helpers import max_rel_rows, rel_err
from poison import poisoned_scratch  # noqa: F401
from step_factory import step_opt

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _bad(t):
    return ~torch.isfinite(t.detach().cpu())


def _counts(name, got_bad, ref_bad):
    print("%s: non-finite %d of %d here, %d in the fp64 reference" % (name, int(got_bad.sum()), got_bad.numel(), int(ref_bad.sum())))


# ---- (a) the SA block, training mode -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", NS.SA_TRAIN_CASES, ids=NS.ids(NS.SA_TRAIN_CASES))
def test_sa_training_forward_is_non_finite_where_the_reference_is(case):
    """sa_mlp_forward(training=True) against oracle_pooled in fp64: isfinite(pooled) and isfinite of the six running buffers
    equal the reference's, element for element; elements the reference keeps finite agree with it (5e-5 per row, the bound of
    test_sa_ragged_unit_counts at these unit counts; 2e-6 on the buffers, the bound of test_sa_forward_vs_oracle)."""
    from facl_amd import sa_mlp
    from helpers import sa_params
    x, sd = NS.sa_inputs(case)
    p = sa_params(sd, DEV)
    pooled, _ = sa_mlp.sa_mlp_forward(x.to(DEV), p, True, K=case["K"], precision=case["precision"])
    torch.cuda.synchronize()
    ref = NS.sa_reference(case, True)
    got, want = pooled.cpu(), ref["pooled"]
    assert got.shape == want.shape
    gb, rb = _bad(got), _bad(want)
    _counts("pooled", gb, rb)
    wrong = []
    if not torch.equal(gb, rb):
        wrong.append(("pooled", int(gb.sum()), int(rb.sum())))
    for k, r in ref["buffers"].items():
        b = _bad(p[k])
        _counts(k, b, _bad(r))
        if not torch.equal(b, _bad(r)):
            wrong.append((k, int(b.sum()), int(_bad(r).sum())))
    assert not wrong, wrong
    cols = ~rb.any(dim=0)
    if cols.any():
        assert max_rel_rows(got[:, cols].numpy(), want[:, cols].numpy()) < 5e-5
    for k, r in ref["buffers"].items():
        fine = ~_bad(r)
        if fine.any():
            assert rel_err(p[k].cpu()[fine].numpy(), r[fine].numpy()) < 2e-6, k


# ---- (b) the SA block, eval mode ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", NS.SA_EVAL_CASES, ids=NS.ids(NS.SA_EVAL_CASES))
def test_sa_eval_forward_is_non_finite_where_the_reference_is(case):
    """sa_mlp_forward(training=False) with a NaN / +inf coordinate against oracle_pooled in fp64.
    Default fused path (csrc/sa_eval.hip): exactly the reference's groups hold a non-finite feature (the kernel poisons the whole
    group where the reference, for an inf, keeps the features whose ReLU closed: compared per group), every other group agrees
    with the reference (2e-5, the bound of test_sa_eval_one_kernel_vs_training_kernels_and_fp64).
    Opt-in paths (the unfused passes, precisions "x3" / "f16"): they have no per-group flag, the flag travels through the
    operand maximum of x into the constants of the last layer -- every output is non-finite at least wherever the reference's is.
    A SUPERSET (all groups non-finite) is accepted there: an extraction that is loud in too many rows is still loud."""
    from facl_amd import sa_mlp
    from helpers import sa_params
    x, sd = NS.sa_inputs(case)
    p = sa_params(sd, DEV)
    path = case["path"]
    prec = path if path in ("x3", "f16") else "f32"
    assert sa_mlp._EVAL_FUSED and sa_mlp._FWD_H3
    sa_mlp._EVAL_FUSED = path != "unfused"
    try:
        pooled, _ = sa_mlp.sa_mlp_forward(x.to(DEV), p, False, K=case["K"], precision=prec)
        torch.cuda.synchronize()
    finally:
        sa_mlp._EVAL_FUSED = True
    want = NS.sa_reference(case, False)["pooled"]
    got = pooled.cpu()
    gb, rb = _bad(got), _bad(want)
    _counts("pooled (%s)" % path, gb, rb)
    if path == "fused":
        assert torch.equal(gb.any(dim=1), rb.any(dim=1))
        keep = ~rb.any(dim=1)
        assert max_rel_rows(got[keep].numpy(), want[keep].numpy()) < 2e-5
    else:
        assert bool((gb | ~rb).all()), int((rb & ~gb).sum())


# ---- (c) the SA backward --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", NS.SA_BWD_CASES, ids=NS.ids(NS.SA_BWD_CASES))
def test_sa_backward_spreads_a_non_finite_upstream_gradient(case):
    """Finite forward, one NaN / +inf element of dpooled: every parameter gradient that torch fp64 autograd makes non-finite
    somewhere is non-finite here wherever autograd's is.  One direction only: the closed-form Gram assembly of
    facl_sa_bwd_final may spread the value over rows of dW3 the reference keeps finite, which is still loud.
    The conv biases in front of a train-mode BatchNorm have no gradient here by construction (None: the optimizer never touches
    them, so no value can enter them) where autograd returns a rounding-noise gradient that the value poisons; asserted as None."""
    from facl_amd import sa_mlp
    from helpers import sa_params
    x, sd = NS.sa_inputs(dict(case, site=None))
    p = sa_params(sd, DEV)
    params = [p[k].clone().requires_grad_(True) for k in sa_mlp._PARAM_ORDER]
    state = dict(training=True, K=case["K"], buffers={k: p[k] for k in NS.SA_BUFFERS})
    pooled = sa_mlp.SAMLPFunction.apply(x.to(DEV), state, *params)
    assert torch.isfinite(pooled).all()
    pooled.backward(NS.sa_bwd_upstream(case).to(DEV))
    torch.cuda.synchronize()
    ref = NS.sa_bwd_reference(case)
    missing = []
    for k, prm in zip(sa_mlp._PARAM_ORDER, params):
        rb = _bad(ref[k]).reshape(-1)
        if k in ("b1", "b2", "b3"):
            assert prm.grad is None, k
            continue
        gb = _bad(prm.grad).reshape(-1)
        _counts("d" + k, gb, rb)
        if not bool((gb | ~rb).all()):
            missing.append((k, int((rb & ~gb).sum())))
    assert not missing, missing


# ---- (d) the whole model and the losses ------------------------------------------------------------------------------------------
def _opt(c, B):
    return SimpleNamespace(temperal_num=3, knn_K=c["K"], ball_radius=0.16, ball_radius2=0.25, sample_num_level1=c["S"],
                           sample_num_level2=c["S"], INPUT_FEATURE_NUM=c["D"], Num_Class=512, batchSize=B,
                           pooling="concatenation", SAMPLE_NUM=512)


@pytest.mark.parametrize("case", NS.MODEL_CASES, ids=NS.ids(NS.MODEL_CASES))
def test_model_and_loss_are_non_finite_where_the_reference_is(case):
    """PointNet_Plus.forward(xt, yt) in training mode + the HIP contrastive losses against helpers.forward64 + oracle.loss (no
    routing), both tail paths: the loss is non-finite if and only if the reference's is (a finite one agrees to 1e-4, the
    one-step bound of the suite).  The values go in behind the grouping."""
    from facl_amd import tail as _tail
    from facl_amd.cn3d_model_conbag import PointNet_Plus
    from facl_amd.neg_queue import NegativeQueue
    from facl_amd.utils_my import contrastive_losses_stacked
    c = NS.MODEL_SHAPES[case["tail"]]
    M, S, K, G, D = c["M"], c["S"], c["K"], c["G"], c["D"]
    B = M // G
    x_rows, cen, sd, order, queue = NS.model_inputs(case)
    net = PointNet_Plus(_opt(c, B), gost=G)
    net.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
    net = net.to(DEV).train()
    widths = (256, 256, 512, 1024)
    assert _tail.net3dv3_supported(M * S, widths, S, "f32") == (case["tail"] == "rs")
    xt = x_rows.to(DEV).view(M, S, K, D).permute(0, 3, 1, 2)
    yt = cen.to(DEV).view(M, 1, S, 3).transpose(1, 3)
    x, code, x_nor, xg = net(xt, yt, 1)
    kw = {}
    if case["loss"] == "cosine":
        kw = dict(NS.COSINE_MODE)
    elif case["loss"] == "queue":
        q = NegativeQueue(NS.QUEUE_L, 512, B, DEV)
        q.buf[:NS.QUEUE_VALID].copy_(queue)
        q.state.copy_(torch.tensor([NS.QUEUE_VALID, NS.QUEUE_VALID], dtype=torch.int32))
        kw = dict(queue=q)
    _, _, loss = contrastive_losses_stacked(G, net._stacked, order, with_sum=True, **kw)
    torch.cuda.synchronize()
    loss = float(loss.detach())
    ref = NS.model_reference(case, DEV)
    print("loss %r, fp64 reference %r; non-finite x rows %d of %d (reference %d)" % (
        loss, ref["loss"], int(_bad(x).any(dim=1).sum()), M, int(_bad(ref["x"]).any(dim=1).sum())))
    assert bool(np.isfinite(loss)) == bool(np.isfinite(ref["loss"]))
    if np.isfinite(ref["loss"]):
        assert abs(loss - ref["loss"]) <= 1e-4 * abs(ref["loss"])


# ---- (e) one step, eager and graph-replayed --------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["eager", "graph"])
def test_step_returns_a_non_finite_loss_on_the_clip_that_holds_a_nan(mode):
    """ContrastiveStep on a clip that is finite on the first step and holds one NaN feature value (channel 3 of a centroid point:
    the grouping reads coordinates only, so the captured grouping is unaffected) on the second; eager, and replayed from a
    captured graph whose batch tensor is refilled between the replays.  The reference (oracle grouping + encoder + losses,
    tests/nonfinite_sites.py: step_reference) is finite on the first clip and non-finite on the second; so must the step be."""
    from facl_amd.cn3d_model_conbag import PointNet_Plus
    from facl_amd.optim import FusedAdam
    from facl_amd.train_common import ContrastiveStep, GraphedStep
    c = NS.STEP_SHAPE
    clips, sd, order = NS.step_inputs()
    opt = step_opt(c["D"], c["B"], c["N"])
    net = PointNet_Plus(opt, gost=c["G"])
    net.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
    net = net.to(DEV).train()
    optim = FusedAdam(net.parameters(), lr=3e-4, betas=(0.5, 0.999), eps=1e-6)
    step = ContrastiveStep(net, optim, opt, c["G"])
    run = step if mode == "eager" else GraphedStep(step, clips[0].to(DEV), c["G"], restore=True)
    losses = []
    for clip in clips:
        out = run(clip.to(DEV), order=order)
        torch.cuda.synchronize()
        losses.append(float(out[0]))
    refs = [NS.step_reference(k) for k in range(2)]
    print("%s: losses %r, reference (each clip at the initial weights) %r" % (mode, losses, refs))
    assert np.isfinite(refs[0]) and not np.isfinite(refs[1])
    assert np.isfinite(losses[0]) and abs(losses[0] - refs[0]) <= 1e-3 * abs(refs[0])        # smoke()'s bound on this comparison
    assert not np.isfinite(losses[1])


# ---- (f) grouping ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["facl_group", "facl_group_clips"])
@pytest.mark.parametrize("case", NS.GROUP_CASES, ids=NS.ids(NS.GROUP_CASES))
def test_grouping_with_a_non_finite_non_centroid_point(case, entry):
    """A NaN / +inf coordinate or feature of a point that is no centroid (index >= S), against oracle.grouping.group_points:
    idx equal, xt / yt equal with the NaN positions equal.  No non-finite CENTROID is ever handed to the kernel (its radix
    select assumes K real keys below +inf)."""
    from facl_amd import utils_my
    pts = NS.group_inputs(case)
    S, K, N, D = case["S"], case["K"], case["N"], case["D"]
    assert np.isfinite(pts[:, :S]).all() and K <= N - 2
    t = torch.from_numpy(pts).to(DEV)
    if entry == "facl_group_clips":
        t = t.view(2, 2, N, D).permute(1, 0, 2, 3).contiguous()        # (B, G, N, D): cloud g*B + b is clip b's view g
    xt, yt, idx = utils_my.knn_radius_group(t, S, K, NS.GROUP_R2, want_idx=True)
    torch.cuda.synchronize()
    ridx, rxt, ryt = NS.group_reference(case)
    np.testing.assert_array_equal(idx.cpu().numpy(), ridx)
    np.testing.assert_array_equal(xt.permute(0, 2, 3, 1).cpu().numpy(), rxt)          # NaN == NaN by position
    np.testing.assert_array_equal(yt.squeeze(-1).permute(0, 2, 1).cpu().numpy(), ryt)


# ---- (g) the training entry ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", ["1", "0"])
def test_training_entry_stops_on_the_batch_that_holds_a_nan(tmp_path, graph):
    """The appearance entry (D = 4) on a dataset on disk whose one clip holds a NaN in one feature value (channel 3).  The
    reference pipeline on the batch that draws the clip (oracle.views -> oracle grouping, encoder, losses) gives a non-finite
    loss; the entry must raise check_finite_loss's FloatingPointError at epoch 0 in exactly that iteration, replayed from the
    captured graph and eager, and write neither a checkpoint nor a training state."""
    import gc
    import glob
    import os
    from facl_amd import cn3d_train_apperance_GL as train
    bad, batches = NS.entry_tree(tmp_path / "d")
    ref_loss, views = NS.entry_reference(tmp_path / "d", batches)
    assert np.isfinite(views[..., :3]).all()                             # no grouping kernel sees a non-finite centroid
    assert not np.isfinite(ref_loss)
    ck = tmp_path / "ck"
    args = ["--synthetic", "0", "--data_root", str(tmp_path / "d"), "--dataset", "ntu120", "--batchSize", str(NS.ENTRY["B"]),
            "--nepoch", "1", "--num_crop", "10", "--SAMPLE_NUM", "512", "--INPUT_FEATURE_NUM", "4", "--save_root_dir", str(ck),
            "--save_state_every", "1", "--graph", graph]
    with pytest.raises(FloatingPointError, match=r"epoch 0, iteration %d$" % NS.ENTRY["iteration"]):
        train.main(args)
    torch.cuda.synchronize()
    gc.collect()                                                         # the epoch's batch iterator: its producer thread ends
    assert not glob.glob(os.path.join(str(ck), "*.pth"))          # no checkpoint, no state, whatever their names


@pytest.mark.parametrize("extra", [(), ("--resident", "1", "--view_rng", "philox")], ids=["disk", "resident"])
def test_training_entry_refuses_a_non_finite_coordinate_before_grouping(tmp_path, extra):
    """The same dataset with the NaN in a COORDINATE of the clip: the grouping kernel's selection is undefined for a non-finite
    centroid, so the loaders refuse the clip by name on the host -- the batch loader in the iteration that reads
    it, the resident ingest before the first step -- and nothing is written."""
    import gc
    import glob
    from facl_amd import cn3d_train_apperance_GL as train
    bad, _ = NS.entry_tree(tmp_path / "d", column=1)
    ck = tmp_path / "ck"
    args = ["--synthetic", "0", "--data_root", str(tmp_path / "d"), "--dataset", "ntu120", "--batchSize", str(NS.ENTRY["B"]),
            "--nepoch", "1", "--num_crop", "10", "--SAMPLE_NUM", "512", "--INPUT_FEATURE_NUM", "4", "--save_root_dir", str(ck),
            "--save_state_every", "1"] + list(extra)
    with pytest.raises(ValueError, match=r"clip %s: non-finite coordinate" % bad):
        train.main(args)
    torch.cuda.synchronize()
    gc.collect()
    assert not glob.glob(str(ck / "*.pth"))


# ---- (h) FusedAdam ---------------------------------------------------------------------------------------------------------------
GUARD, SENTINEL = 8, 12345.0                        # guard bands as in test_gpu_optim_recipe.py


@pytest.mark.parametrize("case", NS.ADAM_CASES, ids=NS.ids(NS.ADAM_CASES))
def test_fused_adam_with_a_non_finite_gradient_element(case):
    """One FusedAdam step with a NaN / +inf / -inf in one gradient element against torch.optim.Adam in fp64 (after
    clip_grad_norm_ when max_grad_norm is on): parameters and both moments have the reference's finiteness mask and, where
    finite, its values (2e-6 of the tensor's largest value: test_fused_adam_equals_torch_adam); the guard bands around every
    parameter stay untouched.  With clipping the norm and clip_coef() are what clip_grad_norm_ computes (NaN -> NaN, inf -> 0)."""
    from facl_amd.optim import FusedAdam
    ps, gs = NS.adam_inputs(case)
    bufs, params = [], []
    for p in ps:
        buf = torch.full((GUARD + p.numel() + GUARD,), SENTINEL, device=DEV)
        view = buf[GUARD:GUARD + p.numel()]
        view.copy_(p)
        bufs.append(buf)
        params.append(view.requires_grad_(True))
    opt = FusedAdam(params, betas=(0.5, 0.999), max_grad_norm=case["max_grad_norm"], **NS.ADAM_HYPER)
    for p, g in zip(params, gs):
        p.grad = g.to(DEV)
    opt.step()
    torch.cuda.synchronize()
    ref, norm = NS.adam_reference(case)
    if case["max_grad_norm"]:
        coef = min(1.0, case["max_grad_norm"] / (norm + 1e-6)) if norm == norm else float("nan")
        got_norm, got_coef = float(opt.grad_norm()), float(opt.clip_coef())
        print("norm %r (reference %r), coefficient %r (reference %r)" % (got_norm, norm, got_coef, coef))
        assert (got_norm != got_norm) if norm != norm else got_norm == norm
        assert (got_coef != got_coef) if coef != coef else got_coef == coef
    for i, (p, buf, (rp, rm, rv)) in enumerate(zip(params, bufs, ref)):
        assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + p.numel():] == SENTINEL).all()), i
        for name, got, want in (("param", p, rp), ("exp_avg", opt.state[p]["exp_avg"], rm), ("exp_avg_sq", opt.state[p]["exp_avg_sq"], rv)):
            got = got.detach().cpu().double()
            gb, rb = _bad(got), _bad(want)
            assert torch.equal(gb, rb), (i, name, int(gb.sum()), int(rb.sum()))
            fine = ~rb
            if fine.any():
                scale = float(want[fine].abs().max())
                assert float((got[fine] - want[fine]).abs().max()) <= 2e-6 * scale + 1e-30, (i, name)
