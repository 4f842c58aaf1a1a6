"""Supervised fine-tuning (facl_amd/finetune.py): one step against a torch-fp64 evaluation (encoder through helpers.forward64
with the kernel's discrete decisions pinned, then normalise -> Linear -> cross-entropy written out here), three graph replays
with changing labels / clouds / learning rate, and the entry end to end on a tiny dataset.
The whole module runs on NaN-poisoned scratch."""
import os

import pytest
import torch
import torch.nn.functional as F

from helpers import FUSED_ADAM_BETAS, PRE_BN_BIAS, adam64, forward64, max_rel_rows, routing_taps, snapshot
from poison import poisoned_scratch  # noqa: F401
from step_factory import class_labels, grouped, make_finetune_step, points
from synth_tree import write_tree

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-4              # logits / loss / gradients: the one-step bound of the suite
ADAM_TOL = 2e-6         # Adam on the kernel's own gradients
S = K = 64             # step_factory's
NCLS = 12

CONFIGS = {
    # tests/test_gpu_trajectory.py's family, shrunk: clip-major with N no power of two; view-major rows with 4 channels
    "ragged": dict(B=3, G=5, N=1000, D=3, view_major=False),
    "view_major": dict(B=4, G=2, N=512, D=4, view_major=True),
}


def _reference(c, before, pts, labels, routing, other_labels=None):
    """The supervised step in torch fp64 from the state `before`: encoder (forward64, routed through the kernel's max-pool
    and ReLU decisions), the clip-major vector [x_view0 .. x_view(G-1), x_global], F.normalize, Linear, mean cross-entropy."""
    B, G = c["B"], c["G"]
    x_rows, centers = grouped(c, pts)
    x, xg, _, q, ties = forward64(x_rows, centers, before["net"], G, S, K, DEV, routing=routing, grad=True)
    feat = torch.cat((x, xg), dim=0).view(G + 1, B, 512).permute(1, 0, 2).reshape(B, (G + 1) * 512)
    logits = F.normalize(feat, p=2, dim=1) @ q["head.fc.weight"].t() + q["head.fc.bias"]
    loss = F.cross_entropy(logits, labels.long())
    loss.backward()
    out = {"logits": logits.detach(), "loss": float(loss.detach()), "ties": ties,
           "g64": {k: v.grad.detach() for k, v in q.items() if v.grad is not None},
           "hits": int((logits.detach().argmax(dim=1) == labels.long()).sum())}
    if other_labels is not None:
        out["loss_other"] = float(F.cross_entropy(logits.detach(), other_labels.long()))
    return out


def _check_step(tag, c, before, after, pts, labels, routing, out, grads, params, other_labels=None):
    """Logits, loss, every parameter gradient (1e-4; a gradient against max(its norm, 1e-2 of the largest norm), as
    tests/test_gpu_headline.py does), the counters, and FusedAdam against fp64 Adam on the kernel's own gradients (2e-6)."""
    loss, logits, stats = out
    ref = _reference(c, before, pts, labels, routing, other_labels)
    e_lg = max_rel_rows(logits.detach().cpu().numpy(), ref["logits"].cpu().numpy())
    e_l = abs(float(loss) - ref["loss"]) / abs(ref["loss"])
    ties = max([v for n, v in ref["ties"].items() if not n.endswith("_flips")] + [0.0])
    g64 = ref["g64"]
    gmax = max(float(g64[n].norm()) for n in grads)
    e_g, bad, floored = 0.0, [], []
    for n, mine in grads.items():
        r = g64[n].reshape(mine.shape)
        if float(r.norm()) < 1e-2 * gmax:
            floored.append((n, "%.1e" % (float(r.norm()) / gmax)))
        err = float((mine.double() - r).norm()) / max(float(r.norm()), 1e-2 * gmax)
        e_g = max(e_g, err)
        if not err <= TOL:
            bad.append((n, err))
    ak, akf = adam64(before, grads), adam64(before, grads, FUSED_ADAM_BETAS)
    e_ad, bad_adam = 0.0, []
    for n, (p64, _, _) in ak.items():
        _, m64, v64 = akf[n]
        for what, got, want in (("param", params[n], p64), ("exp_avg", after["adam"][n]["exp_avg"], m64),
                                ("exp_avg_sq", after["adam"][n]["exp_avg_sq"], v64)):
            d = float((got.to(DEV).double().reshape(want.shape) - want).abs().max()) / max(float(want.abs().max()), 1e-30)
            e_ad = max(e_ad, d)
            if not d <= ADAM_TOL:
                bad_adam.append((n, what, d))
    print("[%s] logits %.2e  loss %.2e  grad %.2e  adam %.2e  ties %.1e  stats %s" % (tag, e_lg, e_l, e_g, e_ad, ties, stats.tolist()))
    print("[%s] gradients measured against the floor 1e-2 * gmax (name, norm / gmax): %s" % (tag, floored))
    assert e_lg < TOL and e_l < TOL, (tag, e_lg, e_l)
    assert ties < 1e-5, (tag, ref["ties"])
    want_grads = {k for k in g64} - PRE_BN_BIAS
    assert set(grads) == want_grads, (tag, sorted(set(grads) ^ want_grads))
    assert not bad, (tag, bad)
    assert not bad_adam, (tag, bad_adam)
    assert stats.tolist() == [ref["hits"], 0], (tag, stats.tolist(), ref["hits"])
    return ref


def _grads_params(net):
    return ({n: p.grad.detach().clone() for n, p in net.named_parameters() if p.grad is not None},
            {n: p.detach().clone() for n, p in net.named_parameters()})


@pytest.mark.parametrize("cfg", ["ragged", "view_major"])
def test_one_step_vs_fp64(cfg):
    c = CONFIGS[cfg]
    net, optim, step = make_finetune_step(c, NCLS)
    pts, labels = points(c, 100), class_labels(c, 1, NCLS)
    step.labels.copy_(labels)
    before = snapshot(net, optim)
    with routing_taps() as routing:
        out = step(pts)
    torch.cuda.synchronize()
    grads, params = _grads_params(net)
    _check_step(cfg, c, before, snapshot(net, optim), pts, labels, routing, out, grads, params)
    assert float(optim._step[0]) == 1


def test_graph_replay_follows_labels_clouds_and_lr():
    """Three replays of GraphedStep(restore=True), each with other labels and clouds, the learning rate changed at step 2:
    every replay against the fp64 step from the state the kernels left (the routing comes from an eager twin started from
    that state, whose loss must equal the replay's to the bit); the labels reach the replay."""
    from facl_amd.train_common import GraphedStep
    c = CONFIGS["ragged"]
    net_g, opt_g, step_g = make_finetune_step(c, NCLS)
    snap0 = snapshot(net_g, opt_g)
    g = GraphedStep(step_g, points(c, 99), c["G"], restore=True)
    torch.cuda.synchronize()
    after0 = snapshot(net_g, opt_g)
    for k in snap0["net"]:
        assert torch.equal(snap0["net"][k], after0["net"][k]), k                # the three warm-up steps undone
    net_t, opt_t, step_t = make_finetune_step(c, NCLS)
    sched = [(points(c, 200 + k), class_labels(c, 10 + k, NCLS), lr) for k, lr in enumerate((3e-4, 3e-4, 1e-3))]
    assert not torch.equal(sched[0][1], sched[1][1])
    for k, (pts, labels, lr) in enumerate(sched):
        opt_g.param_groups[0]["lr"] = lr
        before = snapshot(net_g, opt_g)
        step_g.labels.copy_(labels)
        out = tuple(t.detach().clone() for t in g(pts))
        torch.cuda.synchronize()
        grads, params = _grads_params(net_g)
        after = snapshot(net_g, opt_g)
        net_t.load_state_dict(before["net"])
        opt_t.load_state_dict(before["optim"])
        step_t.labels.copy_(labels)
        with routing_taps() as routing:
            out_t = step_t(pts)
        assert torch.equal(out_t[0].detach(), out[0]) and torch.equal(out_t[1].detach(), out[1]), k
        other = sched[1][1] if k == 0 else None
        ref = _check_step("graph %d" % k, c, before, after, pts, labels, routing, out, grads, params, other)
        assert after["step"] == k + 1 and after["lr"] == lr
        if k == 0:
            # the same state under step 1's labels gives another loss: the replay read step 0's labels
            # (by more than ten times the bound the loss is held to)
            assert abs(float(out[0]) - ref["loss_other"]) > 10 * TOL * abs(ref["loss"]), (float(out[0]), ref["loss_other"])


# ---- the entry on a tiny dataset (synth_tree.write_tree) ------------------------------------------------------------------------
def test_entry_end_to_end(tmp_path, capsys):
    from facl_amd import finetune
    from facl_amd.cn3d_model_conbag import PointNet_Plus
    from facl_amd.linear_classify import Final_FC
    write_tree(str(tmp_path / "d"))
    runs = []
    for tag in ("a", "b"):
        ck = tmp_path / ("ck" + tag)
        args = ["--synthetic", "0", "--data_root", str(tmp_path / "d"), "--dataset", "ntu120", "--batchSize", "4", "--nepoch", "2",
                "--num_crop", "10", "--SAMPLE_NUM", "512", "--INPUT_FEATURE_NUM", "4", "--save_root_dir", str(ck),
                "--eval_every", "1", "--label_fraction", "0.5", "--num_class", "4"]
        top1 = finetune.main(args)
        text = capsys.readouterr().out
        assert isinstance(top1, float) and 0.0 <= top1 <= 100.0
        assert "epoch: 1 test top1: %s" % top1 in text and "epoch: 0 test top1:" in text
        assert "labelled clips: 8 of 16" in text
        enc = torch.load(str(ck / "finetune_enc_1.pth"), map_location="cpu", weights_only=True)
        fc = torch.load(str(ck / "finetune_fc_1.pth"), map_location="cpu", weights_only=True)
        assert os.path.exists(str(ck / "finetune_enc_0.pth")) and os.path.exists(str(ck / "finetune_fc_0.pth"))
        runs.append((top1, enc, fc))
    top1, enc, fc = runs[0]
    opt = finetune.finetune_parser().parse_args(args)
    PointNet_Plus(opt, gost=10).load_state_dict(enc, strict=True)
    Final_FC(input_dim=512, gost=11, num_class=4).load_state_dict(fc, strict=True)
    assert int(enc["net3DV_1.1.num_batches_tracked"]) == 2 * (8 // 4)             # 8 labelled clips, B = 4, two epochs
    assert runs[1][0] == top1
    for a, b in ((enc, runs[1][1]), (fc, runs[1][2])):
        assert a.keys() == b.keys()
        for k in a:
            assert torch.equal(a[k], b[k]), k
