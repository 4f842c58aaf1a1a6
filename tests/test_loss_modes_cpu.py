"""Loss modes of the global / circle losses (cosine similarity, temperature, negatives-only mask), host side: the fp64
closed forms of facl_amd.utils_my against materialised logits through F.cross_entropy, the flags and their refusals."""
import argparse
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

G, B, C = 4, 3, 16
MODES = list(itertools.product((False, True), (1.0, 0.07), ("zero", "exclude")))


def _rows(x, normalize, tau):
    s = float(np.float32(1.0 / np.sqrt(tau)))
    if normalize:
        x = x / x.norm(dim=1, keepdim=True).clamp_min(1e-12)
    return x * s


def _negatives(sim_rows, clip, Bk, mask):
    """sim_rows (A, G*Bk) of ONE clip -> its shared negative set: same-clip columns zeroed in place, or physically removed."""
    same = (torch.arange(sim_rows.shape[1]) % Bk) == clip
    if mask == "zero":
        return torch.where(same[None, :], torch.zeros((), dtype=sim_rows.dtype), sim_rows).reshape(-1)
    return sim_rows[:, ~same].reshape(-1)


def _materialised(xg, x, keys, order, off, normalize, tau, mask):
    """(loss_c, loss_circle) the long way: per anchor slot the logits [positive | negatives of the clip], label 0,
    F.cross_entropy with mean over the B clips, summed over the slots."""
    xg, x, keys = _rows(xg, normalize, tau), _rows(x, normalize, tau), _rows(keys, normalize, tau)
    Bk = keys.shape[0] // G
    xv = x.view(G, B, C)
    label = torch.zeros(1, dtype=torch.long)
    loss_c = torch.zeros((), dtype=x.dtype)
    loss_o = torch.zeros((), dtype=x.dtype)
    for n in range(B):
        neg_g = _negatives((xg[n:n + 1] @ keys.t()), n + off, Bk, mask)
        for g in range(G):
            pos = (xg[n] * xv[g, n]).sum().reshape(1)
            loss_c = loss_c + F.cross_entropy(torch.cat((pos, neg_g))[None, :], label) / B
        anchors = torch.stack([xv[order[i], n] for i in range(G - 1)])
        neg_o = _negatives(anchors @ keys.t(), n + off, Bk, mask)
        for i in range(G - 1):
            pos = (xv[order[i], n] * xv[order[i + 1], n]).sum().reshape(1)
            loss_o = loss_o + F.cross_entropy(torch.cat((pos, neg_o))[None, :], label) / B
    return loss_c, loss_o


@pytest.mark.parametrize("world", [1, 2])
@pytest.mark.parametrize("normalize,tau,mask", MODES)
def test_closed_forms_vs_materialised_logits_fp64(normalize, tau, mask, world):
    from facl_amd.utils_my import circle_contrast, global_contrast
    torch.manual_seed(11)
    Bk, off = B * world, B * (world - 1)
    keys3 = torch.randn(G, Bk, C, dtype=torch.float64) * 1.5
    x = keys3[:, off:off + B].reshape(G * B, C).clone()
    keys = keys3.reshape(G * Bk, C)
    xg = torch.randn(B, C, dtype=torch.float64) * 1.5
    order = np.random.RandomState(3).permutation(G)
    kw = dict(normalize=normalize, temperature=tau, mask=mask)
    x_keys = keys if world > 1 else None
    lc = global_contrast(G, xg, x, None, x_keys=x_keys, clip_offset=off, **kw)
    lo = circle_contrast(G, x, B, order=order, x_keys=x_keys, clip_offset=off, **kw)
    rc, ro = _materialised(xg, x, keys, order, off, normalize, tau, mask)
    assert abs(float(lc) - float(rc)) <= 1e-12 * abs(float(rc))
    assert abs(float(lo) - float(ro)) <= 1e-12 * abs(float(ro))


def test_defaults_are_the_reference_loss():
    """Explicit defaults change nothing: the same bits as the call without the keywords."""
    from facl_amd.utils_my import circle_contrast, global_contrast
    torch.manual_seed(2)
    x, xg = torch.randn(G * B, C, dtype=torch.float64), torch.randn(B, C, dtype=torch.float64)
    order = np.arange(G)
    kw = dict(normalize=False, temperature=1.0, mask="zero")
    assert torch.equal(global_contrast(G, xg, x, None), global_contrast(G, xg, x, None, **kw))
    assert torch.equal(circle_contrast(G, x, B, order=order), circle_contrast(G, x, B, order=order, **kw))


def test_closed_forms_refuse_bad_modes():
    from facl_amd.utils_my import circle_contrast, global_contrast
    x, xg = torch.randn(G * 1, C), torch.randn(1, C)
    for tau in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="temperature"):
            global_contrast(G, xg, x, None, temperature=tau)
    with pytest.raises(ValueError, match="mask"):
        circle_contrast(G, x, 1, order=np.arange(G), mask="drop")
    with pytest.raises(ValueError, match="negative"):
        global_contrast(G, xg, x, None, mask="exclude")                   # one key clip


def test_parser_defaults_and_flag_refusals():
    from facl_amd.train_common import build_parser, check_loss_flags
    p = build_parser('0')
    opt = p.parse_args([])
    assert (opt.loss_normalize, opt.loss_temperature, opt.loss_mask) == (0, 1.0, 'zero')
    check_loss_flags(opt, world=1)
    check_loss_flags(p.parse_args(["--loss_normalize", "1", "--loss_temperature", "0.07", "--loss_mask", "exclude"]), world=1)
    for tau in ("0", "-0.5", "nan", "inf"):
        with pytest.raises(RuntimeError, match="temperature"):
            check_loss_flags(p.parse_args(["--loss_temperature", tau]), world=1)
    one = p.parse_args(["--loss_mask", "exclude", "--batchSize", "1"])
    with pytest.raises(RuntimeError, match="negative"):
        check_loss_flags(one, world=1)
    check_loss_flags(one, world=2)                                         # two ranks of one clip each: a negative exists
    with pytest.raises(SystemExit):
        p.parse_args(["--loss_mask", "drop"])


def test_training_entry_refuses_before_the_device(monkeypatch):
    from facl_amd import cn3d_train_motion_GL
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(RuntimeError, match="temperature"):
        cn3d_train_motion_GL.main(["--synthetic", "1", "--nepoch", "1", "--loss_temperature", "0"])


def test_finetune_refuses_non_default_loss_flags():
    from facl_amd import finetune
    p = finetune.finetune_parser()
    finetune.check_finetune_flags(p.parse_args([]), world=1)
    for bad in (["--loss_normalize", "1"], ["--loss_temperature", "0.1"], ["--loss_mask", "exclude"]):
        with pytest.raises(RuntimeError, match="contrastive loss"):
            finetune.check_finetune_flags(p.parse_args(bad), world=1)


def test_step_from_a_namespace_without_the_flags_holds_the_defaults():
    from facl_amd.train_common import ContrastiveStep
    net = torch.nn.Linear(2, 2)
    step = ContrastiveStep(net, None, argparse.Namespace(SAMPLE_NUM=512), 4)
    assert step.loss_mode == dict(normalize=False, temperature=1.0, mask="zero")
    opt = argparse.Namespace(SAMPLE_NUM=512, loss_normalize=1, loss_temperature=0.2, loss_mask="exclude")
    assert ContrastiveStep(net, None, opt, 4).loss_mode == dict(normalize=True, temperature=0.2, mask="exclude")
