"""Frozen-BatchNorm fine-tuning, the parts that need no GPU: the fp64 helper of the GPU tests (tests/eval_grad_ref.py) against
torch.nn modules in .eval() under autograd, and the --freeze_bn flag checks of facl_amd.finetune."""
import numpy as np
import pytest
import torch
import torch.nn as nn

from eval_grad_ref import BN_KEYS, bn_eval, forward64_eval

WIDTHS_1, WIDTHS_3, FC = (64, 64, 256), (256, 512, 1024), (1024, 512)


def _stack(cin, widths, pool=None):
    mods = []
    for c in widths:
        mods += [nn.Conv2d(cin, c, kernel_size=(1, 1)), nn.BatchNorm2d(c), nn.ReLU()]
        cin = c
    if pool is not None:
        mods.append(nn.MaxPool2d(pool, stride=1))
    return nn.Sequential(*mods)


def _random_state(nets, seed):
    """Random parameters AND running statistics (away from 0 / 1) for the modules; returns the 52-key-style state dict."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for prefix, net in nets.items():
        for k, v in net.state_dict().items():
            if k.endswith("num_batches_tracked"):
                continue
            if k.endswith("running_var"):
                t = torch.rand(v.shape, generator=g, dtype=torch.float64) + 0.5
            elif k.endswith("running_mean"):
                t = torch.randn(v.shape, generator=g, dtype=torch.float64) * 0.3
            elif k.endswith("weight") and v.dim() == 1:                        # gamma: both signs
                t = torch.randn(v.shape, generator=g, dtype=torch.float64)
            else:
                fan = v[0].numel() if v.dim() > 1 else 16
                t = torch.randn(v.shape, generator=g, dtype=torch.float64) / np.sqrt(fan)
            sd["%s.%s" % (prefix, k)] = t
        net.load_state_dict({k[len(prefix) + 1:]: v for k, v in sd.items() if k.startswith(prefix + ".")}, strict=False)
    return sd


@pytest.mark.parametrize("D", [3, 4])
def test_helper_equals_torch_modules_in_eval(D):
    M, S, K, G = 4, 3, 5, 2                                                    # B = 2 clips, 2 views, 3 centroids of 5 neighbours
    torch.manual_seed(0)
    nets = {"net3DV_1": _stack(D, WIDTHS_1, (1, K)).double(), "net3DV_3": _stack(3 + WIDTHS_1[2], WIDTHS_3).double(),
            "netR_FC": nn.Sequential(nn.Linear(WIDTHS_3[2], FC[0]), nn.BatchNorm1d(FC[0]), nn.ReLU(), nn.Linear(FC[0], FC[1])).double()}
    sd = _random_state(nets, 7 + D)
    for net in nets.values():
        net.eval()
    g = torch.Generator().manual_seed(3)
    xt = torch.rand(M, D, S, K, generator=g, dtype=torch.float64) - 0.5
    yt = torch.rand(M, 3, S, 1, generator=g, dtype=torch.float64) - 0.5
    wx = torch.randn(M, FC[1], generator=g, dtype=torch.float64)
    wg = torch.randn(M // G, FC[1], generator=g, dtype=torch.float64)

    # cn3d_model_conbag.py:213-229 on the modules
    h = torch.cat((yt, nets["net3DV_1"](xt)), 1)
    loc = nets["net3DV_3"](h)
    C = loc.shape[1]
    xp = nn.MaxPool2d((S, 1), stride=1)(loc).squeeze(-1).squeeze(-1)
    xg = loc.reshape(G, -1, C, S).permute(1, 2, 0, 3).reshape(-1, C, G * S, 1)
    xg = nn.MaxPool2d((S * G, 1), stride=1)(xg).squeeze(-1).squeeze(-1)
    x_m, xg_m = nets["netR_FC"](xp), nets["netR_FC"](xg)
    ((x_m * wx).sum() + (xg_m * wg).sum()).backward()
    want = {"%s.%s" % (p, k): v.grad for p, net in nets.items() for k, v in net.named_parameters()}

    x_rows = xt.permute(0, 2, 3, 1).reshape(-1, D)
    centers = yt.permute(0, 2, 1, 3).reshape(M * S, 3)
    x, xgl, stats, q, ties = forward64_eval(x_rows, centers, sd, G, S, K, "cpu", grad=True)
    ((x * wx).sum() + (xgl * wg).sum()).backward()
    assert stats == {} and ties == {}

    def err(a, b):
        return float((a - b.reshape(a.shape)).abs().max() / b.abs().max())
    assert err(x.detach(), x_m.detach()) < 1e-12 and err(xgl.detach(), xg_m.detach()) < 1e-12
    got = {k: v.grad for k, v in q.items() if v.grad is not None}
    assert set(got) == set(want) and len(got) == 6 * 4 + 4 + 2
    for bias in ("net3DV_1.0.bias", "net3DV_1.3.bias", "net3DV_1.6.bias", "net3DV_3.0.bias", "net3DV_3.3.bias",
                 "net3DV_3.6.bias", "netR_FC.0.bias"):
        assert float(want[bias].abs().max()) > 0                               # a real gradient in eval mode
    worst = max((err(got[k], want[k]), k) for k in want)
    assert worst[0] < 1e-12, worst
    # the running statistics took part and did not move
    for key in BN_KEYS:
        prefix, idx = key.split(".")
        bn = nets[prefix][int(idx)]
        assert torch.equal(bn.running_mean, sd[key + ".running_mean"]) and int(bn.num_batches_tracked) == 0


def test_bn_eval_is_the_constant_affine():
    g = torch.Generator().manual_seed(1)
    y = torch.randn(9, 6, generator=g, dtype=torch.float64)
    gamma, beta, rm = (torch.randn(6, generator=g, dtype=torch.float64) for _ in range(3))
    rv = torch.rand(6, generator=g, dtype=torch.float64) + 0.2
    s = gamma / torch.sqrt(rv + 1e-5)
    assert torch.allclose(bn_eval(y, gamma, beta, rm, rv), s * y + (beta - rm * s), rtol=0, atol=1e-14)


def test_freeze_bn_flag_checks(monkeypatch):
    from facl_amd import finetune
    p = finetune.finetune_parser()
    opt = p.parse_args([])
    assert opt.freeze_bn == 0                                                   # the default: today's behaviour
    finetune.check_finetune_flags(opt, world=1)
    opt = p.parse_args(["--freeze_bn", "0", "--checkpoint", "x.pth"])
    finetune.check_finetune_flags(opt, world=1)
    finetune.check_finetune_flags(p.parse_args(["--freeze_bn", "1", "--checkpoint", "x.pth"]), world=1)
    with pytest.raises(RuntimeError, match="--freeze_bn 1 .* needs --checkpoint"):
        finetune.check_finetune_flags(p.parse_args(["--freeze_bn", "1"]), world=1)
    with pytest.raises(RuntimeError, match="one rank"):
        finetune.check_finetune_flags(p.parse_args(["--freeze_bn", "1", "--checkpoint", "x.pth"]), world=2)
    with pytest.raises(SystemExit):
        p.parse_args(["--freeze_bn", "2"])

    # the entry refuses before any device call
    def no_device(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(torch.cuda, "set_device", no_device)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(RuntimeError, match="needs --checkpoint"):
        finetune.main(["--synthetic", "1", "--nepoch", "1", "--freeze_bn", "1"])
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(RuntimeError, match="one rank"):
        finetune.main(["--synthetic", "1", "--nepoch", "1", "--freeze_bn", "1", "--checkpoint", "x.pth"])

