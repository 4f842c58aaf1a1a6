"""INPUT_FEATURE_NUM 3..8 on the CPU side: the oracle at D = 8 against the reference's own run (c1_d8.npz, written by
tools/make_golden_d8.py), the D -> layer-1 layout rule of include/facl_hip.h against facl_amd/_lib.py, and the width checks of
the native entries (they return before any launch, so they run without a GPU)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from oracle import encoder as E
from oracle import grouping as OG
from oracle import loss as OL
from oracle import step as OS
from oracle.weights import formula_state_dict

from helpers import canon_groups_np, load_golden, max_rel_rows, rel_err
from test_oracle_golden import GTOL, PARAM3_TOL_CPU, PRE_BN_BIAS, TOL, check_param3

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def _conv_without_onednn():
    """As in test_oracle_golden.py: the oracle's fp32 1x1 convolutions through ATen's GEMM path (host-independent order)."""
    prev = torch.backends.mkldnn.enabled
    torch.backends.mkldnn.enabled = False
    try:
        yield
    finally:
        torch.backends.mkldnn.enabled = prev


def test_c1_d8_oracle_forward_loss_backward_adam(_conv_without_onednn):
    """test_oracle_golden.py::test_c1_forward_loss_backward_adam's assertions on the 8-channel fixture, minus the stage taps
    and the normalised features that the fixture does not carry (its size limit; the D = 3 / 4 fixtures pin those stages)."""
    tag, D, neg = "d8", 8, False
    g = load_golden(f"c1_{tag}.npz")
    B, G, N, S, K, D_ = [int(v) for v in g["meta"]]
    assert D_ == D
    pts = g["points"]
    idx, xt, yt = OG.group_points(pts, S, K, 0.06)
    xt_c = canon_groups_np(xt)
    np.testing.assert_array_equal(xt_c[:len(g["xt_first8"])], g["xt_first8"])     # the fixture keeps the first groups
    np.testing.assert_allclose(xt_c.sum(axis=2), g["xt_sum"], rtol=0, atol=1e-4)
    M = G * B
    xt_t = torch.from_numpy(xt).permute(0, 3, 1, 2)
    yt_t = torch.from_numpy(yt).view(M, 1, S, 3).transpose(1, 3)
    np.testing.assert_array_equal(yt_t.contiguous().numpy(), g["yt"])

    # Truth = the oracle evaluated in fp64.  The golden is the reference's fp32 run on the machine that made it; the
    # oracle's fp32 run on THIS machine (other core count / oneDNN blocking) rounds differently, and train-mode BN over few
    # rows plus max-pool near-ties amplify that (golden vs fp64: 4e-5 on d4 up to 1.5e-3 on d3's x_global).  So: the fp64
    # oracle must sit within fp32 noise of the golden (the PIN), and the fp32 oracle within twice that noise + TOL.
    def sd_as(dtype):
        return {k: (torch.as_tensor(v).to(dtype) if np.asarray(v).dtype.kind == "f" else torch.as_tensor(v).clone())
                for k, v in formula_state_dict(D, neg_gamma=neg).items()}

    def check(mine32, ref64, gold, name, pin=3e-3):
        floor = max_rel_rows(gold, ref64)
        assert floor < pin, (name, floor)                               # fp64 oracle == reference up to its fp32 noise
        assert max_rel_rows(mine32, gold) < 2 * floor + TOL, name

    xt64, yt64 = xt_t.double(), yt_t.double()
    # eval
    sd = E.clone_state(formula_state_dict(D, neg_gamma=neg))
    with torch.no_grad():
        ev = E.encoder_forward(sd, xt_t, yt_t, G, training=False)
        ev64 = E.encoder_forward(sd_as(torch.float64), xt64, yt64, G, training=False)
    for name, t, t64 in zip(("x", "code", "x_nor", "x_global"), ev, ev64):
        if f"eval_{name}" not in g:                                    # x_nor: dropped from the fixture (tools/make_golden_d8.py)
            continue
        check(t.numpy(), t64.numpy(), g[f"eval_{name}"], "eval_" + name)

    # fp64 truth of the first training step (outputs, taps, losses, gradients)
    sd64 = sd_as(torch.float64)
    pk = E.param_keys(sd64)
    for k in pk:
        sd64[k].requires_grad_(True)
    out64, inter64 = E.encoder_forward(sd64, xt64, yt64, G, training=True, return_intermediates=True)
    lc64, lo64 = OL.global_contrast(G, out64[3], out64[0], B), OL.circle_contrast(G, out64[0], B, g["order"])
    (lc64 + lo64).backward()
    g64 = {k: sd64[k].grad.numpy() for k in pk if sd64[k].grad is not None}

    # 3 training steps
    sd = E.clone_state(formula_state_dict(D, neg_gamma=neg))
    opt = OS.AdamState(sd)
    order = g["order"]
    losses = []
    for it in range(3):
        r = OS.train_step(sd, opt, None, B, G, S, K, 0.06, order, epoch=0, grouped=(xt_t, yt_t))
        losses.append(r["loss"])
        if it == 0:
            for name, t, t64 in zip(("x", "code", "x_nor", "x_global"), r["outputs"], out64):
                if f"train_{name}" not in g:
                    continue
                check(t.numpy(), t64.detach().numpy(), g[f"train_{name}"], name)
            for mine_l, key, l64 in ((r["loss_c"], "loss_c", float(lc64)), (r["loss_circle"], "loss_circle", float(lo64))):
                gold = float(g[key])
                assert abs(gold - l64) <= 1e-3 * abs(l64), key
                assert abs(mine_l - gold) <= 2 * abs(gold - l64) + TOL * abs(gold), key
            gmax = max(float(g[k]) for k in g if k.startswith("gradnorm/"))
            for k, gr in r["grads"].items():
                if f"gradnone/{k}" in g:
                    continue
                gn = float(g[f"gradnorm/{k}"])
                mine = float(np.linalg.norm(gr.numpy().astype(np.float64)))
                if k in PRE_BN_BIAS:
                    # a bias feeding a train-mode BN has mathematically ZERO gradient; the reference's
                    # value is pure cancellation noise (norm ~1e-1 at loss ~1e2) -> only bound it.
                    wn = float(g[f"gradnorm/{k[:-4]}weight"])
                    assert mine <= 1e-2 * wn and gn <= 1e-2 * wn, (k, mine, gn, wn)
                    continue
                # atol: 1e-6 of the largest parameter-gradient norm (net3DV_3.7.bias is mathematically
                # ~0 too: a common shift of x_pre[:,c] is removed by netR_FC's BatchNorm1d).
                scale = max(gn, 1e-2 * gmax)
                floor_n = abs(gn - float(np.linalg.norm(g64[k])))        # the golden's own distance to the fp64 truth
                assert abs(mine - gn) <= 2 * floor_n + GTOL * scale + 1e-5, (k, mine, gn)
                if f"grad/{k}" in g:
                    floor_v = np.linalg.norm(g[f"grad/{k}"] - g64[k])
                    assert floor_v <= 6e-2 * scale + 1e-5, (k, floor_v)  # the PIN: fp64 oracle gradient == reference's (fp32 noise: up to 3e-2 on d3)
                    assert np.linalg.norm(gr.numpy() - g[f"grad/{k}"]) <= 2 * floor_v + GTOL * scale + 1e-5, k
            for k in sd:
                if "running_" in k:
                    floor_b = rel_err(g[f"buf1/{k}"], sd64[k].detach().numpy())      # golden (fp32) vs fp64 truth
                    assert floor_b < 1e-3, (k, floor_b)
                    assert rel_err(sd[k].numpy(), g[f"buf1/{k}"]) < 2 * floor_b + 1e-5, k
                if "num_batches" in k:
                    assert int(sd[k]) == int(g[f"buf1/{k}"]), k
    l64 = float(lc64 + lo64)
    assert abs(losses[0] - g["losses3"][0]) <= 2 * abs(g["losses3"][0] - l64) + TOL * abs(l64)
    # later steps amplify rounding differences through Adam's normalised update (another CPU's fp32 summation order moves
    # step 3 by up to 2 %): looser bound
    np.testing.assert_allclose(losses, g["losses3"], rtol=3e-2)
    for k in sd:
        if "running_" in k:
            # the pre-BN biases random-walk by +-lr per step on their pure-noise gradients (see
            # PRE_BN_BIAS) and running_mean follows them: 1e-4 absolute on values of ~5e-2.
            assert rel_err(sd[k].numpy(), g[f"buf3/{k}"]) < 1e-2, k
    # fp64 truth of the three Adam steps (the fp32 runs -- the reference's and this machine's -- scatter around it)
    sd64b = sd_as(torch.float64)
    opt64 = OS.AdamState(sd64b)
    for it in range(3):
        OS.train_step(sd64b, opt64, None, B, G, S, K, 0.06, order, epoch=0, grouped=(xt64, yt64))
    check_param3(g, {k: v.detach().numpy() for k, v in sd.items()}, formula_state_dict(D, neg_gamma=neg), tol=PARAM3_TOL_CPU,
                 truth={k: v.detach().numpy() for k, v in sd64b.items()})


def _header():
    return open(os.path.join(ROOT, "include", "facl_hip.h")).read()


def test_header_and_binding_agree_on_the_layer1_layouts():
    from facl_amd import _lib
    txt = _header()
    dmin = int(re.search(r"#define\s+FACL_SA_D_MIN\s+(\d+)", txt).group(1))
    dmax = int(re.search(r"#define\s+FACL_SA_D_MAX\s+(\d+)", txt).group(1))
    assert (dmin, dmax) == (_lib.SA_D_MIN, _lib.SA_D_MAX) == (3, 8)
    m = re.search(r"#define\s+FACL_SA_L1_COLS\(D\)\s+\(\(D\)\s*<=\s*(\d+)\s*\?\s*(\d+)\s*:\s*(\d+)\)", txt)
    assert m, "FACL_SA_L1_COLS(D) is no longer of the form ((D) <= a ? b : c)"
    lim, narrow, wide = (int(v) for v in m.groups())
    m = re.search(r"#define\s+FACL_SA_BWD2_OUT\(D\)\s+\(64 \* 64 \+ 64 \* FACL_SA_L1_COLS\(D\)\)", txt)
    assert m, "FACL_SA_BWD2_OUT(D) changed form"
    for D in range(dmin, dmax + 1):
        cols = narrow if D <= lim else wide
        assert _lib.sa_l1_cols(D) == cols
        assert cols - 4 >= D and cols % 4 == 0              # every weight fits before the bias column; float4 rows
        assert _lib.sa_bwd2_out(D) == 64 * 64 + 64 * cols
        assert cols >= D + 1                                # R1: D rows of x_d dz1, then sum dz1
    # D <= 4 keeps the layouts it always had
    assert _lib.sa_l1_cols(3) == _lib.sa_l1_cols(4) == 8 and _lib.sa_bwd2_out(4) == 4608
    assert _lib.sa_bwd2_out(8) == 4864


@pytest.mark.parametrize("D", [2, 9])
def test_native_entries_refuse_unsupported_widths(D):
    from facl_amd import _lib, build
    build.build()
    lib = _lib.load_library()
    M, N, S, K = 1, 64, 8, 8
    pts = np.zeros((M, N, max(D, 1)), dtype=np.float32)
    idx = np.zeros((M, S, K), dtype=np.int32)
    xt = np.zeros((M, S, K, max(D, 1)), dtype=np.float32)
    yt = np.zeros((M, S, 3), dtype=np.float32)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)            # noqa: E731  host buffers: the shape check returns first
    assert lib.facl_group(p(pts), M, N, D, S, K, 0.06, p(idx), p(xt), p(yt), None) == -1
    assert lib.facl_group_clips(p(pts), 1, 1, N, D, S, K, 0.06, p(idx), p(xt), p(yt), None) == -1
    x = np.zeros((64, max(D, 1)), dtype=np.float32)
    mom = np.zeros(D + D * D, dtype=np.float64)
    ws = np.zeros(16, dtype=np.uint8)
    assert lib.facl_sa_x_moments(p(x), 64, D, p(mom), p(ws), None) == -1
