"""INPUT_FEATURE_NUM 5..8 (xyz + up to five feature channels) on the MI355X: grouping, the set-abstraction passes, the full
step, the entries and the data-parallel step, held to the bars the D = 3 / 4 tests of the suite hold those paths to.  Where a
test of the suite is written for any D, it is called here with the wide widths; everything else is restated for them."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from helpers import canon_groups_np, load_golden, max_rel_rows, sa_params
from poison import poisoned  # noqa: F401  (as the autouse fixtures of the modules whose tests are called below)
from ranks import rank_env, run_ranks
from step_factory import dp_step, make_net, step_opt

import test_gpu_sa_mlp as TSA
import test_gpu_trajectory as TTRJ

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WIDE = [5, 6, 7, 8]


# ---- 1. grouping ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", WIDE)
@pytest.mark.parametrize("N", [100, 512, 2048, 4096])
def test_group_wide_vs_oracle_bitwise(D, N):
    """facl_group (through utils_my.knn_radius_group) == oracle.grouping, idx / xt / yt bit for bit; the input starts one float
    past an aligned address (rows of 5..8 floats carry no alignment rule) and the outputs are written at odd offsets too."""
    from facl_amd import _lib
    from oracle import grouping as OG
    M, S, K, r2 = 3, min(64, N), min(64, N), 0.06 if N <= 512 else 0.16
    rng = np.random.RandomState(D * 7919 + N)
    pts = (rng.rand(M, N, D) - 0.5).astype(np.float32)
    buf = torch.zeros(M * N * D + 1, device=DEV)
    buf[1:] = torch.from_numpy(pts).reshape(-1).to(DEV)
    src = buf[1:]
    idx = torch.full((M * S * K,), -7, dtype=torch.int32, device=DEV)
    xt_buf = torch.full((M * S * K * D + 1,), float("nan"), device=DEV)
    yt = torch.full((M * S * 3,), float("nan"), device=DEV)
    lib = _lib.load_library()
    _lib.check(lib.facl_group(_lib.ptr(src), M, N, D, S, K, r2, _lib.ptr(idx), _lib.ptr(xt_buf[1:]), _lib.ptr(yt), _lib.stream()),
               "facl_group")
    ridx, rxt, ryt = OG.group_points(pts, S, K, r2)
    np.testing.assert_array_equal(idx.view(M, S, K).cpu().numpy(), ridx)
    np.testing.assert_array_equal(xt_buf[1:].view(M, S, K, D).cpu().numpy(), rxt)
    np.testing.assert_array_equal(yt.view(M, S, 3).cpu().numpy(), ryt)
    assert torch.isnan(xt_buf[0])                                       # nothing written in front of the output


@pytest.mark.parametrize("D", WIDE)
@pytest.mark.parametrize("N", [100, 512, 2048, 4096])
def test_group_clips_wide_clip_major_vs_oracle(D, N):
    """facl_group_clips on the loader's (B,G,N,D) batch: view-major outputs (cloud m = g*B + b) == the oracle on the permuted copy."""
    from facl_amd import utils_my
    from oracle import grouping as OG
    B, G = 2, 3
    torch.manual_seed(D * N)
    clips = torch.rand(B, G, N, D) - 0.5
    S, K = min(64, N), min(64, N)
    xt, yt, idx = utils_my.knn_radius_group(clips.to(DEV), S, K, 0.1, want_idx=True)
    ridx, rxt, ryt = OG.group_points(clips.permute(1, 0, 2, 3).reshape(-1, N, D).numpy(), S, K, 0.1)
    np.testing.assert_array_equal(idx.cpu().numpy(), ridx)
    np.testing.assert_array_equal(xt.permute(0, 2, 3, 1).cpu().numpy(), rxt)
    np.testing.assert_array_equal(yt.squeeze(-1).permute(0, 2, 1).cpu().numpy(), ryt)


def test_group_c1_d8_golden():
    """The reference's own group_points_3DV at D = 8 (c1_d8.npz): xt_sum, the first groups and yt, bit for bit."""
    from facl_amd import utils_my
    g = load_golden("c1_d8.npz")
    opt = SimpleNamespace(SAMPLE_NUM=512, sample_num_level1=64, knn_K=1, ball_radius=0.16, INPUT_FEATURE_NUM=0)
    xt, yt = utils_my.group_points_3DV(torch.from_numpy(g["points"]).to(DEV), opt)
    assert opt.INPUT_FEATURE_NUM == 8
    c = canon_groups_np(xt.permute(0, 2, 3, 1).cpu().numpy())
    np.testing.assert_array_equal(c[:len(g["xt_first8"])], g["xt_first8"])
    np.testing.assert_array_equal(c.sum(axis=2), g["xt_sum"])
    np.testing.assert_array_equal(yt.contiguous().cpu().numpy(), g["yt"])


# ---- 2. / 3. moments and the layer-1 chain -------------------------------------------------------------------------------
@pytest.mark.parametrize("D", WIDE)
def test_x_moments_wide_vs_numpy_fp64(D, poisoned):
    from facl_amd import _lib, sa_mlp
    lib = _lib.load_library()
    P = 64 * 1021 + 64
    x = ((torch.rand(P, D, device=DEV, generator=torch.Generator(device=DEV).manual_seed(D)) - 0.3) * 2).contiguous()
    mom = torch.full((D + D * D,), float("nan"), dtype=torch.float64, device=DEV)
    ws = sa_mlp._Workspace.get(x.device)
    _lib.check(lib.facl_sa_x_moments(_lib.ptr(x), P, D, _lib.ptr(mom), _lib.ptr(ws), _lib.stream()), "facl_sa_x_moments")
    xd = x.cpu().numpy().astype(np.float64)
    ref = np.concatenate((xd.sum(0), (xd.T @ xd).reshape(-1)))
    got = mom.cpu().numpy()
    assert np.all(np.abs(got - ref) <= 1e-12 * np.maximum(np.abs(ref), np.abs(xd).sum(0).max())), np.abs(got - ref).max()
    X2 = got[D:].reshape(D, D)
    np.testing.assert_array_equal(X2, X2.T)                                # the mirrored triangle


@pytest.mark.parametrize("D", WIDE)
def test_bn1_chain_wide_equals_its_three_launches_bitwise(D):
    """facl_sa_bn1_chain == facl_bn1_sums_from_moments + facl_bn_finalize + facl_sa_l1tab, every output bit for bit, with the
    wide layer-1 table (64, 12): weights in columns 0..7 (zero past D), the bias in column 8."""
    from facl_amd import _lib
    lib = _lib.load_library()
    p = _lib.ptr
    L = _lib.sa_l1_cols(D)
    assert L == 12
    g = torch.Generator(device=DEV).manual_seed(17 + D)
    P = 50000.0
    x = torch.randn(4096, D, device=DEV, generator=g, dtype=torch.float64)
    mom = torch.cat(((x.sum(0) * (P / 4096)), ((x.t() @ x) * (P / 4096)).reshape(-1))).contiguous()
    W1 = (torch.randn(64, D, device=DEV, generator=g) * 0.5).contiguous()
    b1 = torch.randn(64, device=DEV, generator=g)
    gam = torch.randn(64, device=DEV, generator=g)
    bet = torch.randn(64, device=DEV, generator=g)
    outs = []
    for fused in (False, True):
        rm, rv = torch.zeros(64, device=DEV), torch.ones(64, device=DEV)
        sums = torch.full((64, 2), float("nan"), device=DEV, dtype=torch.float64)
        bnc = torch.full((5, 64), float("nan"), device=DEV)
        tab = torch.full((64, L), float("nan"), device=DEV)
        amax = torch.zeros(_lib.AMAX_WORDS, dtype=torch.int32, device=DEV)
        if fused:
            _lib.check(lib.facl_sa_bn1_chain(p(mom), P, D, p(W1), p(b1), p(gam), p(bet), 1e-5, 0.1, p(rm), p(rv), p(sums), p(bnc),
                                             p(amax), p(tab), _lib.stream()), "chain")
        else:
            _lib.check(lib.facl_bn1_sums_from_moments(p(mom), P, D, p(W1), p(b1), p(sums), _lib.stream()), "sums")
            _lib.check(lib.facl_bn_finalize(p(sums), 64, P, p(gam), p(bet), 1e-5, 0.1, p(rm), p(rv), p(bnc), p(amax), None,
                                            _lib.stream()), "finalize")
            _lib.check(lib.facl_sa_l1tab(p(W1), p(b1), D, p(bnc[2]), p(bnc[3]), p(tab), None, None, _lib.stream()), "l1tab")
        outs.append([t.cpu() for t in (sums, bnc, tab, rm, rv, amax)])
    for a, b in zip(*outs):
        assert torch.equal(a.view(torch.uint8) if a.is_floating_point() else a, b.view(torch.uint8) if b.is_floating_point() else b)
    tab = outs[1][2]
    torch.testing.assert_close(tab[:, :D], (outs[1][1][2][:, None] * W1.cpu()), rtol=0, atol=0)
    assert torch.all(tab[:, D:8] == 0) and torch.all(tab[:, 9:] == 0)
    assert torch.equal(tab[:, 8], outs[1][1][2] * b1.cpu() + outs[1][1][3])


# ---- 4. / 5. the SA point-MLP: forward, backward, ragged unit counts, the one-kernel eval ----------------------------------
@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("D", WIDE)
def test_sa_forward_wide_vs_oracle(D, training, poisoned):
    TSA.test_sa_forward_vs_oracle(D, False, training)


@pytest.mark.parametrize("D", WIDE)
def test_sa_backward_wide_vs_oracle_fp64(D, poisoned):
    TSA.test_sa_backward_vs_oracle_fp64(D, False)


@pytest.mark.parametrize("D", [5, 8])
def test_sa_backward_wide_negative_gamma(D, poisoned):
    TSA.test_sa_backward_vs_oracle_fp64(D, True)


@pytest.mark.parametrize("D", WIDE)
@pytest.mark.parametrize("nunits", [7, 1021, 1026])
def test_sa_ragged_unit_counts_wide(D, nunits, poisoned):
    """test_gpu_sa_mlp.py::test_sa_ragged_unit_counts at the wide widths (forward and every parameter gradient vs fp64 routed
    through the kernels' max-pool decisions, NaN-poisoned scratch)."""
    from facl_amd import sa_mlp
    from oracle.weights import formula_state_dict
    K = 64
    torch.manual_seed(nunits + 100 * D)
    x_rows = ((torch.rand(nunits * K, D, device=DEV) - 0.5) * 0.8).contiguous()
    sd = formula_state_dict(D)
    p = sa_params(sd, DEV)
    params = [p[k].clone().requires_grad_(True) for k in sa_mlp._PARAM_ORDER]
    state = {"buffers": {k: p[k] for k in ("rm1", "rv1", "rm2", "rv2", "rm3", "rv3")}, "training": True}
    pooled = sa_mlp.SAMLPFunction.apply(x_rows, state, *params)
    w = torch.randn(pooled.shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    (pooled * w).sum().backward()
    q = {k: p[k].detach().double().requires_grad_(True) for k in sa_mlp._PARAM_ORDER}
    h = x_rows.double()
    for Wk, bk, gk, bek in (("W1", "b1", "g1", "be1"), ("W2", "b2", "g2", "be2"), ("W3", "b3", "g3", "be3")):
        y = h @ q[Wk].reshape(q[Wk].shape[0], -1).t() + q[bk]
        mean, var = y.mean(0), y.var(0, unbiased=False)
        h = torch.relu((y - mean) / torch.sqrt(var + 1e-5) * q[gk] + q[bek])
    h3 = h.view(nunits, K, 256)
    ref, ref_arg = h3.max(dim=1)
    assert max_rel_rows(pooled.detach().cpu().numpy(), ref.detach().cpu().numpy()) < 5e-5
    my_arg = pooled.grad_fn.c["arg"].long()
    flips = int((my_arg != ref_arg).sum())
    assert flips <= max(2, 1e-4 * ref_arg.numel())
    got = torch.gather(h3, 1, my_arg.unsqueeze(1)).squeeze(1)
    assert float(((ref - got).abs() / torch.maximum(ref.abs(), h3.detach().abs().mean())).max()) < 1e-5
    (got * w.double()).sum().backward()
    gmax = max(float(q[k].grad.norm()) for k in q)
    for k, mine in zip(sa_mlp._PARAM_ORDER, params):
        if k in ("b1", "b2", "b3"):
            continue
        g64 = q[k].grad
        err = float((mine.grad.double() - g64).norm())
        assert err <= 2e-3 * max(float(g64.norm()), 1e-2 * gmax), (k, err, float(g64.norm()), flips)


@pytest.mark.parametrize("D,K", [(8, 64), (5, 64), (6, 64), (7, 64), (8, 128)])
def test_sa_eval_one_kernel_wide(D, K, poisoned):
    TSA.test_sa_eval_one_kernel_vs_training_kernels_and_fp64(D, False, K)


# ---- 6. the full model step at D = 8 --------------------------------------------------------------------------------------
@pytest.fixture
def d8_config(monkeypatch):
    # B = 4, G = 8: at B = 3, G = 5 the contrastive loss of the 8-channel formula weights is small (~0.5) and cancels -- plain
    # torch fp32 misses the 1e-4 loss bar there by itself (1.9e-4 measured); here fp32 sits at ~1e-6 of fp64
    monkeypatch.setitem(TTRJ.CONFIGS, "d8", dict(B=4, G=8, N=512, D=8, view_major=False))
    return "d8"


def test_consecutive_steps_d8_vs_fp64(d8_config, poisoned):
    """Grouping, encoder, both losses, backward and FusedAdam at D = 8 against helpers.reference_step64, step after step
    (test_gpu_trajectory.py's bars)."""
    TTRJ.test_consecutive_eager_steps_vs_fp64(d8_config)


def test_graph_replay_steps_equal_eager_steps_d8(d8_config, poisoned):
    TTRJ.test_graph_replay_steps_equal_eager_steps_bitwise(d8_config)


def test_c1_d8_golden_features(poisoned):
    """The model's eval- and training-mode features on the reference's D = 8 fixture: within the golden's own fp32 distance to
    the fp64 oracle + 1e-4 (as test_gpu_encoder.py does for d3 / d4)."""
    from facl_amd.utils_my import group_points_3DV
    from oracle import encoder as E, grouping as OG
    from oracle.weights import formula_state_dict
    g = load_golden("c1_d8.npz")
    B, G, N, S, K, D = [int(v) for v in g["meta"]]
    assert D == 8
    xt, yt = group_points_3DV(torch.from_numpy(g["points"]).to(DEV), step_opt(D, B, 512))
    _, xo, yo = OG.group_points(g["points"], S, K, 0.06)
    xt64 = torch.from_numpy(xo).permute(0, 3, 1, 2).double()
    yt64 = torch.from_numpy(yo).view(G * B, 1, S, 3).transpose(1, 3).double()
    for mode in ("eval", "train"):
        net = make_net(D, G, B)
        net = net.eval() if mode == "eval" else net.train()
        with torch.no_grad():
            out = net(xt, yt) if mode == "eval" else net(xt, yt, 1)
            sd64 = {k: (torch.as_tensor(v).double() if np.asarray(v).dtype.kind == "f" else torch.as_tensor(v).clone())
                    for k, v in formula_state_dict(D).items()}
            ref = E.encoder_forward(sd64, xt64, yt64, G, training=(mode == "train"))
        for name, mine, r64 in zip(("x", "code", "x_nor", "x_global"), out, ref):
            if f"{mode}_{name}" not in g:
                continue
            floor = max_rel_rows(g[f"{mode}_{name}"], r64.numpy())
            e = max_rel_rows(mine.detach().cpu().numpy(), r64.numpy())
            print(f"{mode} {name}: mine-vs-fp64 {e:.2e}  golden-vs-fp64 {floor:.2e}")
            assert e < floor + 1e-4, (mode, name, e, floor)


# ---- 7. the entries -------------------------------------------------------------------------------------------------------
def test_train_d8_checkpoint_then_extract(tmp_path):
    from facl_amd import cn3d_train_motion_GL as train, extract_motion_feature as ext
    from facl_amd.cn3d_model_conbag import PointNet_Plus
    from facl_amd.extract_common import extract_batch, save_single_feature
    from oracle import encoder as E, grouping as OG
    from oracle.weights import state_dict_shapes
    D = 8
    ck = str(tmp_path / "ck")
    train.main(["--batchSize", "4", "--nepoch", "1", "--steps_per_epoch", "2", "--num_crop", "4", "--SAMPLE_NUM", "512",
                "--save_root_dir", ck, "--INPUT_FEATURE_NUM", str(D), "--synthetic", "1"])
    path = os.path.join(ck, "corr_GL_0.pth")
    sd = torch.load(path, map_location="cpu", weights_only=True)
    assert list(sd.keys()) == [k for k, _ in state_dict_shapes(D)] and len(sd) == 52
    assert tuple(sd["net3DV_1.0.weight"].shape) == (64, D, 1, 1)
    assert all(torch.isfinite(v).all() for v in sd.values() if v.is_floating_point())
    feats = ext.main(["--checkpoint", path, "--batchSize", "3", "--num_crop", "4", "--SAMPLE_NUM", "512",
                      "--INPUT_FEATURE_NUM", str(D), "--num_batches", "1", "--save_path", str(tmp_path / "f")])
    assert feats.shape == (3, 5 * 512) and np.isfinite(feats).all()
    opt = step_opt(D, 3, 512)
    m = PointNet_Plus(opt, gost=4)
    m.load_state_dict(sd)
    m = m.to(DEV).eval()
    torch.manual_seed(0)
    clip = torch.rand(3, 4, 512, D) - 0.5
    with torch.no_grad():
        f = extract_batch(m, clip.to(DEV), opt).cpu().numpy()
    pts = clip.permute(1, 0, 2, 3).reshape(-1, 512, D).numpy()
    _, xt, yt = OG.group_points(pts, 64, 64, 0.06)
    sdo = {k: v.double() if v.is_floating_point() else v.clone() for k, v in sd.items()}
    with torch.no_grad():
        x, _, _, xg = E.encoder_forward(sdo, torch.from_numpy(xt).permute(0, 3, 1, 2).double(),
                                        torch.from_numpy(yt).view(12, 1, 64, 3).transpose(1, 3).double(), 4, training=False)
    ref = save_single_feature(torch.cat((x, xg), 0).numpy(), str(tmp_path), ["a", "b", "c"], num_crop=5)
    err = np.linalg.norm(f - ref, axis=1) / np.linalg.norm(ref, axis=1)
    assert err.max() < 1e-4, err


def test_appearance_entries_d8(tmp_path):
    from facl_amd import cn3d_train_apperance_GL as train, extract_apperance_feature as ext
    ck = str(tmp_path / "ck")
    train.main(["--batchSize", "4", "--nepoch", "1", "--steps_per_epoch", "1", "--num_crop", "4", "--SAMPLE_NUM", "512",
                "--save_root_dir", ck, "--INPUT_FEATURE_NUM", "8", "--synthetic", "1"])
    path = os.path.join(ck, "corr_GL_appereance_0.pth")               # the appearance entry's checkpoint name
    sd = torch.load(path, map_location="cpu", weights_only=True)
    assert tuple(sd["net3DV_1.0.weight"].shape) == (64, 8, 1, 1)
    feats = ext.main(["--checkpoint", path, "--batchSize", "2", "--num_crop", "4", "--SAMPLE_NUM", "512",
                      "--INPUT_FEATURE_NUM", "8", "--num_batches", "1", "--save_path", str(tmp_path / "f")])
    assert np.isfinite(feats).all()


def test_dataset_entry_still_refuses_d8(tmp_path):
    from facl_amd import cn3d_train_motion_GL as train
    with pytest.raises(RuntimeError, match="--INPUT_FEATURE_NUM 4"):
        train.main(["--batchSize", "4", "--nepoch", "1", "--num_crop", "10", "--SAMPLE_NUM", "512", "--INPUT_FEATURE_NUM", "8",
                    "--synthetic", "0", "--data_root", str(tmp_path), "--save_root_dir", str(tmp_path / "ck")])


# ---- 8. two ranks on one GPU at D = 8 ------------------------------------------------------------------------------------
def _worker_d8(rank, world, port, q, extra_env=None):
    rank_env(rank, world, port, FACL_DIST_BACKEND="gloo", **(extra_env or {}))
    import torch.distributed as dist
    from facl_amd import dist as fdist
    torch.cuda.set_device(0)
    fdist.init_from_env()
    torch.manual_seed(3)
    G, Bl, N, D = 4, 2, 512, 8
    full = torch.rand(Bl * world, G, N, D) - 0.5
    loss, grads, bufs = dp_step(full[rank * Bl:(rank + 1) * Bl], G, rank, world)
    q.put((rank, loss, {k: v.numpy() for k, v in grads.items()}, {k: v.numpy() for k, v in bufs.items()}))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("oneshot", [False, True])
def test_two_ranks_d8_equal_single_process_global_batch(oneshot):
    port = 31700 + (os.getpid() % 2000) + (7 if oneshot else 0)
    env = {"FACL_ONESHOT_SYNCBN": "1" if oneshot else "0"}
    res = run_ranks(_worker_d8, 2, port, args=(env,), timeout=300)
    torch.manual_seed(3)
    G, Bl, N, D = 4, 2, 512, 8
    full = torch.rand(Bl * 2, G, N, D) - 0.5
    loss1, grads1, bufs1 = dp_step(full, G, 0, 1)
    loss2 = 0.5 * (res[0][1] + res[1][1])
    assert abs(loss1 - loss2) <= 1e-5 * abs(loss1)
    gmax = max(float(np.linalg.norm(v.numpy())) for v in grads1.values())
    for k, g1 in grads1.items():
        g1 = g1.numpy()
        for r in (0, 1):
            g2 = res[r][2][k]
            assert np.linalg.norm(g2 - g1) <= 2e-4 * max(np.linalg.norm(g1), 1e-2 * gmax) + 1e-6, (k, r)
    for k, b1 in bufs1.items():
        assert np.allclose(res[0][3][k], b1.numpy(), rtol=2e-5, atol=1e-7), k


# ---- the A/B switches of the layer-1 kernels, at the wide widths ---------------------------------------------------------
# The switches are read once per process (static initialisers in the library, module constants in sa_mlp.py): each case runs in a
# fresh interpreter.
_SWITCH_SCRIPT = r"""
import sys
sys.path[:0] = [{root!r}, {tests!r}]
import torch
from facl_amd import _lib
import test_gpu_sa_mlp as T
D, expect = int(sys.argv[1]), sys.argv[2]
with _lib.poisoned():
    if expect == "refused":
        try:
            T.test_sa_backward_vs_oracle_fp64(D, False)
        except RuntimeError as e:
            assert "facl_sa_bwd2 failed: unsupported configuration" in str(e), e
            print("SWITCH-REFUSED")
        sys.exit(0)
    T.test_sa_forward_vs_oracle(D, False, True)
    T.test_sa_forward_vs_oracle(D, False, False)
    T.test_sa_backward_vs_oracle_fp64(D, False)
print("SWITCH-OK")
"""


@pytest.mark.parametrize("switch,D,expect", [
    ("FACL_SA_F32", 8, "ok"),        # fwd2 on the exact-fp32 MFMA: k_sa_fwd2<8>
    ("FACL_FWD_H3", 8, "ok"),        # value 0: bf16x6 forward, k_sa_fwd2_sb<8, false> (and the unfused eval path)
    ("FACL_BWD_H3", 8, "ok"),        # value 0: bf16x6 backward, k_sa_bwd2_sb<8, false>
    ("FACL_BWD2_F32", 4, "ok"),      # the exact-fp32 bwd2 kernel, D <= 4 as before
    ("FACL_BWD2_F32", 8, "refused"),  # ... which does not fit a CU's LDS at D > 4: FACL_E_CONFIG, never a silent substitute
])
def test_layer1_switches_at_wide_widths(switch, D, expect):
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    value = "0" if switch in ("FACL_FWD_H3", "FACL_BWD_H3") else "1"
    env = dict(os.environ, **{switch: value})
    r = subprocess.run([sys.executable, "-c", _SWITCH_SCRIPT.format(root=root, tests=os.path.join(root, "tests")), str(D), expect],
                       env=env, cwd=root, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0, out[-3000:]
    assert ("SWITCH-REFUSED" if expect == "refused" else "SWITCH-OK") in out, out[-3000:]
