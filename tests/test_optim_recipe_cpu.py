"""The optimizer recipe (--adamw_decay, --clip_grad_norm, --lr_schedule, --warmup_steps, --lr_decay_epochs, --lr_min), host side:
the closed form of the schedule, the flag checks, the state file's compatibility with states written before the flags, the
refusals of the entries before the device, and the C ABI symbols and their refusals (all before any launch, so they run
without a device)."""
import ctypes
import math
import os
import re

import pytest

from facl_amd import train_state as ts
from facl_amd.train_common import build_parser, check_optim_flags

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_SHAPE, E_NULL = -1, -2
LR0, LR_MIN = 3e-4, 1e-5


# ---- 1: lr_at_step -----------------------------------------------------------------------------------------------------------
def _direct(lr0, t, schedule, W, T, lr_min):
    """The issue's formulas, written out again in fp64."""
    warm = min(1.0, t / W) if W else 1.0
    if schedule == "step":
        return warm * lr0
    tp, Tp = max(t - W, 0), T - W
    return warm * (lr_min + (lr0 - lr_min) * 0.5 * (1.0 + math.cos(math.pi * min(tp, Tp) / Tp)))


@pytest.mark.parametrize("schedule,W,T", [("step", 0, 0), ("step", 5, 0), ("cosine", 0, 10), ("cosine", 3, 10)])
def test_lr_at_step_against_the_direct_formula(schedule, W, T):
    from facl_amd.optim import lr_at_step
    TT = T or 10
    ts_ = sorted({1, max(W, 1), W + 1, TT, TT + 1, 10 * TT})
    lr_min = LR_MIN if schedule == "cosine" else 0.0
    for t in ts_:
        got = lr_at_step(LR0, t, schedule, W, T, lr_min)
        want = _direct(LR0, t, schedule, W, T, lr_min)
        assert abs(got - want) <= 4 * 2.0 ** -53 * LR0, (t, got, want)      # the same few fp64 operations
    # the warm-up is linear in t and ends at the base rate (under cosine lr_min + (lr0 - lr_min), one rounding from lr0)
    top = LR0 if schedule == "step" else lr_min + (LR0 - lr_min) * 0.5 * 2.0
    assert abs(top - LR0) <= 2.0 ** -52 * LR0
    for t in range(1, W + 1):
        assert lr_at_step(LR0, t, schedule, W, T, lr_min) == (t / W) * top, t
    if W:
        assert lr_at_step(LR0, W, schedule, W, T, lr_min) == top
    if schedule == "step":
        assert all(lr_at_step(LR0, t, schedule, W, T) == LR0 for t in (W + 1, 50, 1000))
    else:
        assert lr_at_step(LR0, T, schedule, W, T, lr_min) == lr_min         # cos(pi) = -1 exactly
        assert lr_at_step(LR0, T + 1, schedule, W, T, lr_min) == lr_min and lr_at_step(LR0, 10 * T, schedule, W, T, lr_min) == lr_min
        mid = [lr_at_step(LR0, t, schedule, W, T, lr_min) for t in range(max(W, 1), T + 1)]
        assert all(a > b for a, b in zip(mid, mid[1:]))                     # falling from the end of the warm-up to T


def test_lr_at_step_refuses():
    from facl_amd.optim import lr_at_step
    with pytest.raises(ValueError, match="schedule"):
        lr_at_step(LR0, 1, "linear")
    with pytest.raises(ValueError, match="decay_steps"):
        lr_at_step(LR0, 1, "cosine", 5, 5)


# ---- 2: check_optim_flags ----------------------------------------------------------------------------------------------------
COSINE = ["--lr_schedule", "cosine", "--lr_decay_epochs", "2"]


def test_parser_defaults_are_the_state_defaults():
    o = build_parser('0').parse_args([])
    assert {k: getattr(o, k) for k in ts.LATER_FLAG_DEFAULTS} == ts.LATER_FLAG_DEFAULTS
    assert set(ts.LATER_FLAG_DEFAULTS) <= set(ts.TRAJECTORY_FLAGS)
    assert (o.weight_decay, o.momentum, o.learning_rate_decay) == (0.0008, 0.9, 1e-7)      # parsed and unread, as in the reference


def test_check_optim_flags():
    p = build_parser('0')
    check_optim_flags(p.parse_args([]), world=1)
    check_optim_flags(p.parse_args([]), world=2)                            # the defaults: nothing to refuse
    check_optim_flags(p.parse_args(["--adamw_decay", "0.05", "--clip_grad_norm", "1", "--warmup_steps", "3", "--lr_min", "1e-5"]
                                   + COSINE), world=1)
    for flag in ("adamw_decay", "clip_grad_norm"):
        for v, shown in (("-1", r"-1\.0"), ("nan", "nan"), ("inf", "inf")):
            with pytest.raises(RuntimeError, match=r"--%s must be finite and >= 0 \(got %s\)" % (flag, shown)):
                check_optim_flags(p.parse_args(["--" + flag, v]), world=1)
    for v, shown in (("-1e-5", "-1e-05"), ("nan", "nan"), ("inf", "inf")):
        with pytest.raises(RuntimeError, match=r"--lr_min must be finite and >= 0 \(got %s\)" % shown):
            check_optim_flags(p.parse_args(COSINE + ["--lr_min=" + v]), world=1)
    with pytest.raises(RuntimeError, match=r"--warmup_steps must be >= 0 \(got -2\)"):
        check_optim_flags(p.parse_args(["--warmup_steps", "-2"]), world=1)
    with pytest.raises(RuntimeError, match=r"--lr_decay_epochs must be >= 0 \(got -1\)"):
        check_optim_flags(p.parse_args(["--lr_decay_epochs", "-1"]), world=1)
    with pytest.raises(RuntimeError, match=r"cosine needs --lr_decay_epochs >= 1 \(got 0\)"):
        check_optim_flags(p.parse_args(["--lr_schedule", "cosine"]), world=1)
    # T = 2 epochs x 8 steps = 16 <= W
    for W in ("16", "40"):
        with pytest.raises(RuntimeError, match=r"--lr_decay_epochs 2 x 8 steps per epoch = 16 steps must exceed --warmup_steps %s" % W):
            check_optim_flags(p.parse_args(COSINE + ["--warmup_steps", W]), world=1)
    check_optim_flags(p.parse_args(COSINE + ["--warmup_steps", "15"]), world=1)
    with pytest.raises(RuntimeError, match=r"--lr_decay_epochs 3 is the span of --lr_schedule cosine \(got --lr_schedule step\)"):
        check_optim_flags(p.parse_args(["--lr_decay_epochs", "3"]), world=1)
    with pytest.raises(RuntimeError, match=r"--lr_min 1e-05 is the end of --lr_schedule cosine"):
        check_optim_flags(p.parse_args(["--lr_min", "1e-5"]), world=1)


@pytest.mark.parametrize("args,named", [(["--adamw_decay", "0.05"], "--adamw_decay 0.05"), (["--clip_grad_norm", "2"], "--clip_grad_norm 2.0"),
                                        (COSINE, "--lr_schedule cosine"), (["--warmup_steps", "4"], "--warmup_steps 4"),
                                        (COSINE + ["--lr_min", "1e-5"], "--lr_schedule cosine")])
def test_check_optim_flags_one_rank_only(args, named):
    p = build_parser('0')
    check_optim_flags(p.parse_args(args), world=1)
    with pytest.raises(RuntimeError, match=r"%s runs on one rank only \(got 2 ranks\)" % named):
        check_optim_flags(p.parse_args(args), world=2)


def test_optim_recipe_counts_the_cosine_in_steps():
    from facl_amd.train_common import optim_recipe
    p = build_parser('0')
    assert optim_recipe(p.parse_args([]), 8) == dict(weight_decay=0.0, max_grad_norm=0.0, schedule="step", warmup_steps=0, lr_min=0.0)
    kw = optim_recipe(p.parse_args(COSINE + ["--warmup_steps", "3", "--adamw_decay", "0.05", "--clip_grad_norm", "1.5"]), 7)
    assert kw == dict(weight_decay=0.05, max_grad_norm=1.5, schedule="cosine", warmup_steps=3, lr_min=0.0, decay_steps=14)
    with pytest.raises(RuntimeError, match="must exceed --warmup_steps 3"):
        optim_recipe(p.parse_args(COSINE + ["--warmup_steps", "3"]), 1)     # a split of one step per epoch, known only on disk


# ---- 3: state compatibility --------------------------------------------------------------------------------------------------
BASE = ["--batchSize", "4", "--neg_queue", "16", "--key_encoder", "1", "--save_root_dir", "a"]


def _old_state(opt, drop=()):
    """A state as the code before the recipe flags wrote it: no entry for any of the six."""
    flags = {k: v for k, v in ts.flags_of(opt).items() if k not in ts.LATER_FLAG_DEFAULTS and k not in drop}
    return ts.assemble(1, 16, flags, {}, {}, {"queue": None, "key_encoder": None, "swav": None}, ts.capture_rng())


def test_a_state_from_before_the_flags_loads_as_their_defaults(tmp_path):
    p = build_parser('0')
    opt = p.parse_args(BASE)
    path = ts.state_path(str(tmp_path), 1)
    ts.write_atomic(_old_state(opt), path)
    assert not set(ts.LATER_FLAG_DEFAULTS) & set(__import__("torch").load(path, weights_only=True)["flags"])
    back = ts.load_state(path)
    assert back["format"] == ts.FORMAT == 1
    assert {k: back["flags"][k] for k in ts.LATER_FLAG_DEFAULTS} == ts.LATER_FLAG_DEFAULTS
    ts.check_compatible(back["flags"], opt)
    with pytest.raises(RuntimeError, match=r"--clip_grad_norm 1\.0 \(the state: 0\.0\)"):
        ts.check_compatible(back["flags"], p.parse_args(BASE + ["--clip_grad_norm", "1"]))
    ts.write_atomic(_old_state(opt, drop=("key_momentum",)), path)
    with pytest.raises(RuntimeError, match=r"lacks flags\.key_momentum") as e:
        ts.load_state(path)
    assert "clip_grad_norm" not in str(e.value)
    # a state of today carries the six, and each of them pins the resumed run
    saved = ts.flags_of(p.parse_args(BASE + COSINE + ["--warmup_steps", "2"]))
    assert saved["lr_schedule"] == "cosine" and saved["lr_decay_epochs"] == 2 and saved["warmup_steps"] == 2
    with pytest.raises(RuntimeError, match=r"--warmup_steps 3 \(the state: 2\)"):
        ts.check_compatible(saved, p.parse_args(BASE + COSINE + ["--warmup_steps", "3"]))


# ---- 4: the entries refuse before the device -------------------------------------------------------------------------------------
def test_entries_refuse_a_bad_recipe_before_the_device(tmp_path, monkeypatch):
    """No device here: a refusal that came after the device was touched would fail in another way."""
    from facl_amd import cn3d_train_apperance_GL, cn3d_train_motion_GL, finetune
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    run = ["--synthetic", "1", "--nepoch", "1", "--batchSize", "4", "--save_root_dir", str(tmp_path / "ck")]
    for entry in (cn3d_train_motion_GL, cn3d_train_apperance_GL, finetune):
        with pytest.raises(RuntimeError, match=r"--clip_grad_norm must be finite and >= 0 \(got -1\.0\)"):
            entry.main(run + ["--clip_grad_norm", "-1"])
        with pytest.raises(RuntimeError, match="cosine needs --lr_decay_epochs >= 1"):
            entry.main(run + ["--lr_schedule", "cosine"])
        with pytest.raises(RuntimeError, match="must exceed --warmup_steps 8"):
            entry.main(run + ["--lr_schedule", "cosine", "--lr_decay_epochs", "1", "--warmup_steps", "8"])
        with pytest.raises(RuntimeError, match="--lr_min 0.001 is the end of --lr_schedule cosine"):
            entry.main(run + ["--lr_min", "1e-3"])
    monkeypatch.setenv("WORLD_SIZE", "2")
    for entry in (cn3d_train_motion_GL, cn3d_train_apperance_GL):
        with pytest.raises(RuntimeError, match=r"--adamw_decay 0\.05 runs on one rank only"):
            entry.main(run + ["--adamw_decay", "0.05"])
    assert not (tmp_path / "ck").exists()


# ---- the C ABI: declared, bound, exported, and its refusals (GPU test 7 runs the same calls beside a device) -----------------
NEW = {"facl_grad_sqnorm": 5, "facl_adam_prep_ex": 13, "facl_adamw_apply": 13}


def _lib():
    from facl_amd import _lib, build
    build.build()
    return _lib, _lib.load_library()


def test_symbols_are_declared_bound_and_exported():
    _l, lib = _lib()
    hdr = open(os.path.join(ROOT, "include", "facl_hip.h")).read()
    assert re.search(r"#define\s+FACL_LR_STEP\s+0", hdr) and re.search(r"#define\s+FACL_LR_COSINE\s+1", hdr)
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for s, nargs in NEW.items():
        m = re.search(r"int\s+%s\s*\(([^)]*)\)" % s, hdr)
        assert m, s
        assert s in _l.SIGNATURES and hasattr(lib, s), s
        assert len(m.group(1).split(",")) == len(_l.SIGNATURES[s]) == nargs, s
    from facl_amd import optim
    assert optim.SCHEDULES == {"step": 0, "cosine": 1}


def abi_refusals(lib):
    """Every refusal of the three entries; nothing is launched and no address is dereferenced.  Shared with the GPU module."""
    def tables(nt, n=8, null_at=None, which=0):
        addr = [[4096 + 64 * i for i in range(nt)] for _ in range(4)]
        if null_at is not None:
            addr[which][null_at] = None
        arr = ctypes.c_void_p * max(nt, 1)
        return [arr(*a) for a in addr], (ctypes.c_int * max(nt, 1))(*([n] * nt)), (ctypes.c_int * max(nt, 1))(*([1] * nt))

    some = ctypes.c_void_p(8192)                              # a non-NULL device address that no refused call reads
    (P, G, M, V), N, D = tables(65)
    for nt in (0, 65, -1):
        assert lib.facl_grad_sqnorm(nt, G, N, some, None) == E_SHAPE, nt
        assert lib.facl_adamw_apply(nt, P, G, M, V, N, D, some, 0.5, 0.999, 1e-6, 0.0, None) == E_SHAPE, nt
    (P, G, M, V), N, D = tables(3)
    for bad in (0, -5):
        N[1] = bad
        assert lib.facl_grad_sqnorm(3, G, N, some, None) == E_SHAPE
        assert lib.facl_adamw_apply(3, P, G, M, V, N, D, some, 0.5, 0.999, 1e-6, 0.0, None) == E_SHAPE
    N[1] = 8
    for wd in (-0.01, float("nan")):
        assert lib.facl_adamw_apply(3, P, G, M, V, N, D, some, 0.5, 0.999, 1e-6, wd, None) == E_SHAPE, wd
    # NULL arrays and NULL entries
    assert lib.facl_grad_sqnorm(3, None, N, some, None) == E_NULL and lib.facl_grad_sqnorm(3, G, None, some, None) == E_NULL
    assert lib.facl_grad_sqnorm(3, G, N, None, None) == E_NULL
    for k in range(7):
        args = [P, G, M, V, N, D, some]
        args[k] = None
        assert lib.facl_adamw_apply(3, *args, 0.5, 0.999, 1e-6, 0.0, None) == E_NULL, k
    for which in range(4):
        for at in (0, 2):
            (p, g, m, v), n, d = tables(3, null_at=at, which=which)
            assert lib.facl_adamw_apply(3, p, g, m, v, n, d, some, 0.5, 0.999, 1e-6, 0.0, None) == E_NULL, (which, at)
            if which == 1:
                assert lib.facl_grad_sqnorm(3, g, n, some, None) == E_NULL, at
    # facl_adam_prep_ex(lr, step, b1, b2, partial, npartial, max_norm, schedule, W, T, lr_min, consts, stream)
    prep = lambda *a: lib.facl_adam_prep_ex(*a, None)
    ok = [some, some, 0.5, 0.999, some, 4, 1.0, 0, 0, 0, 0.0, some]
    for k in (0, 1, 4, 11):
        a = list(ok)
        a[k] = None
        assert prep(*a) == E_NULL, k
    for k, vals in ((5, (-1,)), (6, (0.0, -1.0, float("nan"))), (7, (2, -1)), (8, (-1,)), (10, (-1e-5, float("nan")))):
        for val in vals:
            a = list(ok)
            a[k] = val
            assert prep(*a) == E_SHAPE, (k, val)
    for W, T in ((0, 0), (5, 5), (5, 3)):                      # T <= W under cosine
        a = list(ok)
        a[7], a[8], a[9] = 1, W, T
        assert prep(*a) == E_SHAPE, (W, T)


def test_abi_refusals():
    abi_refusals(_lib()[1])


def test_timing_tool_keeps_the_blocks_it_does_not_produce(tmp_path):
    import importlib.util
    import json
    spec = importlib.util.spec_from_file_location("time_optim_recipe", os.path.join(ROOT, "tools", "time_optim_recipe.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    out = tmp_path / "o.json"
    out.write_text(json.dumps({"bench_ab": {"parent": [1]}, "off_graph_ms": 1.0}))
    tool.write_results(str(out), {"off_graph_ms": 3.0})
    assert json.loads(out.read_text()) == {"bench_ab": {"parent": [1]}, "off_graph_ms": 3.0}
    with open(os.path.join(ROOT, "profiles", "optim_recipe.json")) as f:
        recorded = json.load(f)
    assert len(recorded["bench_ab"]["parent"]) == len(recorded["bench_ab"]["this"]) == 3
    assert recorded["on_minus_off_us"] == 1e3 * (recorded["on_graph_ms"] - recorded["off_graph_ms"])
    k = recorded["kernel_only"]
    assert k["on_minus_off_us"] == 1e3 * (k["optimizer_on_ms"] - k["optimizer_off_ms"])
    assert recorded["clip_coef"] <= 1.0 and recorded["grad_norm"] > 0.0


def test_fused_adam_refuses_a_bad_recipe_on_the_host():
    """No CPU path for the recipe either, and a decay mask must name every tensor."""
    import torch
    from facl_amd.optim import FusedAdam
    with pytest.raises(RuntimeError, match="GPU only"):
        FusedAdam([torch.nn.Parameter(torch.zeros(3))], weight_decay=0.1)
    with pytest.raises(ValueError, match="decay_mask has 2 entries for 1 tensors"):
        FusedAdam([torch.nn.Parameter(torch.zeros(3))], decay_mask=[True, False])
