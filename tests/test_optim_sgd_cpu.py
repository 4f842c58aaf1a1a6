"""--optim sgd / lars, host side: the training entries' parsers (train_flags.train_parser / finetune_train_parser: build_parser
and finetune_parser, which the extraction and prediction entries share and tests/golden/train_flag_defaults.json records, plus
the optimizer's five flags) and their defaults, every refusal of the new flags with its message, the state file's
compatibility with states from before the flags, the C ABI declarations against _lib.SIGNATURES and their refusals (all before a
launch, so they run without a device), and the fp64 reference of the update rule (tests/sgd_reference.py) against
torch.optim.SGD in fp64 on the CPU, which pins what the GPU tests compare the kernels with."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from facl_amd import train_flags as tf
from facl_amd import train_state as ts
from sgd_reference import lars_step, sgd_step

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_SHAPE, E_NULL = -1, -2
NEW_FLAGS = {"optim": "adam", "sgd_momentum": 0.9, "sgd_nesterov": 0, "sgd_weight_decay": 0.0, "lars_eta": 0.001}


# ---- 1: the parser and the checks ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("parser", [lambda: tf.train_parser('0'), tf.finetune_train_parser])
def test_parser_defaults(parser):
    p = parser()
    o = p.parse_args([])
    assert {k: getattr(o, k) for k in NEW_FLAGS} == NEW_FLAGS
    assert (o.momentum, o.weight_decay) == (0.9, 0.0008)                          # parsed and unread, as before
    helps = {a.dest: a.help for a in p._actions}
    assert "never read" in helps["momentum"] and "--sgd_momentum" in helps["momentum"]
    assert "never read" in helps["weight_decay"] and "--sgd_weight_decay" in helps["weight_decay"]
    with pytest.raises(SystemExit):
        p.parse_args(["--optim", "lamb"])
    with pytest.raises(SystemExit):
        p.parse_args(["--sgd_nesterov", "2"])
    assert tf.OPTIMIZER_FLAG_DEFAULTS == NEW_FLAGS == ts.OPTIMIZER_FLAG_DEFAULTS


def test_the_shared_parsers_are_the_training_parsers_without_the_five():
    """build_parser / finetune_parser (extraction, prediction, the recorded parser) carry none of the five and their help is as it
    was; the entries' parsers add exactly the five; a namespace without them is an Adam run."""
    for shared, entry in ((tf.build_parser('0'), tf.train_parser('0')), (tf.finetune_parser(), tf.finetune_train_parser())):
        a, b = vars(shared.parse_args([])), vars(entry.parse_args([]))
        assert set(b) - set(a) == set(NEW_FLAGS) and all(b[k] == v for k, v in a.items())
        assert {x.dest: x.help for x in shared._actions}["momentum"] == "momentum (SGD only)"
    bare = tf.build_parser('0').parse_args([])
    assert vars(tf.optimizer_flags(bare)) == NEW_FLAGS and tf.describe_optimizer(bare) is None
    tf.check_train_flags(bare, 2)
    assert {k: ts.flags_of(bare)[k] for k in NEW_FLAGS} == NEW_FLAGS


def _check(args, world=1):
    tf.check_train_flags(tf.train_parser('0').parse_args(args), world)


def test_accepted_configurations():
    _check([])
    _check([], world=2)                                                           # the defaults: nothing to refuse
    _check(["--optim", "sgd"])
    _check(["--optim", "sgd", "--sgd_momentum", "0", "--sgd_nesterov", "1", "--sgd_weight_decay", "1e-4", "--lars_eta", "0"])
    _check(["--optim", "lars", "--sgd_weight_decay", "1e-4", "--clip_grad_norm", "1", "--warmup_steps", "2",
            "--lr_schedule", "cosine", "--lr_decay_epochs", "2", "--lr_min", "1e-5"])
    tf.check_finetune_train_flags(tf.finetune_train_parser().parse_args(["--optim", "sgd", "--sgd_nesterov", "1"]), 1)


@pytest.mark.parametrize("optim", ["sgd", "lars"])
def test_refusals_under_sgd_and_lars(optim):
    base = ["--optim", optim]
    with pytest.raises(RuntimeError, match=r"^--optim %s runs on one rank only \(got 2 ranks\): the optimizer has never run "
                                           r"data-parallel$" % optim):
        _check(base, world=2)
    with pytest.raises(RuntimeError, match=r"^--adamw_decay 0\.05 is the decoupled decay of --optim adam: --optim %s takes "
                                           r"--sgd_weight_decay$" % optim):
        _check(base + ["--adamw_decay", "0.05"])
    for v, shown in (("1", r"1\.0"), ("-0.1", r"-0\.1"), ("nan", "nan"), ("1.5", r"1\.5")):
        with pytest.raises(RuntimeError, match=r"^--sgd_momentum must be in \[0, 1\) \(got %s\)$" % shown):
            _check(base + ["--sgd_momentum=" + v])
    for flag in ("sgd_weight_decay", "lars_eta"):
        for v, shown in (("-1e-4", r"-0\.0001"), ("nan", "nan"), ("inf", "inf")):
            with pytest.raises(RuntimeError, match=r"^--%s must be finite and >= 0 \(got %s\)$" % (flag, shown)):
                _check(base + ["--%s=%s" % (flag, v)])
    if optim == "lars":
        with pytest.raises(RuntimeError, match=r"^--optim lars needs --lars_eta > 0 \(got 0\.0\)"):
            _check(base + ["--lars_eta", "0"])


@pytest.mark.parametrize("args,named", [(["--sgd_momentum", "0.5"], "--sgd_momentum 0.5"), (["--sgd_nesterov", "1"], "--sgd_nesterov 1"),
                                        (["--sgd_weight_decay", "1e-4"], "--sgd_weight_decay 0.0001"),
                                        (["--lars_eta", "0.01"], "--lars_eta 0.01")])
def test_refusals_under_adam(args, named):
    with pytest.raises(RuntimeError, match=r"^%s belongs to --optim sgd / lars \(got --optim adam, which does not read it\)$" % named):
        _check(args)
    with pytest.raises(RuntimeError, match="belongs to --optim sgd / lars"):
        tf.check_finetune_train_flags(tf.finetune_train_parser().parse_args(args), 1)
    _check(["--optim", "sgd"] + args)


def test_entries_refuse_before_the_device(tmp_path, monkeypatch):
    """No device here: a refusal that came after the device was touched would fail in another way."""
    from facl_amd import cn3d_train_apperance_GL, cn3d_train_motion_GL, finetune
    run = ["--synthetic", "1", "--nepoch", "1", "--batchSize", "4", "--save_root_dir", str(tmp_path / "ck")]
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    for entry in (cn3d_train_motion_GL, cn3d_train_apperance_GL, finetune):
        with pytest.raises(RuntimeError, match=r"--sgd_momentum must be in \[0, 1\)"):
            entry.main(run + ["--optim", "sgd", "--sgd_momentum", "1"])
        with pytest.raises(RuntimeError, match="--optim lars takes --sgd_weight_decay"):
            entry.main(run + ["--optim", "lars", "--adamw_decay", "0.1"])
        with pytest.raises(RuntimeError, match="--lars_eta 0.5 belongs to --optim sgd / lars"):
            entry.main(run + ["--lars_eta", "0.5"])
    monkeypatch.setenv("WORLD_SIZE", "2")
    for entry in (cn3d_train_motion_GL, cn3d_train_apperance_GL):
        for optim in ("sgd", "lars"):
            with pytest.raises(RuntimeError, match=r"--optim %s runs on one rank only \(got 2 ranks\)" % optim):
                entry.main(run + ["--optim", optim])
    assert not (tmp_path / "ck").exists()


def test_the_optimizer_line():
    p = tf.train_parser('0')
    assert tf.describe_optimizer(p.parse_args([])) is None
    assert tf.describe_optimizer(p.parse_args(["--optim", "sgd", "--sgd_nesterov", "1"])) \
        == "optimizer: sgd momentum 0.9 nesterov 1 weight decay 0"
    assert tf.describe_optimizer(p.parse_args(["--optim", "lars", "--sgd_weight_decay", "1e-4", "--sgd_momentum", "0.5"])) \
        == "optimizer: lars momentum 0.5 nesterov 0 weight decay 0.0001 eta 0.001"


# ---- 2: the state file -----------------------------------------------------------------------------------------------------------
BASE = ["--batchSize", "4", "--save_root_dir", "a"]


def test_the_flags_are_trajectory_flags_with_the_parser_defaults():
    """The defaults a state without the flags gets are the parser's.  They stand in train_state.OPTIMIZER_FLAG_DEFAULTS, not in
    LATER_FLAG_DEFAULTS: every key of that dict must be a flag of build_parser (tests/test_optim_recipe_cpu.py), and build_parser's
    recorded actions do not hold the five."""
    o = tf.train_parser('0').parse_args([])
    for k, v in NEW_FLAGS.items():
        assert k in ts.TRAJECTORY_FLAGS and ts.OPTIMIZER_FLAG_DEFAULTS[k] == v == getattr(o, k), k
    assert not set(NEW_FLAGS) & set(ts.LATER_FLAG_DEFAULTS)
    assert ts.FORMAT == 1


def test_a_state_from_before_the_flags_resumes_as_an_adam_run(tmp_path):
    p = tf.train_parser('0')
    opt = p.parse_args(BASE)
    flags = {k: v for k, v in ts.flags_of(opt).items() if k not in NEW_FLAGS}
    path = ts.state_path(str(tmp_path), 1)
    ts.write_atomic(ts.assemble(1, 16, flags, {}, {}, {"queue": None, "key_encoder": None, "swav": None}, ts.capture_rng()), path)
    assert not set(NEW_FLAGS) & set(torch.load(path, weights_only=True)["flags"])
    back = ts.load_state(path)
    assert {k: back["flags"][k] for k in NEW_FLAGS} == NEW_FLAGS
    ts.check_compatible(back["flags"], opt)                                        # accepted for a default run
    with pytest.raises(RuntimeError, match=r"--optim 'sgd' \(the state: 'adam'\)"):
        ts.check_compatible(back["flags"], p.parse_args(BASE + ["--optim", "sgd"]))
    saved = ts.flags_of(p.parse_args(BASE + ["--optim", "lars", "--sgd_weight_decay", "1e-4"]))
    with pytest.raises(RuntimeError, match=r"--optim 'sgd' \(the state: 'lars'\)"):
        ts.check_compatible(saved, p.parse_args(BASE + ["--optim", "sgd", "--sgd_weight_decay", "1e-4"]))
    with pytest.raises(RuntimeError, match=r"--lars_eta 0\.01 \(the state: 0\.001\)"):
        ts.check_compatible(saved, p.parse_args(BASE + ["--optim", "lars", "--sgd_weight_decay", "1e-4", "--lars_eta", "0.01"]))


# ---- 3: the C ABI ----------------------------------------------------------------------------------------------------------------
NEW = {"facl_tensor_sqnorms": 7, "facl_sgd_prep": 19, "facl_sgd_apply": 12}


def _lib():
    from facl_amd import _lib, build
    build.build()
    return _lib, _lib.load_library()


def test_symbols_are_declared_bound_and_exported():
    _l, lib = _lib()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "facl_hip.h")).read(), flags=re.S)
    for s, nargs in NEW.items():
        m = re.search(r"int\s+%s\s*\(([^)]*)\)" % s, hdr)
        assert m, s
        assert s in _l.SIGNATURES and hasattr(lib, s), s
        assert len(m.group(1).split(",")) == len(_l.SIGNATURES[s]) == nargs, s


def sgd_abi_refusals(lib):
    """Every refusal of the three entries; nothing is launched and no address is dereferenced.  Shared with the GPU module."""
    def tables(nt, n=8, null_at=None, which=0):
        addr = [[4096 + 64 * i for i in range(nt)] for _ in range(3)]
        if null_at is not None:
            addr[which][null_at] = None
        arr = ctypes.c_void_p * max(nt, 1)
        return [arr(*a) for a in addr], (ctypes.c_int * max(nt, 1))(*([n] * nt)), (ctypes.c_int * max(nt, 1))(*([1] * nt))

    some = ctypes.c_void_p(8192)                              # a non-NULL device address that no refused call reads
    sq = lambda nt, p, g, n, pp, pg: lib.facl_tensor_sqnorms(nt, p, g, n, pp, pg, None)
    ap = lambda nt, p, g, b, n, d, consts=some, trust=None, mu=0.9, wd=0.0, nest=0: \
        lib.facl_sgd_apply(nt, p, g, b, n, d, consts, trust, mu, wd, nest, None)
    (P, G, B), N, D = tables(65)
    for nt in (0, 65, -1):
        assert sq(nt, P, G, N, some, some) == E_SHAPE and ap(nt, P, G, B, N, D) == E_SHAPE, nt
    (P, G, B), N, D = tables(3)
    for bad in (0, -5):
        N[1] = bad
        assert sq(3, P, G, N, some, some) == E_SHAPE and ap(3, P, G, B, N, D) == E_SHAPE
    N[1] = 8
    for mu in (-0.1, 1.0, 1.5, float("nan")):
        assert ap(3, P, G, B, N, D, mu=mu) == E_SHAPE, mu
    for wd in (-0.01, float("nan")):
        assert ap(3, P, G, B, N, D, wd=wd) == E_SHAPE, wd
    for k in range(5):
        a = [P, G, N, some, some]
        a[k] = None
        assert sq(3, *a) == E_NULL, k
    for k in range(6):
        a = [P, G, B, N, D, some]
        a[k] = None
        assert ap(3, *a) == E_NULL, k
    for which in range(3):
        for at in (0, 2):
            (p, g, b), n, d = tables(3, null_at=at, which=which)
            assert ap(3, p, g, b, n, d) == E_NULL, (which, at)
            if which < 2:
                assert sq(3, p, g, n, some, some) == E_NULL, (which, at)
    # facl_sgd_prep(lr, step, partial_g, partial_p, npartial, nt, n, mask, max_norm, clip_on, schedule, W, T, lr_min, eta, wd,
    #               consts, trust, stream); 3 tensors of 8 elements are 3 chunks
    prep = lambda *a: lib.facl_sgd_prep(*a, None)
    lars = [some, some, some, some, 3, 3, N, D, 1.0, 1, 0, 0, 0, 0.0, 1e-3, 1e-4, some, some]
    for k in (0, 1, 2, 6, 7, 16, 17):
        a = list(lars)
        a[k] = None
        assert prep(*a) == E_NULL, k
    plain = [some, some, None, None, 0, 0, None, None, 0.0, 0, 0, 0, 0, 0.0, 0.0, 0.0, some, None]
    for k in (0, 1, 16):
        a = list(plain)
        a[k] = None
        assert prep(*a) == E_NULL, k
    a = list(plain)
    a[9], a[8] = 1, 1.0                                       # clipping needs the gradient partials
    assert prep(*a) == E_NULL
    for k, vals in ((4, (-1, 2, 4)), (5, (0, 65, -1)), (8, (0.0, -1.0, float("nan"))), (10, (2, -1)), (11, (-1,)),
                    (13, (-1e-5, float("nan"))), (14, (-1e-3, float("nan"))), (15, (-1e-4, float("nan")))):
        for val in vals:
            a = list(lars)
            a[k] = val
            assert prep(*a) == E_SHAPE, (k, val)
    for W, T in ((0, 0), (5, 5), (5, 3)):                      # T <= W under cosine
        a = list(lars)
        a[10], a[11], a[12] = 1, W, T
        assert prep(*a) == E_SHAPE, (W, T)
    N[1] = 0
    assert prep(*lars) == E_SHAPE
    N[1] = 8


def test_abi_refusals():
    sgd_abi_refusals(_lib()[1])


def test_fused_sgd_refuses_on_the_host():
    from facl_amd.optim import FusedSGD
    w = [torch.nn.Parameter(torch.zeros(3))]
    with pytest.raises(RuntimeError, match="GPU only"):
        FusedSGD(w, lr=0.1)
    with pytest.raises(ValueError, match="decay_mask has 2 entries for 1 tensors"):
        FusedSGD(w, lr=0.1, decay_mask=[True, False])


# ---- 4: the fp64 reference ---------------------------------------------------------------------------------------------------------
SHAPES = [(7, 5), (11,), (3, 4, 2), (1,)]
MASK = [True, False, True, False]
LR, MU, WD = 0.05, 0.9, 1e-2


def _data(steps):
    r = np.random.RandomState(11)
    p0 = [r.randn(*s) for s in SHAPES]
    grads = [[r.randn(*s) for s in SHAPES] for _ in range(steps)]
    return p0, grads


@pytest.mark.parametrize("nesterov", [False, True])
def test_the_fp64_reference_reproduces_torch_sgd(nesterov):
    p0, grads = _data(4)
    tp = [torch.nn.Parameter(torch.from_numpy(a.copy())) for a in p0]
    opt = torch.optim.SGD([{"params": [t for t, m in zip(tp, MASK) if m], "weight_decay": WD},
                           {"params": [t for t, m in zip(tp, MASK) if not m], "weight_decay": 0.0}],
                          lr=LR, momentum=MU, dampening=0, nesterov=nesterov)
    p, buf = [a.copy() for a in p0], [np.zeros_like(a) for a in p0]
    for g in grads:
        for t, gi in zip(tp, g):
            t.grad = torch.from_numpy(gi.copy())
        opt.step()
        sgd_step(p, g, buf, LR, MU, WD, MASK, nesterov)
        for t, a, b in zip(tp, p, buf):
            assert np.abs(t.detach().numpy() - a).max() <= 1e-14 * np.abs(a).max()
            tb = opt.state[t]["momentum_buffer"].numpy()
            assert np.abs(tb - b).max() <= 1e-14 * np.abs(b).max()


def test_the_lars_reference_with_all_masks_off_is_the_sgd_reference():
    p0, grads = _data(4)
    none = [False] * len(SHAPES)
    a, ba = [x.copy() for x in p0], [np.zeros_like(x) for x in p0]
    b, bb = [x.copy() for x in p0], [np.zeros_like(x) for x in p0]
    for g in grads:
        sgd_step(a, g, ba, LR, MU, WD, none, True)
        lars_step(b, g, bb, LR, MU, WD, none, True, eta=1e-3)
    for x, y in zip(a + ba, b + bb):
        assert np.array_equal(x, y)
    # and with a mask on it is another trajectory: the ratio is live
    lars_step(b, grads[0], bb, LR, MU, WD, MASK, True, eta=1e-3)
    sgd_step(a, grads[0], ba, LR, MU, WD, MASK, True)
    assert not np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
