"""The training-state file (facl_amd/train_state.py), host side only: atomic write, discovery, pruning, the option check and
the round trip of a state -- generators included -- through torch.load(weights_only=True).  No device is touched."""
import os
import random

import numpy as np
import pytest
import torch

from facl_amd import train_state as ts
from facl_amd.train_common import build_parser, check_state_flags


def _touch(folder, *names):
    for n in names:
        with open(os.path.join(str(folder), n), "wb") as f:
            f.write(b"x")


# ---- write_atomic --------------------------------------------------------------------------------------------------------
def test_write_atomic_leaves_no_temporary(tmp_path):
    path = ts.state_path(str(tmp_path), 3)
    ts.write_atomic({"a": torch.arange(4)}, path)
    assert os.listdir(str(tmp_path)) == ["state_3.pth"]
    assert torch.equal(torch.load(path, weights_only=True)["a"], torch.arange(4))


def test_write_atomic_keeps_the_old_file_when_the_save_raises(tmp_path, monkeypatch):
    path = ts.state_path(str(tmp_path), 3)
    ts.write_atomic({"a": torch.arange(4)}, path)
    before = open(path, "rb").read()

    def half_written(obj, f, *args, **kwargs):
        f.write(b"half a file")
        raise OSError("disk full")

    monkeypatch.setattr(torch, "save", half_written)
    with pytest.raises(OSError, match="disk full"):
        ts.write_atomic({"a": torch.arange(8)}, path)
    monkeypatch.undo()
    assert open(path, "rb").read() == before
    assert os.listdir(str(tmp_path)) == ["state_3.pth"]
    assert ts.find_latest(str(tmp_path)) == path


# ---- find_latest / prune -------------------------------------------------------------------------------------------------
def test_find_latest_orders_by_epoch_number_and_ignores_other_files(tmp_path):
    assert ts.find_latest(str(tmp_path)) is None
    assert ts.find_latest(str(tmp_path / "not_there")) is None
    _touch(tmp_path, "state_9.pth", "state_10.pth", "state_2.pth")
    _touch(tmp_path, "state_11.pth.tmp123", "state_12.pth.tmp", "corr_GL_95.pth", "corr_GL_95_key.pth", "state_x.pth",
           "state_13.pt", "xstate_14.pth", "state_15.pth.bak", "state_.pth")
    assert ts.find_latest(str(tmp_path)) == os.path.join(str(tmp_path), "state_10.pth")
    assert [e for e, _ in ts.list_states(str(tmp_path))] == [2, 9, 10]


def test_prune_keeps_the_newest(tmp_path):
    names = ["state_%d.pth" % e for e in (1, 5, 9, 10, 11)]
    other = ["state_12.pth.tmp7", "corr_GL_0.pth"]
    _touch(tmp_path, *names, *other)
    assert ts.prune(str(tmp_path), 0) == []                                   # 0 keeps all
    assert sorted(os.listdir(str(tmp_path))) == sorted(names + other)
    gone = ts.prune(str(tmp_path), 2)
    assert sorted(os.path.basename(p) for p in gone) == ["state_1.pth", "state_5.pth", "state_9.pth"]
    assert sorted(os.listdir(str(tmp_path))) == sorted(["state_10.pth", "state_11.pth"] + other)
    assert ts.prune(str(tmp_path), 5) == []


# ---- check_compatible ----------------------------------------------------------------------------------------------------
BASE = ["--batchSize", "4", "--neg_queue", "16", "--key_encoder", "1", "--save_root_dir", "a"]


def test_check_compatible_accepts_the_options_that_may_differ():
    p = build_parser('0')
    saved = ts.flags_of(p.parse_args(BASE))
    assert set(saved) == set(ts.TRAJECTORY_FLAGS) and saved["group_radius"] is None
    ts.check_compatible(saved, p.parse_args(BASE))
    ts.check_compatible(saved, p.parse_args(
        ["--batchSize", "4", "--neg_queue", "16", "--key_encoder", "1", "--nepoch", "7", "--save_root_dir", "b", "--log_file", "l",
         "--graph", "0", "--prefetch", "0", "--resident", "1", "--resident_max_gb", "2", "--knn_every", "3", "--knn_k", "5",
         "--knn_T", "0.5", "--main_gpu", "1", "--workers", "4", "--save_state_every", "2", "--keep_states", "9", "--resume", "auto"]))


def test_check_compatible_names_every_differing_flag_with_both_values():
    p = build_parser('0')
    saved = ts.flags_of(p.parse_args(BASE))
    with pytest.raises(RuntimeError) as e:
        ts.check_compatible(saved, p.parse_args(["--batchSize", "8", "--neg_queue", "16", "--key_encoder", "1",
                                                 "--loss_mask", "exclude", "--learning_rate", "0.001", "--group_radius", "0.1"]))
    msg = str(e.value)
    for name, new, old in (("batchSize", "8", "4"), ("loss_mask", "'exclude'", "'zero'"), ("learning_rate", "0.001", "0.0003"),
                           ("group_radius", "0.1", "None")):
        assert "--%s %s (the state: %s)" % (name, new, old) in msg, msg
    assert "neg_queue" not in msg and "nepoch" not in msg
    for flag in ts.TRAJECTORY_FLAGS:                         # every one of them is checked
        other = dict(saved)
        other[flag] = "something else"
        with pytest.raises(RuntimeError, match="--%s " % flag):
            ts.check_compatible(other, p.parse_args(BASE))


def test_check_state_flags():
    p = build_parser('0')
    o = p.parse_args([])
    assert (o.save_state_every, o.keep_states, o.resume) == (0, 2, '')
    check_state_flags(o, world=2)                                              # off: nothing to refuse
    check_state_flags(p.parse_args(["--resume", "auto", "--save_state_every", "1"]), world=1)
    with pytest.raises(RuntimeError, match="--resume auto runs on one rank only"):
        check_state_flags(p.parse_args(["--resume", "auto"]), world=2)
    with pytest.raises(RuntimeError, match="--save_state_every 5 runs on one rank only"):
        check_state_flags(p.parse_args(["--save_state_every", "5"]), world=2)
    with pytest.raises(RuntimeError, match=">= 0"):
        check_state_flags(p.parse_args(["--keep_states", "-1"]), world=1)


# ---- a whole state -------------------------------------------------------------------------------------------------------
def _draws(np_global, py, view, gen):
    """The next draws of every generator a state holds (the CPU generator `gen` stands in for the entry's device one)."""
    a = np.arange(10)
    np_global.shuffle(a)
    return (a.tolist(), np_global.standard_normal(3).tolist(), py.random(), py.gauss(0, 1), py.gauss(0, 1), torch.rand(3).tolist(),
            view.randint(0, 1000, 5).tolist(), view.standard_normal(3).tolist(), torch.rand(3, generator=gen).tolist())


def _assert_same(a, b, where="state"):
    assert type(a) is type(b), where
    if torch.is_tensor(a):
        assert a.dtype == b.dtype and a.device.type == "cpu" and torch.equal(a, b), where
    elif isinstance(a, dict):
        assert list(a) == list(b), where
        for k in a:
            _assert_same(a[k], b[k], "%s.%s" % (where, k))
    elif isinstance(a, list):
        assert len(a) == len(b), where
        for i, (x, y) in enumerate(zip(a, b)):
            _assert_same(x, y, "%s[%d]" % (where, i))
    else:
        assert a == b, where


def test_a_state_round_trips_through_weights_only_load(tmp_path):
    p = build_parser('0')
    opt = p.parse_args(BASE)
    random.seed(5)
    np.random.seed(6)
    torch.manual_seed(7)
    view, gen = np.random.RandomState(2000), torch.Generator()
    gen.manual_seed(1000)
    # every generator mid-stream, the Gaussian ones with a cached second value
    np.random.standard_normal(1), view.standard_normal(1), random.gauss(0, 1), torch.rand(5), torch.rand(5, generator=gen)
    w = torch.nn.Parameter(torch.randn(3, 4))
    model = torch.nn.BatchNorm1d(4).state_dict()                               # an OrderedDict with an int64 buffer
    optim = {"state": {0: {"step": torch.tensor(6.0), "exp_avg": torch.randn(3, 4), "exp_avg_sq": torch.rand(3, 4)}},
             "param_groups": [{"lr": 3e-4, "betas": (0.5, 0.999), "eps": 1e-6, "weight_decay": 0, "amsgrad": False, "params": [0]}]}
    step_state = {"queue": {"buf": torch.randn(16, 8), "state": torch.tensor([8, 16], dtype=torch.int32)},
                  "key_encoder": {"w": w.detach()}, "swav": None}
    state = ts.assemble(1, 6, ts.flags_of(opt), model, optim, step_state, ts.capture_rng(gen, view, None))
    assert state["optimizer"]["state"][0]["exp_avg"].data_ptr() != optim["state"][0]["exp_avg"].data_ptr()     # deep-copied
    path = ts.state_path(str(tmp_path), 1)
    ts.write_atomic(state, path)
    want = _draws(np.random, random, view, gen)

    back = ts.load_state(path)                              # torch.load(map_location="cpu", weights_only=True)
    _assert_same(back, state)
    assert back["epoch"] == 1 and back["steps_done"] == 6 and back["format"] == ts.FORMAT and back["swav"] is None
    ts.check_compatible(back["flags"], opt)
    np.random.seed(0), random.seed(0), torch.manual_seed(0)
    view2, gen2 = np.random.RandomState(0), torch.Generator()
    ts.apply_rng(back["rng"], gen2, view2, None)
    assert _draws(np.random, random, view2, gen2) == want
    with pytest.raises(RuntimeError, match="view_source"):
        ts.apply_rng(back["rng"], gen2, view2, np.random.RandomState(0))


def test_training_entries_refuse_before_the_device(tmp_path, monkeypatch):
    """No device here: a refusal that came after the device was touched would fail in another way."""
    from facl_amd import cn3d_train_apperance_GL, cn3d_train_motion_GL
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    run = ["--synthetic", "1", "--nepoch", "4", "--save_root_dir", str(tmp_path / "ck")]
    for entry, branch in ((cn3d_train_motion_GL, '0'), (cn3d_train_apperance_GL, '1')):
        opt = build_parser(branch).parse_args(BASE)
        good = ts.assemble(1, 16, ts.flags_of(opt), {}, {}, {"queue": None, "key_encoder": None, "swav": None}, ts.capture_rng())
        path = ts.state_path(str(tmp_path), 1)
        ts.write_atomic(good, path)
        with pytest.raises(RuntimeError, match=r"--batchSize 8 \(the state: 4\); --key_momentum 0.5 \(the state: 0.999\)"):
            entry.main(run + ["--batchSize", "8", "--neg_queue", "16", "--key_encoder", "1", "--key_momentum", "0.5", "--resume", path])
        good["format"] += 1
        ts.write_atomic(good, path)
        with pytest.raises(RuntimeError, match="format %d" % good["format"]):
            entry.main(run + BASE[:-2] + ["--resume", path])
        with pytest.raises(RuntimeError, match="does not load"):
            entry.main(run + BASE[:-2] + ["--resume", str(tmp_path / "state_7.pth")])
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(RuntimeError, match="--resume auto runs on one rank only"):
        cn3d_train_motion_GL.main(run + ["--resume", "auto"])
    assert not (tmp_path / "ck").exists()


def test_load_state_refuses_with_the_path(tmp_path):
    opt = build_parser('0').parse_args(BASE)
    good = ts.assemble(0, 3, ts.flags_of(opt), {}, {}, {"queue": None, "key_encoder": None, "swav": None}, ts.capture_rng())
    path = os.path.join(str(tmp_path), "state_0.pth")
    for change, match in ((lambda s: s.update(format=ts.FORMAT + 1), "format %d" % (ts.FORMAT + 1)),
                          (lambda s: s.pop("optimizer"), "lacks optimizer"),
                          (lambda s: s["rng"].pop("numpy"), r"lacks rng\.numpy"),
                          (lambda s: s["flags"].pop("key_momentum"), r"lacks flags\.key_momentum")):
        bad = {k: (dict(v) if isinstance(v, dict) else v) for k, v in good.items()}
        change(bad)
        ts.write_atomic(bad, path)
        with pytest.raises(RuntimeError, match=match) as e:
            ts.load_state(path)
        assert path in str(e.value) and not isinstance(e.value, ts.StateUnreadable)
    torch.save({"net3DV_1.0.weight": torch.zeros(2)}, path)                    # an encoder checkpoint is not a state
    with pytest.raises(RuntimeError, match="not a training state") as e:
        ts.load_state(path)
    assert path in str(e.value)
    with open(path, "wb") as f:
        f.write(b"not an archive")
    with pytest.raises(ts.StateUnreadable) as e:
        ts.load_state(path)
    assert path in str(e.value)
