"""--save_state_every / --resume through the training entry: a run resumed from a state file ends bit-identical to the run that
never stopped -- the returned model, every entry of the last state file (model, Adam moments and step, negative queue and its
{head, valid}, key encoder, every RNG stream) and the printed epoch losses -- with and without graph replay on either side, from
synthetic batches and from clips on disk (resident and through the producer thread); --resume auto; the SwAV queue through
ContrastiveStep.state_dict(); the refusals.  Equality everywhere, no tolerance.

The queue holds L = 16 rows and a step pushes 4: after the 6 steps of two epochs it has wrapped and its head is 8, so a head
reset to 0 or a queue restored as empty changes what epochs 2 and 3 compute."""
import contextlib
import io
import os
import re
import shutil

import numpy as np
import pytest
import torch

from step_factory import step_opt
from synth_tree import assert_same_state, run_train_entry, write_tree

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

BASE = ["--synthetic", "1", "--batchSize", "4", "--num_crop", "4", "--SAMPLE_NUM", "512", "--steps_per_epoch", "3",
        "--neg_queue", "16", "--key_encoder", "1", "--key_momentum", "0.5", "--loss_normalize", "1", "--loss_temperature", "0.1",
        "--loss_mask", "exclude", "--save_state_every", "1", "--keep_states", "0"]


def _run(folder, *extra, base=BASE):
    """One run of the motion entry into `folder`: (the returned model's state_dict on the CPU, what it printed)."""
    return run_train_entry(list(base) + ["--save_root_dir", str(folder)] + [str(a) for a in extra])


def _losses(printed):
    """{epoch: the mean loss as printed}"""
    return {int(e): v for e, v in re.findall(r"epoch: (\d+) loss mode is : 1 --loss: (\S+)", printed)}


def _state(folder, epoch):
    from facl_amd import train_state
    return train_state.load_state(os.path.join(str(folder), "state_%d.pth" % epoch))


def _assert_run_equals(got, want, got_dir, want_dir, epochs=(2, 3), last=3):
    (sd_g, out_g), (sd_w, out_w) = got, want
    assert_same_state(sd_g, sd_w, "model")
    assert_same_state(_state(got_dir, last), _state(want_dir, last), "state_%d" % last)
    lg, lw = _losses(out_g), _losses(out_w)
    assert all(np.isfinite(float(lw[e])) for e in epochs)
    assert {e: lg[e] for e in epochs} == {e: lw[e] for e in epochs}, (lg, lw)


# ---- the shared runs: A never stops, B stops after epoch 1 ---------------------------------------------------------------
@pytest.fixture(scope="module")
def run_a(tmp_path_factory):
    d = tmp_path_factory.mktemp("a")
    return _run(d, "--nepoch", 4, "--graph", 1), d


@pytest.fixture(scope="module")
def runs_b(tmp_path_factory):
    made = {}

    def get(graph):
        if graph not in made:
            d = tmp_path_factory.mktemp("b%d" % graph)
            made[graph] = (_run(d, "--nepoch", 2, "--graph", graph), d)
        return made[graph]
    return get


def test_the_saved_queue_has_wrapped_and_the_state_is_complete(run_a):
    (sd, out), d = run_a
    assert sorted(os.listdir(str(d))) == ["corr_GL_0.pth", "corr_GL_0_key.pth"] + ["state_%d.pth" % e for e in range(4)]
    s = _state(d, 1)
    assert s["epoch"] == 1 and s["steps_done"] == 6
    assert s["queue"]["state"].tolist() == [8, 16] and tuple(s["queue"]["buf"].shape)[0] == 16
    assert int((s["queue"]["buf"] != 0).any(dim=1).sum()) == 16
    assert float(s["optimizer"]["state"][0]["step"]) == 6
    assert int(s["key_encoder"]["net3DV_1.1.num_batches_tracked"]) == 6 == int(s["model"]["net3DV_1.1.num_batches_tracked"])
    assert any(not torch.equal(s["key_encoder"][k], s["model"][k]) for k in s["model"] if k.endswith(".weight"))
    assert s["swav"] is None and s["rng"]["view_source"] is None and s["rng"]["device"] is not None
    assert all(not t.is_cuda for t in s["model"].values())


def test_control_two_plain_runs_are_bit_identical(run_a, tmp_path):
    """The parent's own path: without this equality nothing below could hold."""
    got = _run(tmp_path, "--nepoch", 4, "--graph", 1)
    _assert_run_equals(got, run_a[0], tmp_path, run_a[1], epochs=(0, 1, 2, 3))
    for e in range(3):
        assert_same_state(_state(tmp_path, e), _state(run_a[1], e), "state_%d" % e)


@pytest.mark.parametrize("graph_b,graph_c", [(1, 1), (0, 0), (1, 0), (0, 1)])
def test_resumed_equals_uninterrupted(run_a, runs_b, tmp_path, graph_b, graph_c):
    (_, out_b), dir_b = runs_b(graph_b)
    assert sorted(_losses(out_b)) == [0, 1]
    src = os.path.join(str(dir_b), "state_1.pth")
    got = _run(tmp_path, "--nepoch", 4, "--graph", graph_c, "--resume", src)
    assert "resumed from %s: epoch 2" % src in got[1]
    assert sorted(_losses(got[1])) == [2, 3]                                   # epochs 0 and 1 are not run again
    assert sorted(n for n in os.listdir(str(tmp_path)) if n.startswith("state_")) == ["state_2.pth", "state_3.pth"]
    _assert_run_equals(got, run_a[0], tmp_path, run_a[1])
    assert_same_state(_state(tmp_path, 2), _state(run_a[1], 2), "state_2")


def test_resume_auto(run_a, runs_b, tmp_path):
    (_, _), dir_b = runs_b(1)
    d = tmp_path / "continued"
    shutil.copytree(str(dir_b), str(d))
    got = _run(d, "--nepoch", 4, "--resume", "auto", base=BASE[:-1] + ["2"])   # --keep_states 2
    assert "resumed from %s: epoch 2" % os.path.join(str(d), "state_1.pth") in got[1]
    assert sorted(n for n in os.listdir(str(d)) if n.startswith("state_")) == ["state_2.pth", "state_3.pth"]
    _assert_run_equals(got, run_a[0], d, run_a[1])
    # nothing to resume from: one line says so, and the run is the plain run
    e = tmp_path / "empty"
    got = _run(e, "--nepoch", 4, "--resume", "auto")
    assert "no state under %s, starting from scratch" % e in got[1] and "resumed from" not in got[1]
    _assert_run_equals(got, run_a[0], e, run_a[1], epochs=(0, 1, 2, 3))
    # a damaged newest state: a warning, and the next older one is taken
    with open(os.path.join(str(e), "state_3.pth"), "wb") as f:
        f.write(b"killed while writing")
    got = _run(e, "--nepoch", 4, "--resume", "auto")
    assert "warning:" in got[1] and "resumed from %s: epoch 3" % os.path.join(str(e), "state_2.pth") in got[1]
    _assert_run_equals(got, run_a[0], e, run_a[1], epochs=(3,))


# ---- the SwAV queue through ContrastiveStep.state_dict() -----------------------------------------------------------------
def test_swav_state_round_trips_through_the_step():
    """Four eager steps with the SwAV term against two steps, state_dict() -> load_state_dict() into a fresh model, optimizer
    and step, and two more.  The queue holds 2 batches, so it is full -- and read by the loss -- from the third step on."""
    from facl_amd import swav_cld, train_state
    from facl_amd.cn3d_model_conbag import PointNet_Plus
    from facl_amd.optim import FusedAdam
    from facl_amd.train_common import ContrastiveStep
    from oracle.weights import formula_state_dict
    D, B, G, N = 4, 4, 4, 512
    opt = step_opt(D, B, N)
    gen = torch.Generator(device=DEV)
    gen.manual_seed(3)
    points = [torch.rand((B, G, N, D), device=DEV, generator=gen) - 0.5 for _ in range(4)]
    orders = [np.random.RandomState(k).permutation(G) for k in range(4)]

    def make(with_swav_state):
        net = PointNet_Plus(opt, gost=G)
        net.load_state_dict({k: torch.as_tensor(v) for k, v in formula_state_dict(D).items()})
        net = net.to(DEV).train()
        optim = FusedAdam(net.parameters(), lr=3e-4, betas=(0.5, 0.999), eps=1e-6)
        step = ContrastiveStep(net, optim, opt, G, swa_if=1)
        if with_swav_state:
            step.swav_state = swav_cld.SwavState(B, G, 512, queue_length=2 * B, epoch_queue_starts=0)
        return net, optim, step

    def steps(step, ks):
        out = []
        for k in ks:
            out.append([t.detach().clone() for t in step(points[k], epoch=0, order=orders[k])])
            torch.cuda.synchronize()
        return out

    net_a, optim_a, step_a = make(True)
    assert step_a.state_dict()["swav"] is None
    want = steps(step_a, range(4))
    assert step_a.swav_state.use_the_queue

    net_b, optim_b, step_b = make(True)
    got = steps(step_b, range(2))
    saved = train_state.to_cpu({"model": net_b.state_dict(), "optimizer": optim_b.state_dict(), **step_b.state_dict()})
    assert saved["swav"]["filled"] == 2 * B and tuple(saved["swav"]["queue"].shape) == (G - 1, 2 * B, 512)
    net_c, optim_c, step_c = make(False)                    # no SwavState: load_state_dict creates it, before the first batch
    net_c.load_state_dict(saved["model"])
    optim_c.load_state_dict(saved["optimizer"])
    step_c.load_state_dict(saved)
    assert step_c.swav_state.use_the_queue and step_c.swav_state.queue.is_cuda
    got += steps(step_c, range(2, 4))
    for k, (g, w) in enumerate(zip(got, want)):
        for a, b in zip(g, w):
            assert torch.isfinite(a).all() and torch.equal(a, b), (k, float(a), float(b))
    assert torch.equal(step_c.swav_state.queue, step_a.swav_state.queue) and step_c.swav_state.filled == step_a.swav_state.filled
    assert_same_state(train_state.to_cpu(dict(net_c.state_dict())), train_state.to_cpu(dict(net_a.state_dict())), "model")


# ---- clips on disk (the tree of tests/test_gpu_resident.py: every clip has its own row count in all four clouds) ----------
@pytest.fixture(scope="module")
def disk_tree(tmp_path_factory):
    root = tmp_path_factory.mktemp("tree")
    write_tree(str(root), scale=1, listed=("res10",))
    return root


def _disk_base(root, *view):
    """16 training clips, 2 of their 4 batches per epoch; the queue, the key encoder and the loss mode of BASE."""
    return ["--synthetic", "0", "--data_root", str(root), "--dataset", "ntu120", "--batchSize", "4", "--INPUT_FEATURE_NUM", "4",
            "--SAMPLE_NUM", "512", "--max_steps_per_epoch", "2"] + list(view) + BASE[10:]


def test_disk_philox_resident_resume_of_a_disk_run(disk_tree, tmp_path):
    """(a) The state a --resident 0 run wrote after epoch 1, resumed with --resident 1, ends equal to the --resident 0 run that
    went on by itself: the philox views depend on (seed, epoch, dataset index) only and the batches on (seed, epoch)."""
    base = _disk_base(disk_tree, "--view_rng", "philox", "--num_crop", "4")
    a, c = tmp_path / "a", tmp_path / "c"
    want = _run(a, "--nepoch", 4, "--resident", 0, base=base)
    assert _state(a, 1)["queue"]["state"].tolist() == [0, 16] and _state(a, 1)["steps_done"] == 4
    got = _run(c, "--nepoch", 4, "--resident", 1, "--resume", os.path.join(str(a), "state_1.pth"), base=base)
    assert "resident: 16 clips" in got[1] and "resident:" not in want[1]
    assert sorted(_losses(got[1])) == [2, 3]
    _assert_run_equals(got, want, c, a)


def test_disk_numpy_views_resume_through_the_producer_thread(disk_tree, tmp_path):
    """(b) --view_rng numpy draws every clip's random numbers from TrainBatches.view_rng on the producer thread: the state is
    taken when that thread has stopped, and the resumed run draws on from there."""
    base = _disk_base(disk_tree, "--view_rng", "numpy", "--num_crop", "10", "--prefetch", "1")
    a, c = tmp_path / "a", tmp_path / "c"
    want = _run(a, "--nepoch", 4, base=base)
    s1 = _state(a, 1)
    fresh = np.random.RandomState(2000).get_state()
    assert not np.array_equal(s1["rng"]["view_source"]["keys"].numpy(), fresh[1].astype(np.int64))     # it has drawn
    got = _run(c, "--nepoch", 4, "--resume", os.path.join(str(a), "state_1.pth"), base=base)
    assert sorted(_losses(got[1])) == [2, 3]
    _assert_run_equals(got, want, c, a)


# ---- refusals: each before any training step -----------------------------------------------------------------------------
def test_refusals(runs_b, tmp_path, monkeypatch):
    from facl_amd import cn3d_train_motion_GL as train
    (_, _), dir_b = runs_b(1)
    src = os.path.join(str(dir_b), "state_1.pth")

    def refused(args, match):
        out = io.StringIO()
        with contextlib.redirect_stdout(out), pytest.raises(RuntimeError, match=match) as e:
            train.main(args + ["--save_root_dir", str(tmp_path / "ck")])
        assert "--loss:" not in out.getvalue() and "resumed from" not in out.getvalue()
        assert not (tmp_path / "ck").exists()               # refused before the run was set up: no folder, no device
        return str(e.value)

    other = list(BASE)
    other[other.index("--batchSize") + 1] = "8"
    msg = refused(other + ["--nepoch", "4", "--resume", src], "batchSize")
    assert "--batchSize 8 (the state: 4)" in msg and "neg_queue" not in msg
    state = torch.load(src, map_location="cpu", weights_only=True)
    state["format"] += 1
    newer = str(tmp_path / "state_1.pth")
    torch.save(state, newer)
    msg = refused(BASE + ["--nepoch", "4", "--resume", newer], "format %d" % state["format"])
    assert newer in msg
    del state["optimizer"]
    state["format"] -= 1
    torch.save(state, newer)
    msg = refused(BASE + ["--nepoch", "4", "--resume", newer], "lacks optimizer")
    assert newer in msg
    monkeypatch.setenv("WORLD_SIZE", "2")
    plain = ["--synthetic", "1", "--batchSize", "4", "--num_crop", "4", "--SAMPLE_NUM", "512", "--steps_per_epoch", "3"]
    refused(plain + ["--resume", src], "--resume .* runs on one rank only")
    refused(plain + ["--save_state_every", "1"], "--save_state_every 1 runs on one rank only")
