"""--optim sgd / lars through the entries, on the clip tree and at the sizes of test_gpu_resume.py's disk runs (16 training clips,
batches of 4, two steps per epoch, four philox views): the motion entry under LARS with decay, clipping and warm-up, its resume
from a state file, the refusal of another optimizer on resume, fine-tuning under Nesterov SGD, and the silence of a default
run."""
import os
import re

import numpy as np
import pytest
import torch

from synth_tree import assert_same_state, run_train_entry, write_tree

pytestmark = pytest.mark.gpu

LARS = ["--optim", "lars", "--sgd_weight_decay", "1e-4", "--clip_grad_norm", "1", "--warmup_steps", "2"]
OPT_LINE = "optimizer: lars momentum 0.9 nesterov 0 weight decay 0.0001 eta 0.001"
EPOCH_LINE = (r"epoch: %d loss mode is : 1 --loss: (\S+) \| clips/s: \S+ \| grad norm mean/max: \S+/\S+, clipped \d+/2 steps"
              r" \| trust ratio min/median/max: (\S+)/(\S+)/(\S+)\n")


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = tmp_path_factory.mktemp("tree")
    write_tree(str(root), scale=1, listed=("raw", "res10"))
    return root


def _base(root):
    return ["--synthetic", "0", "--data_root", str(root), "--dataset", "ntu120", "--batchSize", "4", "--INPUT_FEATURE_NUM", "4",
            "--SAMPLE_NUM", "512", "--max_steps_per_epoch", "2", "--view_rng", "philox", "--num_crop", "4"]


def _run(root, folder, *extra):
    return run_train_entry(_base(root) + ["--save_root_dir", str(folder)] + [str(a) for a in extra])


@pytest.fixture(scope="module")
def lars_run(tree, tmp_path_factory):
    """The uninterrupted run: two epochs, a state after each."""
    d = tmp_path_factory.mktemp("a")
    return _run(tree, d, *LARS, "--nepoch", 2, "--save_state_every", 1), d


def test_motion_entry_under_lars(lars_run, tree):
    from facl_amd import train_state
    (sd, out), d = lars_run
    assert out.count(OPT_LINE + "\n") == 1
    for epoch in (0, 1):
        m = re.search(EPOCH_LINE % epoch, out)
        assert m, out
        loss, lo, med, hi = (float(v) for v in m.groups())
        assert np.isfinite(loss) and 0.0 < lo <= med <= hi and np.isfinite(hi)
    assert all(torch.isfinite(v).all() for v in sd.values() if v.is_floating_point())
    state = train_state.load_state(os.path.join(str(d), "state_1.pth"))
    assert state["flags"]["optim"] == "lars" and state["flags"]["sgd_weight_decay"] == 1e-4
    st0 = state["optimizer"]["state"][0]
    assert set(st0) == {"step", "momentum_buffer"} and float(st0["step"]) == 4.0
    assert bool(st0["momentum_buffer"].abs().sum() > 0)
    grp = state["optimizer"]["param_groups"][0]
    assert (grp["momentum"], grp["dampening"], grp["weight_decay"], grp["nesterov"]) == (0.9, 0, 1e-4, False)


def test_the_checkpoint_differs_from_the_initial_weights(lars_run, tree, tmp_path):
    """The checkpoint written after epoch 0 against the one of a run at rate zero: the initial weights, saved by the same entry."""
    _, d = lars_run
    _run(tree, tmp_path, "--optim", "sgd", "--learning_rate", 0, "--nepoch", 1)
    ck, ck0 = (torch.load(os.path.join(str(f), "corr_GL_0.pth"), map_location="cpu", weights_only=True) for f in (d, tmp_path))
    weights = [k for k, v in ck.items() if v.is_floating_point() and "running" not in k]
    assert weights and list(ck) == list(ck0) and all(torch.isfinite(ck[k]).all() for k in weights)
    assert sum(not torch.equal(ck[k], ck0[k]) for k in weights) >= len(weights) // 2


def test_resumed_lars_run_equals_the_uninterrupted_one(lars_run, tree, tmp_path):
    from facl_amd import cn3d_train_motion_GL as train
    from facl_amd import train_state
    (sd_a, out_a), a = lars_run
    _run(tree, tmp_path, *LARS, "--nepoch", 1, "--save_state_every", 1)                # stopped after epoch 0
    sd_b, out_b = _run(tree, tmp_path, *LARS, "--nepoch", 2, "--save_state_every", 1, "--resume", "auto")
    assert "resumed from %s: epoch 1" % os.path.join(str(tmp_path), "state_0.pth") in out_b
    assert re.search(EPOCH_LINE % 1, out_b) and not re.search(EPOCH_LINE % 0, out_b)
    assert_same_state(sd_b, sd_a, "model")
    assert_same_state(train_state.load_state(os.path.join(str(tmp_path), "state_1.pth")),
                      train_state.load_state(os.path.join(str(a), "state_1.pth")), "state_1")
    assert re.search(EPOCH_LINE % 1, out_b).groups() == re.search(EPOCH_LINE % 1, out_a).groups()
    # another optimizer would not continue the trajectory
    args = _base(tree) + ["--save_root_dir", str(tmp_path), "--nepoch", "2", "--resume", "auto"]
    sgd = [("sgd" if a == "lars" else a) for a in LARS]
    with pytest.raises(RuntimeError, match=r"--optim 'sgd' \(the state: 'lars'\)"):
        train.main(args + sgd)


def test_finetune_under_nesterov_sgd(tree, tmp_path, capsys):
    from facl_amd import finetune
    finetune.main(_base(tree) + ["--save_root_dir", str(tmp_path), "--nepoch", "1", "--num_class", "4", "--optim", "sgd",
                                 "--sgd_nesterov", "1"])
    out = capsys.readouterr().out
    assert out.count("optimizer: sgd momentum 0.9 nesterov 1 weight decay 0\n") == 1 and "trust ratio" not in out
    m = re.search(r"epoch: 0 --loss: (\S+) train top1: (\S+) \|", out)
    assert m and np.isfinite(float(m.group(1))) and 0.0 <= float(m.group(2)) <= 100.0, out
    t = re.search(r"epoch: 0 test top1: (\S+)", out)
    assert t and 0.0 <= float(t.group(1)) <= 100.0, out
    assert os.path.exists(os.path.join(str(tmp_path), "finetune_enc_0.pth"))


def test_a_default_run_prints_neither_line(tree, tmp_path):
    _, out = _run(tree, tmp_path, "--nepoch", 1)
    assert "--loss:" in out and "optimizer:" not in out and "trust ratio" not in out
