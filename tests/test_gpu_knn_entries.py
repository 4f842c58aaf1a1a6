"""The weighted-kNN training monitor (--knn_every) and the standalone entry (python -m facl_amd.knn_eval) on a small
dataset tree (synth_tree.write_tree: 16 train clips, 8 test clips, four actions, every action in both splits)."""
import os
import re

import pytest
import torch

from synth_tree import train_argv, write_tree

pytestmark = pytest.mark.gpu
KNN_K = "3"


def _train_args(root, ck, *extra):
    return train_argv(root, ck, *extra, after_batch=("--nepoch", "2", "--max_steps_per_epoch", "2"), before_save=("--knn_k", KNN_K))


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = tmp_path_factory.mktemp("knn_tree")
    return root, write_tree(root)


def _logged(out):
    return [float(v) for v in re.findall(r"knn top1: ([0-9.eE+-]+)", out)]


@pytest.mark.parametrize("graph", ["0", "1"])
def test_monitor_does_not_perturb_training(tree, tmp_path, capsys, graph):
    from facl_amd import cn3d_train_motion_GL as train
    root, _ = tree
    states, files = [], []
    for every in ("1", "0"):
        ck = tmp_path / ("ck" + every)
        capsys.readouterr()
        net = train.main(_train_args(root, ck, "--graph", graph, "--knn_every", every))
        vals = _logged(capsys.readouterr().out)
        if every == "1":
            assert len(vals) == 2 and all(0.0 <= v <= 100.0 for v in vals), vals
        else:
            assert vals == []
        assert net.training
        states.append({k: v.detach().cpu().clone() for k, v in net.state_dict().items()})
        files.append(torch.load(str(ck / "corr_GL_0.pth"), map_location="cpu", weights_only=True))
    for a, b in (states, files):
        assert a.keys() == b.keys()
        for k in a:
            assert torch.equal(a[k], b[k]), k                            # bit-identical, running statistics included


def test_monitor_matches_the_standalone_entry(tree, tmp_path, capsys):
    from facl_amd import cn3d_train_motion_GL as train, extract_motion_feature as ext, knn_eval
    root, names = tree
    ck = tmp_path / "ck"
    capsys.readouterr()
    train.main(_train_args(root, ck, "--graph", "0", "--nepoch", "1", "--knn_every", "1"))
    vals = _logged(capsys.readouterr().out)
    assert len(vals) == 1
    out = tmp_path / "f"
    ext.main(["--synthetic", "0", "--data_root", str(root), "--dataset", "ntu120", "--batchSize", "4",
              "--checkpoint", str(ck / "corr_GL_0.pth"), "--save_path", str(out) + "/"])
    assert sorted(os.listdir(out)) == sorted(n + ".npy" for n in names)
    top1 = knn_eval.main(["--data_root", str(root), "--dataset", "ntu120", "--motion_feature_dir", str(out), "--k", KNN_K])
    assert "knn top1: " in capsys.readouterr().out
    assert 0.0 <= top1 <= 100.0 and top1 == vals[0]


def test_monitor_refuses_synthetic_clouds(tmp_path):
    from facl_amd import cn3d_train_motion_GL as train
    with pytest.raises(RuntimeError, match="needs --synthetic 0"):
        train.main(["--knn_every", "1", "--synthetic", "1", "--save_root_dir", str(tmp_path / "ck")])
    assert not os.path.exists(str(tmp_path / "ck"))                      # refused before anything was set up
