"""The weighted-kNN training monitor (--knn_every) and the standalone entry (python -m facl_amd.knn_eval) on a small
dataset tree written the way tests/test_gpu_dataset.py writes its own."""
import os
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
KNN_K = "3"


def _clip(seed, P):
    r = np.random.RandomState(seed)
    pts = r.rand(P, 8) - 0.5
    pts[r.rand(P) < 0.3, 4] = 0
    pts[r.rand(P) < 0.5, 7] = 0
    pts[0, 4] = pts[0, 7] = 0.25                          # at least one non-zero row in each temporal channel
    return pts, r.rand(300, 8) - 0.5, r.rand(400, 8) - 0.5, r.rand(150, 8) - 0.5


def _tree(root, n=24):
    """n clips: cameras 2 / 3 (cross-view train: 16) and 1 (test: 8), four actions, every action in both splits."""
    from facl_amd.dataset import clip_paths
    names = ["S%03dC%03dP%03dR001A%03d" % (1 + i % 4, (2, 3, 1)[i % 3], 1 + i, 1 + (i // 3) % 4) for i in range(n)]
    os.makedirs(os.path.join(root, "raw"), exist_ok=True)
    for i, nm in enumerate(names):
        for p, a in zip(clip_paths(str(root), nm, "0"), _clip(200 + i, 600 + 7 * i)):
            os.makedirs(os.path.dirname(p), exist_ok=True)
            np.save(p, a)
        np.save(os.path.join(root, "raw", nm + ".npy"), np.zeros((1, 8)))
    return names


def _train_args(root, ck, *extra):
    return ["--synthetic", "0", "--data_root", str(root), "--dataset", "ntu120", "--batchSize", "4", "--nepoch", "2",
            "--max_steps_per_epoch", "2", "--num_crop", "10", "--SAMPLE_NUM", "512", "--INPUT_FEATURE_NUM", "4",
            "--knn_k", KNN_K, "--save_root_dir", str(ck)] + list(extra)


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = tmp_path_factory.mktemp("knn_tree")
    return root, _tree(root)


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
