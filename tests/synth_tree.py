"""A small synthetic 3DV dataset on disk, and the training entry run on it.

`tree_clip` draws the four clouds of one clip; `write_tree` lays clips out the way facl_amd/dataset.py reads them, under
the NTU names of `clip_names`.  (helpers.synth_clip is another formula, tied to tests/golden/views.npz; the two are not
interchangeable.)  `run_train_entry` runs cn3d_train_motion_GL.main on an argv -- `train_argv` builds the common one -- and
`assert_same_state` / `epoch_loss_text` compare what two runs left."""
import contextlib
import io
import os
import re

import numpy as np


def tree_clip(seed, P, Kp=300, R1=400, R2=150, dt=np.float64):
    """The four (rows, 8) clouds of one clip; channels 4 and 7 of the first cloud (the temporal channels) are zero in ~30 % /
    ~50 % of its rows."""
    r = np.random.RandomState(seed)
    pts = r.rand(P, 8) - 0.5
    pts[r.rand(P) < 0.3, 4] = 0
    pts[r.rand(P) < 0.5, 7] = 0
    pts[0, 4] = pts[0, 7] = 0.25                          # at least one non-zero row in each temporal channel
    return tuple(a.astype(dt) for a in (pts, r.rand(Kp, 8) - 0.5, r.rand(R1, 8) - 0.5, r.rand(R2, 8) - 0.5))


def write_clip(root, name, clip, branch="0"):
    from facl_amd.dataset import clip_paths
    for p, a in zip(clip_paths(str(root), name, branch), clip):
        os.makedirs(os.path.dirname(p), exist_ok=True)
        np.save(p, a)


def clip_names(n):
    """n clips over 4 actions: cameras 2 / 3 (cross-view train) and 1 (test), every action in both splits."""
    return ["S%03dC%03dP%03dR001A%03d" % (1 + i % 4, (2, 3, 1)[i % 3], 1 + i, 1 + (i // 3) % 4) for i in range(n)]


def write_tree(root, n=24, dt=np.float64, scale=None, clips=None, listed=("raw",)):
    """n clips under `root`; returns their names.

    scale=None: the first cloud of clip i has 600 + 7 i rows, the others 300 / 400 / 150.  scale=s: every clip has its own
    row count in all four clouds, s * (600 + 7 i, 300 + 3 i, 400 + 5 i, 150 + i).  `clips`: {i: clip} replaces clip i.
    `listed`: the folders beside the clouds that an entry lists the clips from -- "raw": raw/<name>.npy holding
    zeros((1, 8)), the extraction and fine-tuning entries' listing; "res10": the directory reslution/Resolution10/raw, made
    even where no clip was written."""
    names = clip_names(n)
    for i, nm in enumerate(names):
        if scale is None:
            sizes = (600 + 7 * i, 300, 400, 150)
        else:
            sizes = (scale * (600 + 7 * i), scale * (300 + 3 * i), scale * (400 + 5 * i), scale * (150 + i))
        write_clip(root, nm, (clips or {}).get(i) or tree_clip(200 + i, *sizes, dt=dt))
        if "raw" in listed:
            os.makedirs(os.path.join(root, "raw"), exist_ok=True)
            np.save(os.path.join(root, "raw", nm + ".npy"), np.zeros((1, 8)))
    if "res10" in listed:
        os.makedirs(os.path.join(root, "reslution", "Resolution10", "raw"), exist_ok=True)
    return names


def train_argv(root, folder, *extra, after_batch=(), before_save=(), features_first=False):
    """The argv of a training run on a tree: --synthetic 0 --data_root .. --dataset ntu120 --batchSize 4 <after_batch>
    --num_crop 10 --SAMPLE_NUM 512 --INPUT_FEATURE_NUM 4 <before_save> --save_root_dir .. <extra>.  features_first puts
    --INPUT_FEATURE_NUM 4 in front of --batchSize (the order of the loss-mask entries' tests)."""
    feat = ["--INPUT_FEATURE_NUM", "4"]
    return (["--synthetic", "0", "--data_root", str(root), "--dataset", "ntu120"] + (feat if features_first else [])
            + ["--batchSize", "4"] + [str(a) for a in after_batch] + ["--num_crop", "10", "--SAMPLE_NUM", "512"]
            + ([] if features_first else feat) + [str(a) for a in before_save] + ["--save_root_dir", str(folder)]
            + [str(a) for a in extra])


def run_train_entry(argv):
    """One run of the motion training entry: (the returned model's state_dict cloned to the CPU, what it printed)."""
    import torch
    from facl_amd import cn3d_train_motion_GL as train
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        net = train.main(list(argv))
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    return {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}, out.getvalue()


def assert_same_state(a, b, where):
    """Bit equality of two nested states (tensors, dicts in key order, lists and tuples, plain values)."""
    import torch
    assert type(a) is type(b), where
    if torch.is_tensor(a):
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), where
    elif isinstance(a, dict):
        assert list(a) == list(b), where
        for k in a:
            assert_same_state(a[k], b[k], "%s.%s" % (where, k))
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), where
        for i, (x, y) in enumerate(zip(a, b)):
            assert_same_state(x, y, "%s[%d]" % (where, i))
    else:
        assert a == b, (where, a, b)


def epoch_loss_text(out, epoch):
    """The mean loss of `epoch` as the entry printed it: exactly one such line."""
    m = re.findall(r"epoch: %d loss mode is : 1 --loss: (\S+)" % epoch, out)
    assert len(m) == 1, out
    return m[0]
