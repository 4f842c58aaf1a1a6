"""CPU-side checks of prediction (facl_amd/predict.py, csrc/predict.hip): the two C ABI entries' declarations and their
FACL_E_SHAPE refusals (which come before any launch), the host functions `confusion` and `metrics` on hand-written cases, the
entry's refusals (all raised before the device is touched: there is no GPU here) and linear_classify's --save_fc flag."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("facl_cls_probs_acc", "facl_cls_topk")
E_SHAPE, E_NULL = -1, -2


def test_entries_are_declared_and_exported():
    from facl_amd import _lib, build
    build.build()
    lib = _lib.load_library()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "facl_hip.h")).read(), flags=re.S)
    for s in ENTRIES:
        assert re.search(r"int\s+%s\s*\(" % s, hdr), s
        assert s in _lib.SIGNATURES and hasattr(lib, s), s
    assert lib.facl_version() >> 16 == 1


def test_entries_refuse_shapes_outside_their_domain():
    """FACL_E_SHAPE comes before the pointer checks and before any launch, so the refusals run without a GPU (NULL pointers)."""
    from facl_amd import _lib
    lib = _lib.load_library()
    probs = lambda R, ncls, ld: lib.facl_cls_probs_acc(None, ld, R, ncls, None, 1, None)
    assert probs(4, 1, 1) == E_SHAPE and probs(4, 1025, 1025) == E_SHAPE
    assert probs(0, 60, 60) == E_SHAPE and probs(4, 60, 59) == E_SHAPE
    assert probs(4, 2, 2) == E_NULL and probs(1, 1024, 1024) == E_NULL and probs(4, 60, 64) == E_NULL      # inside the domain
    topk = lambda R, ncls, ndraws, k: lib.facl_cls_topk(None, R, ncls, ndraws, k, None, None, None, None, None)
    assert topk(4, 1, 1, 1) == E_SHAPE and topk(4, 1025, 1, 1) == E_SHAPE and topk(0, 60, 1, 1) == E_SHAPE
    assert topk(4, 60, 1, 0) == E_SHAPE and topk(4, 60, 1, 61) == E_SHAPE and topk(4, 2, 1, 3) == E_SHAPE
    assert topk(4, 1024, 1, 65) == E_SHAPE and topk(4, 60, 0, 5) == E_SHAPE
    assert topk(4, 60, 1, 60) == E_NULL and topk(4, 1024, 3, 64) == E_NULL and topk(1, 2, 1, 2) == E_NULL


def test_confusion_by_hand():
    from facl_amd.predict import confusion
    #         true  pred
    labels = [0, 0, 2, 2, 2, 3, 5, -1, 1]
    pred = [0, 2, 2, 2, 0, 3, 0, 0, -1]                  # label 5 / -1 outside [0, 4); prediction -1 = a NaN row
    m, skipped = confusion(labels, pred, 4)
    want = np.zeros((4, 4), dtype=np.int64)
    want[0, 0], want[0, 2], want[2, 2], want[2, 0], want[3, 3] = 1, 1, 2, 1, 1
    assert m.dtype == np.int64 and np.array_equal(m, want) and skipped == 3
    assert m.sum() == len(labels) - skipped and np.trace(m) == 4
    assert m[1].sum() == 0                               # class 1 has no clip that counts
    m, skipped = confusion([], [], 3)
    assert m.shape == (3, 3) and m.sum() == 0 and skipped == 0
    with pytest.raises(ValueError, match="length"):
        confusion([0, 1], [0], 3)


def test_metrics_by_hand():
    from facl_amd.predict import metrics
    # class 0: ranks 0, 1, 4 -> 1 of 3;  class 1 never occurs;  class 2: rank 0 and a NaN row (-1) -> 1 of 2;
    # class 3: rank 2 -> 0 of 1;  one clip with a label outside the range (rank -2): left out and counted
    rank = [0, 1, 4, 0, -1, 2, -2]
    labels = [0, 0, 0, 2, 2, 3, 9]
    m = metrics(rank, labels, 5, 3)
    assert m["clips"] == 6 and m["skipped"] == 1
    assert m["top1"] == 100.0 * 2 / 6
    assert m["topk"] == 100.0 * 4 / 6                    # ranks 0, 1, 0, 2 are below 3; -1 is no hit
    pc = m["per_class"]
    assert pc.shape == (5,) and np.isnan(pc[1]) and np.isnan(pc[4])
    assert pc[0] == 100.0 / 3 and pc[2] == 50.0 and pc[3] == 0.0
    assert m["mean_class"] == pytest.approx((100.0 / 3 + 50.0 + 0.0) / 3, rel=1e-15)
    # k = 1: top-k is top-1
    m1 = metrics(rank, labels, 5, 1)
    assert m1["topk"] == m1["top1"] == m["top1"]
    # every clip right: 100 everywhere, whatever k
    m = metrics([0, 0, 0], [1, 1, 3], 4, 2)
    assert m["top1"] == m["topk"] == m["mean_class"] == 100.0 and m["skipped"] == 0
    with pytest.raises(ValueError, match="length"):
        metrics([0, 1], [0], 3, 1)


def test_save_npz_is_reproducible_and_readable(tmp_path):
    from facl_amd.predict import save_npz
    arrays = dict(names=np.asarray(["S001C001P001R001A001", "S001C002P001R001A002"]), top_c=np.arange(6, dtype=np.int32).reshape(2, 3),
                  top_p=np.linspace(0, 1, 6, dtype=np.float32).reshape(2, 3))
    save_npz(str(tmp_path / "a.npz"), **arrays)
    save_npz(str(tmp_path / "b.npz"), **arrays)
    assert open(str(tmp_path / "a.npz"), "rb").read() == open(str(tmp_path / "b.npz"), "rb").read()
    z = np.load(str(tmp_path / "a.npz"))
    assert sorted(z.files) == sorted(arrays)
    for k, v in arrays.items():
        assert z[k].dtype == v.dtype and np.array_equal(z[k], v), k


def _head(path, num_crop, num_class):
    import torch
    from facl_amd.cls_head import ClipClassifier
    torch.save(ClipClassifier(num_crop, num_class).state_dict(), path)
    return path


def test_entry_refusals_come_before_the_device(tmp_path, monkeypatch):
    import torch
    from facl_amd import predict
    monkeypatch.setattr(torch.cuda, "set_device", lambda *a, **k: pytest.fail("the device was touched"))
    head = _head(str(tmp_path / "fc.pth"), 10, 8)
    enc = str(tmp_path / "enc.pth")
    torch.save({}, enc)
    clips = ["--encoder", enc, "--head", head, "--data_root", str(tmp_path / "none")]
    folders = ["--motion_feature_dir", str(tmp_path / "m"), "--head", head, "--data_root", str(tmp_path / "none")]
    for args, what in ((clips + ["--draws", "0"], "--draws must be >= 1"),
                       (clips + ["--draws", "-2"], "--draws must be >= 1"),
                       (clips + ["--topk", "0"], "--topk must be in 1"),
                       (clips + ["--topk", "65"], "--topk must be in 1"),
                       (clips + ["--topk", "9"], r"--topk must be in 1\.\.min\(num_class, 64\) = 1\.\.8"),       # num_class 8
                       (clips + ["--motion_feature_dir", str(tmp_path / "m")], "got both"),
                       (clips + ["--appearance_feature_dir", str(tmp_path / "a")], "got both"),
                       (["--head", head], "got neither"),
                       (["--encoder", enc], "--head is required"),
                       (folders + ["--draws", "2"], "--draws 2 needs --encoder"),
                       (clips + ["--num_crop", "24"], "--view_rng philox"),                                     # check_view_flags
                       (clips + ["--num_crop", "24", "--view_rng", "philox"], "--num_crop 10 .* --num_crop 24")):
        with pytest.raises(RuntimeError, match=what):
            predict.main(args)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(RuntimeError, match="one rank"):
        predict.main(clips)


def test_head_built_for_other_views_is_refused_with_both_numbers(tmp_path):
    import torch
    from facl_amd import predict
    head_sd = torch.load(_head(str(tmp_path / "fc.pth"), 24, 60), map_location="cpu", weights_only=True)
    opt = predict.predict_parser().parse_args(["--num_crop", "10"])
    with pytest.raises(RuntimeError) as e:
        predict.Classifier(head_sd, opt, encoder_sd={})
    assert "--num_crop 24" in str(e.value) and "--num_crop 10" in str(e.value) and "60 x 12800" in str(e.value)
    # without an encoder the same head is a probe head: num_class and the width come from fc.weight
    clf = predict.Classifier(head_sd)
    assert (clf.num_class, clf.width, clf.views, clf.encoder) == (60, 25 * 512, 24, None)
    with pytest.raises(RuntimeError, match="no 2-D fc.weight"):
        predict.Classifier({"fc.bias": torch.zeros(4)})
    with pytest.raises(RuntimeError, match="not \\(views \\+ 1\\) \\* 512"):
        predict.Classifier({"fc.weight": torch.zeros(4, 700), "fc.bias": torch.zeros(4)})


def test_ordered_views_epoch_defaults_to_zero():
    import inspect
    from facl_amd.extract_common import ordered_views
    p = inspect.signature(ordered_views).parameters
    assert list(p)[:5] == ["opt", "device", "index", "split", "rng"] and p["epoch"].default == 0


def test_linear_classify_accepts_save_fc(tmp_path, capsys, monkeypatch):
    """The flag parses (an unknown flag would end in argparse's SystemExit) and defaults to ''; the run itself then stops at the
    first thing it needs, the device or the data root, neither of which exists here."""
    import torch
    from facl_amd import linear_classify

    class Stop(Exception):
        pass

    def stop(*a, **k):
        raise Stop()
    monkeypatch.setattr(torch.cuda, "set_device", stop)
    base = ["--motion_feature_dir", "m", "--appearance_feature_dir", "a", "--data_root", str(tmp_path / "none")]
    with pytest.raises(Stop):
        linear_classify.main(base + ["--save_fc", str(tmp_path / "probe_fc.pth")])
    assert "save_fc='%s'" % str(tmp_path / "probe_fc.pth") in capsys.readouterr().out
    with pytest.raises(Stop):
        linear_classify.main(base)
    assert "save_fc=''" in capsys.readouterr().out
