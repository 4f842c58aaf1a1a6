"""CPU-side checks of supervised fine-tuning (facl_amd/finetune.py, facl_amd/cls_head.py, csrc/cls.hip): the stratified label
subset, the flag refusals, the three C ABI entries' declarations and their FACL_E_SHAPE refusals (which come before any launch)."""
import math
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("facl_cls_gather_norm_fwd", "facl_cls_gather_norm_bwd", "facl_softmax_ce")
E_SHAPE = -1


def _labels():
    r = np.random.RandomState(3)
    y = np.concatenate([np.full(n, c) for c, n in enumerate((1, 2, 7, 30, 101))])
    return y[r.permutation(len(y))]


def test_label_subset_is_deterministic():
    from facl_amd.finetune import label_subset
    y = _labels()
    a, b = label_subset(y, 0.3, 5), label_subset(y, 0.3, 5)
    assert a.dtype.kind == "i" and (a == b).all() and (np.diff(a) > 0).all()
    assert not np.array_equal(a, label_subset(y, 0.3, 6))
    assert np.array_equal(a, label_subset(list(y), 0.3, 5))


@pytest.mark.parametrize("f", [0.001, 0.1, 0.25, 0.5, 0.99])
def test_label_subset_is_stratified(f):
    from facl_amd.finetune import label_subset
    y = _labels()
    s = label_subset(y, f, 0)
    assert len(set(s.tolist())) == len(s) and s.min() >= 0 and s.max() < len(y)
    for c in np.unique(y):
        assert int((y[s] == c).sum()) == max(1, math.ceil(f * int((y == c).sum()))), (c, f)


def test_label_subset_is_nested_across_fractions():
    from facl_amd.finetune import label_subset
    y = _labels()
    prev = set()
    for f in (0.01, 0.05, 0.1, 0.3, 0.7, 1.0):
        cur = set(label_subset(y, f, 11).tolist())
        assert prev <= cur, f
        prev = cur


def test_label_subset_whole_split_and_refusals():
    from facl_amd.finetune import label_subset
    y = _labels()
    assert np.array_equal(label_subset(y, 1.0, 9), np.arange(len(y)))
    for f in (0.0, -0.1, 1.0001, 2):
        with pytest.raises(ValueError, match="label_fraction"):
            label_subset(y, f, 0)


def test_flag_checks(monkeypatch):
    from facl_amd import finetune
    p = finetune.finetune_parser()
    opt = p.parse_args([])
    assert (opt.checkpoint, opt.label_fraction, opt.label_seed, opt.eval_every) == ('', 1.0, 0, 1)
    finetune.check_finetune_flags(opt, world=1)
    assert opt.num_class == 60
    opt = p.parse_args(["--dataset", "ntu120"])
    finetune.check_finetune_flags(opt, world=1)
    assert opt.num_class == 120
    with pytest.raises(RuntimeError, match="one rank"):
        finetune.check_finetune_flags(p.parse_args([]), world=2)
    for bad, what in ((["--label_fraction", "0"], "label_fraction"), (["--label_fraction", "1.5"], "label_fraction"),
                      (["--synthetic", "2"], "synthetic"), (["--num_class", "1025"], "num_class"), (["--eval_every", "-1"], "eval_every")):
        with pytest.raises(RuntimeError, match=what):
            finetune.check_finetune_flags(p.parse_args(bad), world=1)
    # the entry itself refuses before the device is touched (there is no GPU here)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(RuntimeError, match="one rank"):
        finetune.main(["--synthetic", "1", "--nepoch", "1"])


def test_entries_are_declared_and_exported():
    from facl_amd import _lib, build
    build.build()
    lib = _lib.load_library()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "facl_hip.h")).read(), flags=re.S)
    for s in ENTRIES:
        assert re.search(r"int\s+%s\s*\(" % s, hdr), s
        assert s in _lib.SIGNATURES and hasattr(lib, s), s


def test_entries_refuse_shapes_outside_their_domain():
    """FACL_E_SHAPE comes before the pointer checks and before any launch, so the refusals run without a GPU (NULL pointers)."""
    from facl_amd import _lib
    lib = _lib.load_library()
    fwd = lambda G, B, C: lib.facl_cls_gather_norm_fwd(None, G, B, C, None, None, None)
    bwd = lambda G, B, C: lib.facl_cls_gather_norm_bwd(None, None, None, G, B, C, None, None)
    for fn in (fwd, bwd):
        assert fn(2, 3, 96) == E_SHAPE and fn(0, 3, 512) == E_SHAPE and fn(65, 3, 512) == E_SHAPE
        assert fn(2, 0, 512) == E_SHAPE and fn(2, 3, 0) == E_SHAPE and fn(2, 3, 1088) == E_SHAPE
        assert fn(2, 3, 512) == -2 and fn(64, 1, 1024) == -2 and fn(1, 1, 64) == -2      # inside the domain: FACL_E_NULL
    ce = lambda R, ncls, ld: lib.facl_softmax_ce(None, ld, None, R, ncls, None, None, None, None, None)
    assert ce(4, 1, 1) == E_SHAPE and ce(4, 1025, 1025) == E_SHAPE and ce(4, 60, 59) == E_SHAPE and ce(0, 60, 60) == E_SHAPE
    assert ce(4, 2, 2) == -2 and ce(4, 1024, 1027) == -2
