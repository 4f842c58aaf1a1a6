"""CPU-side checks of the weighted-kNN evaluation (facl_amd/knn_eval.py, csrc/knn.hip): symbols, parsers, refusals."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("facl_knn_ws_bytes", "facl_knn_topk", "facl_knn_vote")


def test_knn_symbols_are_exported_and_declared():
    from facl_amd import _lib, build
    build.build()
    lib = _lib.load_library()
    hdr = open(os.path.join(ROOT, "include", "facl_hip.h")).read()
    for s in ENTRIES:
        assert re.search(r"(?:int|int64_t)\s+%s\s*\(" % s, hdr), s
        assert s in _lib.SIGNATURES and hasattr(lib, s), s


def test_ws_bytes_is_host_only_and_never_quadratic():
    from facl_amd import _lib
    lib = _lib.load_library()
    assert lib.facl_knn_ws_bytes(0, 10, 5) == -1 and lib.facl_knn_ws_bytes(10, 10, 0) == -1
    assert lib.facl_knn_ws_bytes(10, 10, 65) == -1 and lib.facl_knn_ws_bytes(10, 0, 5) == -1
    for nq, nb, k in ((18960, 37920, 20), (3, 4100, 5), (1, 64, 64), (128, 1 << 20, 64)):
        n = lib.facl_knn_ws_bytes(nq, nb, k)
        splits = max(1, 512 // ((nq + 127) // 128))                       # an upper bound of the documented split count
        assert 0 < n <= 8 * (nq + nb) + 256 + 8 * nq * k * splits, (nq, nb, k, n)


def test_cli_parser_takes_one_or_two_feature_directories():
    from facl_amd import knn_eval
    p = knn_eval.build_parser()
    one = p.parse_args(["--motion_feature_dir", "m"])
    assert one.appearance_feature_dir is None and one.k == 20 and one.temperature == 0.1
    two = p.parse_args(["--motion_feature_dir", "m", "--appearance_feature_dir", "a", "--k", "5", "--temperature", "0.07",
                        "--data_root", "r", "--dataset", "ntu60", "--split", "subject", "--full_train", "0", "--main_gpu", "0"])
    assert (two.appearance_feature_dir, two.k, two.temperature, two.split) == ("a", 5, 0.07, "subject")
    with pytest.raises(SystemExit):
        p.parse_args([])


def test_load_split_one_or_two_streams(tmp_path):
    import numpy as np
    from facl_amd.linear_classify import load_split

    class Index:
        def v_name(self, v):
            return "clip%d" % v

        def label(self, v):
            return v % 3

    m, a = tmp_path / "m", tmp_path / "a"
    m.mkdir(), a.mkdir()
    for v in range(4):
        np.save(str(m / ("clip%d.npy" % v)), np.full(6, v, np.float32))
        np.save(str(a / ("clip%d.npy" % v)), np.full(6, 10 + v, np.float32))
    f2, y2 = load_split(Index(), range(4), str(m), str(a))
    assert f2.shape == (4, 12) and f2.dtype == np.float32 and y2.dtype == np.int64 and list(y2) == [0, 1, 2, 0]
    assert (f2[:, :6] == np.arange(4)[:, None]).all() and (f2[:, 6:] == 10 + np.arange(4)[:, None]).all()
    f1, y1 = load_split(Index(), range(4), str(m), None)
    assert f1.shape == (4, 6) and (f1 == f2[:, :6]).all() and (y1 == y2).all()


def test_monitor_flags_default_off_and_refusals():
    from facl_amd.train_common import build_parser, check_knn_flags
    opt = build_parser('0').parse_args([])
    assert (opt.knn_every, opt.knn_k, opt.knn_T) == (0, 20, 0.1)
    check_knn_flags(opt, world=4)                                         # off: nothing to refuse
    opt = build_parser('0').parse_args(["--knn_every", "1", "--synthetic", "1"])
    with pytest.raises(RuntimeError, match="--synthetic 0"):
        check_knn_flags(opt, world=1)
    opt = build_parser('0').parse_args(["--knn_every", "1", "--synthetic", "0"])
    check_knn_flags(opt, world=1)
    with pytest.raises(RuntimeError, match="one rank"):
        check_knn_flags(opt, world=2)


def test_cpu_tensors_raise():
    from facl_amd import knn_eval
    q, x, y = torch.zeros(4, 64), torch.zeros(8, 64), torch.zeros(8, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="GPU only"):
        knn_eval.knn_topk(q, x, 2)
    with pytest.raises(RuntimeError, match="GPU only"):
        knn_eval.knn_predict(q, x, y, k=2, num_class=3)
    with pytest.raises(RuntimeError, match="GPU only"):
        knn_eval.knn_top1(q, y[:4], x, y, k=2)
    with pytest.raises(RuntimeError, match="GPU only"):
        knn_eval.knn_vote(torch.zeros(4, 2), torch.zeros(4, 2, dtype=torch.int32), y, 3)
