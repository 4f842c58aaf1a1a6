"""Host side of the prototype contrastive term (facl_amd/proto.py, --proto_weight): the flag refusals, which come
before the device is touched, the parser defaults, the per-cluster concentrations against a brute-force restatement, and the
header / bindings and argument refusals of the entry, which come before any launch (no GPU here)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLUSTER = ["--loss_mask", "class", "--synthetic", "0", "--class_ids", "cluster", "--clusters", "3", "--cluster_every", "1"]


# ---- flags ------------------------------------------------------------------------------------------------------------------------
def test_parser_defaults():
    from facl_amd.train_common import build_parser
    d = build_parser('0').parse_args([])
    assert (d.proto_weight, d.proto_temperature, d.proto_concentration) == (0.0, 0.2, "cluster")
    with pytest.raises(SystemExit):
        build_parser('0').parse_args(["--proto_concentration", "global"])


def test_entries_refuse_before_the_device(tmp_path, monkeypatch):
    from facl_amd import cn3d_train_apperance_GL as appearance
    from facl_amd import cn3d_train_motion_GL as motion
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    out = str(tmp_path / "ck")
    cases = [
        (["--proto_weight", "1"], "--proto_weight 1 needs --class_ids cluster"),
        (["--proto_weight", "1", "--loss_mask", "class", "--synthetic", "0"], "needs --class_ids cluster"),
        (CLUSTER + ["--proto_weight", "-0.5"], "--proto_weight must be finite and >= 0 \\(got -0.5\\)"),
        (CLUSTER + ["--proto_weight", "nan"], "--proto_weight must be finite and >= 0 \\(got nan\\)"),
        (CLUSTER + ["--proto_weight", "inf"], "--proto_weight must be finite and >= 0"),
        (CLUSTER + ["--proto_weight", "1", "--proto_temperature", "0"], "--proto_temperature must be finite and > 0 \\(got 0.0\\)"),
        (CLUSTER + ["--proto_weight", "1", "--proto_temperature", "nan"], "--proto_temperature must be finite and > 0"),
        (["--proto_temperature", "-1"], "--proto_temperature must be finite and > 0"),
    ]
    for entry in (motion, appearance):
        for args, msg in cases:
            with pytest.raises(RuntimeError, match=msg):
                entry.main(args + ["--save_root_dir", out])
            assert not os.path.exists(out)


def test_check_proto_flags_accepts_and_keeps_the_cluster_refusals():
    from facl_amd.train_common import build_parser, check_proto_flags
    p = build_parser('0')
    check_proto_flags(p.parse_args([]), world=4)                                # off: nothing to refuse
    check_proto_flags(p.parse_args(CLUSTER), world=1)
    check_proto_flags(p.parse_args(CLUSTER + ["--proto_weight", "0.5", "--proto_concentration", "fixed"]), world=1)
    with pytest.raises(RuntimeError, match="--class_ids cluster runs on one rank only"):
        check_proto_flags(p.parse_args(CLUSTER + ["--proto_weight", "0.5"]), world=2)


def test_finetune_refuses_the_weight():
    from facl_amd.finetune import check_finetune_flags, finetune_parser
    for w in ("1", "nan"):
        with pytest.raises(RuntimeError, match="--proto_weight adds the prototype term to the contrastive loss"):
            check_finetune_flags(finetune_parser().parse_args(["--proto_weight", w]), world=1)
    check_finetune_flags(finetune_parser().parse_args(["--proto_weight", "0"]), world=1)


def test_bench_and_dense_do_not_take_the_flags():
    for name in ("bench.py", os.path.join("facl_amd", "dense.py")):
        assert "proto_weight" not in open(os.path.join(ROOT, name)).read(), name


# ---- concentrations ---------------------------------------------------------------------------------------------------------------
def _brute(cos, lab, K, temperature):
    """The definition, element by element, in Python floats (fp64)."""
    phi = []
    for k in range(K):
        d = [math.sqrt(max(0.0, 2.0 - 2.0 * float(c))) for c, l in zip(cos, lab) if l == k]
        phi.append(sum(d) / len(d) / math.log(len(d) + 10.0) if d else 0.0)
    top = max(v for v in phi if v > 0.0)
    phi = sorted((top if v == 0.0 else v, k) for k, v in enumerate(phi))

    def pct(q):                                              # np.percentile's linear rule: position q / 100 (n - 1) of the sorted values
        pos = q / 100.0 * (K - 1)
        lo = int(math.floor(pos))
        hi = min(lo + 1, K - 1)
        return phi[lo][0] + (phi[hi][0] - phi[lo][0]) * (pos - lo)

    lo, hi = pct(10), pct(90)
    out = [0.0] * K
    for v, k in phi:
        out[k] = min(max(v, lo), hi)
    mean = sum(out) / K
    return [temperature * v / mean for v in out], (lo, hi, phi[0][0], phi[-1][0])


def _hand_made_case():
    """K = 22: cluster 3 empty, cluster 5 a singleton sitting on its centroid (cos = 1, d = 0), sizes 1..40 and cosines spread
    from 0.2 to 0.98 so that the 10th / 90th percentile clip moves clusters at both ends (the 90th percentile of 22 values lies
    below the top three, which the two filled-in clusters share with the largest real one)."""
    rng = np.random.RandomState(4)
    sizes = [2, 40, 7, 0, 11, 1, 25, 3, 16, 5, 30, 9, 4, 6, 8, 12, 14, 18, 20, 22, 35, 13]
    tight = [0.96, 0.2, 0.9, 0.0, 0.7, 1.0, 0.5, 0.97, 0.6, 0.3, 0.8, 0.95, 0.25, 0.35, 0.45, 0.55, 0.65, 0.75, 0.85, 0.92, 0.4, 0.98]
    cos, lab = [], []
    for k, (n, c) in enumerate(zip(sizes, tight)):
        for _ in range(n):
            cos.append(1.0 if k == 5 else min(1.0, c + 0.02 * rng.rand()))
            lab.append(k)
    perm = rng.permutation(len(cos))
    return np.asarray(cos, dtype=np.float32)[perm], np.asarray(lab)[perm], len(sizes)     # float32, as the device hands them over


def test_concentrations_against_brute_force():
    from facl_amd.proto import concentrations
    cos, lab, K = _hand_made_case()
    for temperature in (0.2, 0.07):
        want, (lo, hi, smallest, largest) = _brute(cos, lab, K, temperature)
        assert smallest < lo < hi < largest                                            # the clip acts at both ends
        scale = concentrations(cos, lab.astype(np.int32), K, temperature, "cluster")
        assert scale.dtype == np.float32 and scale.shape == (K,)
        phi = 1.0 / scale.astype(np.float64)
        assert np.abs(phi - np.asarray(want)).max() <= 2.0 ** -22 * max(want)         # float32 storage of 1 / phi
        assert abs(phi.mean() - temperature) <= 1e-6 * temperature
        assert (scale > 0).all() and np.isfinite(scale).all()
    # the empty cluster and the singleton on its centroid took the largest phi, which the clip then cut: they sit at the top
    raw = np.asarray(_brute(cos, lab, K, 1.0)[0])
    assert (raw == raw.max()).sum() == 3 and (raw == raw.min()).sum() >= 2
    assert raw[3] == raw.max() and raw[5] == raw.max()
    # float64 cosines of a float32 array give the same answer as the float32 array itself
    assert (concentrations(cos.astype(np.float64), lab, K, 0.2, "cluster") == concentrations(cos, lab, K, 0.2, "cluster")).all()


def test_concentrations_fixed_and_refusals():
    from facl_amd.proto import concentrations
    cos, lab, K = _hand_made_case()
    s = concentrations(cos, lab, K, 0.25, "fixed")
    assert s.dtype == np.float32 and s.shape == (K,) and (s == np.float32(4.0)).all()
    assert (concentrations(None, None, 3, 0.5, "fixed") == np.float32(2.0)).all()      # fixed reads neither argument
    # every cluster empty or on its centroid: one common temperature
    s = concentrations(np.ones(4), np.array([0, 0, 2, 2]), 3, 0.2, "cluster")
    assert np.abs(1.0 / s.astype(np.float64) - 0.2).max() <= 1e-7
    for kw, msg in ((dict(temperature=0.0), "temperature"), (dict(temperature=float("nan")), "temperature"), (dict(mode="pcl"), "mode"),
                    (dict(K=0), "K must be")):
        with pytest.raises(ValueError, match=msg):
            concentrations(**{**dict(cos_own=cos, labels=lab, K=K, temperature=0.2, mode="cluster"), **kw})
    with pytest.raises(ValueError, match="labels must lie in"):
        concentrations(cos, lab + 1, K, 0.2, "cluster")
    with pytest.raises(ValueError, match="differ in length"):
        concentrations(cos[:-1], lab, K, 0.2, "cluster")


# ---- header, bindings, refusals of the entry --------------------------------------------------------------------------------------
def test_header_declares_and_lib_binds_the_entries():
    from facl_amd import _lib
    txt = open(os.path.join(ROOT, "include", "facl_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name, nargs in (("facl_proto_nce_ws_bytes", 1), ("facl_proto_nce", 15)):
        m = re.search(r"(?:int|int64_t)\s+%s\s*\(([^)]*)\)" % name, txt)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name]), name
    assert "facl_proto_nce_ws_bytes" in _lib.RESTYPE_I64


E_SHAPE, E_NULL, E_ALIGN = -1, -2, -3
ARGS = ("stacked", "M", "ld", "C", "B", "classes", "protos", "proto_inv", "scale", "K", "loss", "dstacked", "err", "ws", "stream")


def test_entry_refuses_bad_arguments_before_any_launch():
    """Host buffers stand in for device memory: every call below is refused by the argument checks, which come before the
    first launch, so nothing is ever read through these pointers."""
    from facl_amd import _lib, build
    build.build()
    lib = _lib.load_library()
    raw = (ctypes.c_char * 4096)()
    base = (ctypes.addressof(raw) + 63) & ~63
    ptrs = dict(zip(("stacked", "classes", "protos", "proto_inv", "scale", "loss", "dstacked", "err", "ws"), (base + 256 * i for i in range(9))))
    good = dict(M=8, ld=64, C=64, B=4, K=3, stream=None, **ptrs)
    call = lambda **kw: lib.facl_proto_nce(*[{**good, **kw}[k] for k in ARGS])
    shape_cases = [dict(M=0), dict(M=-8), dict(B=0), dict(B=3), dict(K=0), dict(K=-1), dict(K=1025), dict(C=0), dict(C=32),
                   dict(C=96, ld=96), dict(C=576, ld=576), dict(C=1024, ld=1024), dict(ld=60), dict(ld=66), dict(ld=32)]
    for kw in shape_cases:
        assert call(**kw) == E_SHAPE, kw
    for name in ptrs:
        assert call(**{name: None}) == E_NULL, name
    for name in ("stacked", "protos", "proto_inv", "scale", "dstacked", "ws"):
        assert call(**{name: ptrs[name] + 4}) == E_ALIGN, name
    # precedence: shape, then NULL, then alignment
    assert call(M=0, stacked=None) == E_SHAPE and call(stacked=None, protos=ptrs["protos"] + 4) == E_NULL
    # the workspace: one double per tile of 16 rows, rounded up to 256 bytes
    assert lib.facl_proto_nce_ws_bytes(1) == 256 and lib.facl_proto_nce_ws_bytes(800) == 512 and lib.facl_proto_nce_ws_bytes(16 * 32 + 1) == 512
    assert lib.facl_proto_nce_ws_bytes(0) == E_SHAPE and lib.facl_proto_nce_ws_bytes(-5) == E_SHAPE


def test_wrapper_refuses_cpu_tensors():
    import torch
    from facl_amd import proto
    with pytest.raises(RuntimeError, match="GPU only"):
        proto.proto_nce(torch.zeros(8, 64), torch.zeros(4, dtype=torch.int32), torch.zeros(3, 64), torch.ones(3), torch.ones(3))
