"""Philox views at any view count G and cloud size P, the parts that need no GPU: the NumPy restatement's defaults, the
counters of the recipe (view v = kind v % 10 in round v // 10, slots + 32 * round) never collide, the entries refuse other
sizes on the reference's stream before they touch a device, and the four new C-ABI entries are declared and bound."""
import os
import re

import numpy as np
import pytest

from helpers import synth_clip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ["facl_build_views_philox_gp_f32", "facl_build_views_philox_gp_f64",
               "facl_build_views_resident_gp_f32", "facl_build_views_resident_gp_f64"]


def test_draws_defaults_are_the_generalised_call_at_10_by_512():
    from facl_amd.philox import draws
    clip = synth_clip(3, np.float64, 700, 300, 450, 130)
    base = [0, 700, 1000, 1450]
    a = draws(99, 4, 17, *clip, base=base)
    b = draws(99, 4, 17, *clip, base=base, num_crop=10, num_point=512, round=0, first_point=0)
    c = draws(99, 4, 17, *clip, base=base, num_crop=24, num_point=2048, round=0, first_point=0)
    assert a[0].shape == (10, 512) and a[0].dtype == np.int32 and a[1].shape == (7, 512, 3) and a[2].shape == (2, 2)
    for x, y, z in zip(a, b, c):
        np.testing.assert_array_equal(x, y)
        np.testing.assert_array_equal(x, z)                # a view's values depend on neither size
    # another round / another chunk draws other numbers, of the same form
    for kw in (dict(round=1), dict(first_point=512), dict(round=2, first_point=1536)):
        d = draws(99, 4, 17, *clip, base=base, num_crop=24, num_point=2048, **kw)
        assert d[0].shape == (10, 512) and not np.array_equal(d[0], a[0]) and not np.array_equal(d[1], a[1])
    assert not np.array_equal(draws(99, 4, 17, *clip, base=base, num_crop=24, num_point=2048, round=1)[2], a[2])
    for kw in (dict(num_crop=24, round=3), dict(num_crop=10, round=1), dict(num_point=640, first_point=640),
               dict(num_crop=0), dict(num_crop=65), dict(num_point=32), dict(num_point=96), dict(num_point=4160)):
        with pytest.raises(ValueError):
            draws(99, 4, 17, *clip, base=base, **kw)


@pytest.mark.parametrize("G,P", [(24, 2048), (13, 640)])
def test_no_two_draws_share_a_counter(G, P):
    """Every (view, purpose) reads its own words.  At the level of whole counters (n, slot): the only sharing is the
    recipe's own -- the row words of the (up to four) kinds of one row slot of one round are the four words of one counter."""
    from facl_amd.philox import counters
    users = counters(G, P)
    assert {v for v, _ in users} == set(range(G))
    assert sum(1 for _, p in users if p == 'row') == G
    words, owner = {}, {}
    for key, cs in users.items():
        assert cs and all(0 <= n < P and 0 <= w < 4 for n, _, w in cs)
        for c in cs:
            assert c not in words, "word %r read by %r and %r" % (c, words.get(c), key)
            words[c] = key
        for n, slot, _ in cs:
            other = owner.setdefault((n, slot), key)
            if other != key:
                (v0, p0), (v1, p1) = other, key
                assert p0 == 'row' and p1 == 'row' and v0 // 10 == v1 // 10 and (v0 % 10) >> 2 == (v1 % 10) >> 2, \
                    "counter %r shared by %r and %r" % ((n, slot), other, key)
    # rounds never meet: round r owns slots [32 r, 32 r + 26)
    for (v, _), cs in users.items():
        assert all(32 * (v // 10) <= slot < 32 * (v // 10) + 26 for _, slot, _ in cs)


def test_counters_at_10_by_512_are_the_first_block_of_every_size():
    from facl_amd.philox import counters
    small, big = counters(10, 512), counters(24, 2048)
    for key, cs in small.items():
        assert cs == {c for c in big[key] if c[0] < 512}


def test_entry_refuses_other_sizes_on_the_numpy_stream_before_touching_a_device(tmp_path, monkeypatch):
    import torch
    from facl_amd import cn3d_train_motion_GL as train

    def no_device(*a, **k):
        raise AssertionError("the device was touched before the refusal")
    monkeypatch.setattr(torch.cuda, "set_device", no_device)
    base = ["--synthetic", "0", "--data_root", str(tmp_path), "--save_root_dir", str(tmp_path / "ck")]
    with pytest.raises(RuntimeError, match="philox"):
        train.main(base + ["--view_rng", "numpy", "--num_crop", "24"])
    with pytest.raises(RuntimeError, match="philox"):
        train.main(base + ["--view_rng", "numpy", "--SAMPLE_NUM", "2048"])
    with pytest.raises(RuntimeError, match="philox"):
        train.main(["--synthetic", "2", "--view_rng", "device", "--num_crop", "24", "--save_root_dir", str(tmp_path / "ck")])
    for bad in (["--num_crop", "65"], ["--num_crop", "0"], ["--SAMPLE_NUM", "96"], ["--SAMPLE_NUM", "4160"],
                ["--INPUT_FEATURE_NUM", "3"]):
        with pytest.raises(RuntimeError):
            train.main(base + ["--view_rng", "philox"] + bad)
    # inside the domain the philox stream passes the argument checks and goes on to the device
    with pytest.raises(AssertionError, match="device was touched"):
        train.main(base + ["--view_rng", "philox", "--num_crop", "24", "--SAMPLE_NUM", "2048"])


def test_python_layers_refuse_other_sizes_on_the_numpy_stream():
    from facl_amd.dataset import DiskBatches
    from facl_amd.views import build_views
    with pytest.raises(ValueError, match="philox"):
        DiskBatches(None, "", "0", [], "numpy", "cpu", num_crop=24)
    with pytest.raises(ValueError, match="philox"):
        build_views([synth_clip(1, np.float32)], num_point=2048)
    with pytest.raises(ValueError):
        DiskBatches(None, "", "0", [], "philox", "cpu", num_point=96)


def test_resident_reserve_follows_the_step_size():
    from facl_amd import resident as R
    assert R.step_reserve_bytes(32, 10, 512) == R.STEP_RESERVE_BYTES == R.step_reserve_bytes(4, 10, 512)
    assert R.step_reserve_bytes(32, 24, 2048) == -(-R.STEP_RESERVE_BYTES * 96 // 10)
    with pytest.raises(RuntimeError, match="32 x 10 x 512"):
        R.check_budget(10, 5, reserve=R.step_reserve_bytes(32, 24, 2048))


def _header():
    return open(os.path.join(ROOT, "include", "facl_hip.h")).read()


def test_header_and_binding_list_the_four_new_entries():
    from facl_amd import _lib, build
    txt = _header()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"(?:int|int64_t)\s+(facl_\w+)\s*\(", code))
    build.build()
    lib = _lib.load_library()
    for s in NEW_ENTRIES:
        assert s in declared, f"{s} is not declared in include/facl_hip.h"
        assert s in _lib.SIGNATURES, f"{s} has no ctypes signature in facl_amd/_lib.py"
        assert hasattr(lib, s), f"{s} is not exported by the library"
        old = s.replace("_gp_", "_")
        # today's arguments plus (int G, int P)
        assert len(_lib.SIGNATURES[s]) == len(_lib.SIGNATURES[old]) + 2
        args = re.search(re.escape(s) + r"\s*\(([^)]*)\)", code).group(1)
        assert re.search(r"\bint\s+G\b", args) and re.search(r"\bint\s+P\b", args)
        assert len(args.split(",")) == len(_lib.SIGNATURES[s])
    # the comment blocks state the domain
    for s in ("facl_build_views_philox_gp_", "facl_build_views_resident_gp_"):
        block = [c for c in re.findall(r"/\*.*?\*/", txt, flags=re.S) if s + "*" in c]
        assert block and all("1 <= G <= 64" in c and "64 <= P <= 4096" in c and "P % 64 == 0" in c for c in block)
