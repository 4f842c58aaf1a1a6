"""Momentum key encoder (--key_encoder), host side: the C ABI symbol facl_ema_apply and its refusals (all before any launch,
so they run without a device), the flag checks of the training entries and the parser defaults.

The refusal codes are the header's: FACL_E_NULL (-2) for a null array or entry, FACL_E_SHAPE (-1) for a count, a size or a
momentum outside the domain -- the values every other entry of include/facl_hip.h returns for them."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_SHAPE, E_NULL = -1, -2


def _lib():
    from facl_amd import _lib, build
    build.build()
    return _lib, _lib.load_library()


def _arrays(nt, n=8, null_at=None, which=0):
    """(pk, p, n) host arrays of nt entries with non-NULL addresses (nothing is launched, nothing is dereferenced)."""
    addr = [[4096 + 64 * i for i in range(nt)] for _ in range(2)]
    if null_at is not None:
        addr[which][null_at] = None
    arr = ctypes.c_void_p * max(nt, 1)
    return arr(*addr[0]), arr(*addr[1]), (ctypes.c_int * max(nt, 1))(*([n] * nt))


def test_header_codes_and_symbol_are_declared_bound_and_exported():
    _l, lib = _lib()
    hdr = open(os.path.join(ROOT, "include", "facl_hip.h")).read()
    assert re.search(r"#define\s+FACL_E_SHAPE\s+\(%d\)" % E_SHAPE, hdr) and re.search(r"#define\s+FACL_E_NULL\s+\(%d\)" % E_NULL, hdr)
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"int\s+facl_ema_apply\s*\(([^)]*)\)", hdr)
    assert m
    assert "facl_ema_apply" in _l.SIGNATURES and hasattr(lib, "facl_ema_apply")
    assert len(m.group(1).split(",")) == len(_l.SIGNATURES["facl_ema_apply"]) == 6
    assert "facl_ema_apply" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_ema_refuses_null_arrays_and_null_entries():
    _l, lib = _lib()
    pk, p, n = _arrays(3)
    for args in ((None, p, n), (pk, None, n), (pk, p, None)):
        assert lib.facl_ema_apply(3, *args, 0.5, None) == E_NULL, args
    for which in (0, 1):
        for at in (0, 2):
            a = _arrays(3, null_at=at, which=which)
            assert lib.facl_ema_apply(3, *a, 0.5, None) == E_NULL, (which, at)


def test_ema_refuses_counts_sizes_and_momenta_outside_the_domain():
    _l, lib = _lib()
    pk, p, n = _arrays(65)
    for nt in (0, 65, -1):
        assert lib.facl_ema_apply(nt, pk, p, n, 0.5, None) == E_SHAPE, nt
    pk, p, n = _arrays(3)
    n[1] = 0
    assert lib.facl_ema_apply(3, pk, p, n, 0.5, None) == E_SHAPE
    n[1] = -5
    assert lib.facl_ema_apply(3, pk, p, n, 0.5, None) == E_SHAPE
    pk, p, n = _arrays(3)
    for m in (-0.1, 1.5, float("nan"), float("inf")):
        assert lib.facl_ema_apply(3, pk, p, n, m, None) == E_SHAPE, m


def test_parser_defaults():
    from facl_amd.train_common import build_parser
    o = build_parser('0').parse_args([])
    assert o.key_encoder == 0 and o.key_momentum == 0.999


def test_check_key_flags():
    from facl_amd.train_common import build_parser, check_key_flags
    p = build_parser('0')
    check_key_flags(p.parse_args([]), world=1)
    check_key_flags(p.parse_args([]), world=2)                             # off: nothing to refuse
    check_key_flags(p.parse_args(["--key_momentum", "7"]), world=1)        # off: the momentum is not read
    ok = ["--neg_queue", "64", "--batchSize", "32", "--key_encoder", "1"]
    check_key_flags(p.parse_args(ok), world=1)
    check_key_flags(p.parse_args(ok + ["--key_momentum", "0"]), world=1)
    with pytest.raises(RuntimeError, match="neg_queue"):
        check_key_flags(p.parse_args(["--key_encoder", "1"]), world=1)
    for m in ("1", "1.5", "-0.1", "nan"):
        with pytest.raises(RuntimeError, match="key_momentum"):
            check_key_flags(p.parse_args(ok + ["--key_momentum", m]), world=1)
    with pytest.raises(RuntimeError, match="one rank"):
        check_key_flags(p.parse_args(ok), world=2)


def test_training_entries_refuse_before_the_device(monkeypatch):
    from facl_amd import cn3d_train_apperance_GL, cn3d_train_motion_GL
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    base = ["--synthetic", "1", "--nepoch", "1", "--batchSize", "4", "--key_encoder", "1"]
    for entry in (cn3d_train_motion_GL, cn3d_train_apperance_GL):
        with pytest.raises(RuntimeError, match="neg_queue"):
            entry.main(base)
        with pytest.raises(RuntimeError, match="key_momentum"):
            entry.main(base + ["--neg_queue", "8", "--key_momentum", "1.0"])
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(RuntimeError, match="one rank"):
        cn3d_train_motion_GL.main(base + ["--neg_queue", "8"])


def test_finetune_refuses_the_key_encoder():
    from facl_amd import finetune
    p = finetune.finetune_parser()
    with pytest.raises(RuntimeError, match="contrastive loss"):
        finetune.check_finetune_flags(p.parse_args(["--key_encoder", "1"]), world=1)


def test_step_and_loss_refuse_keys_without_a_queue():
    import torch
    from types import SimpleNamespace
    from facl_amd.train_common import ContrastiveStep, key_checkpoint_name
    from facl_amd.utils_my import contrastive_losses_stacked
    net = torch.nn.Linear(2, 2)
    with pytest.raises(RuntimeError, match="neg_queue"):
        ContrastiveStep(net, None, SimpleNamespace(key_encoder=1, key_momentum=0.5), 4)
    step = ContrastiveStep(net, None, SimpleNamespace(), 4)                # namespaces from before the flags: no key encoder
    assert step.key_momentum is None and step.key_encoder is None
    with pytest.raises(ValueError, match="queue"):
        contrastive_losses_stacked(4, torch.zeros(10, 8), [0, 1, 2, 3], queue_rows=torch.zeros(2, 8))
    assert key_checkpoint_name("/a/b.c/corr_GL_5.pth") == "/a/b.c/corr_GL_5_key.pth"


def test_timing_tool_keeps_the_blocks_it_does_not_produce(tmp_path):
    import importlib.util
    import json
    spec = importlib.util.spec_from_file_location("time_key_encoder", os.path.join(ROOT, "tools", "time_key_encoder.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    out = tmp_path / "k.json"
    out.write_text(json.dumps({"bench_ab": {"parent": [1]}, "queue_graph_ms": 1.0}))
    tool.write_results(str(out), {"queue_graph_ms": 3.0})
    assert json.loads(out.read_text()) == {"bench_ab": {"parent": [1]}, "queue_graph_ms": 3.0}
    with open(os.path.join(ROOT, "profiles", "key_encoder.json")) as f:
        recorded = json.load(f)
    assert len(recorded["bench_ab"]["parent"]) == len(recorded["bench_ab"]["this"]) == 3 and "kernel_trace" in recorded
    assert recorded["key_minus_queue_us"] == 1e3 * (recorded["queue_key_graph_ms"] - recorded["queue_graph_ms"])
