"""The host launch layer (facl_amd/_lib.py: call, call_size) on entries that complete or refuse before any launch: argument
conversion, the stream slot, return codes, the size entries, the stream marks of SIGNATURES against the header, and the
lookup through `load_library` at call time."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# facl_cls_gather_norm_fwd(stacked, G, B, C, out, inv, stream): C = 96 is outside its domain, FACL_E_SHAPE before the pointers
REFUSED = (None, 2, 3, 96, None, None)


@pytest.fixture
def streams(monkeypatch):
    """_lib.stream() without a device: every call is counted and gives the NULL stream."""
    from facl_amd import _lib
    asked = []
    monkeypatch.setattr(_lib, "stream", lambda: asked.append(1) or 0)
    return asked


def test_tensors_become_their_addresses():
    """(a) facl_view_recipe_table (host only) through `call` with CPU tensors writes what the direct ctypes call writes."""
    from facl_amd import _lib
    from facl_amd.philox import Recipe
    lib = _lib.load_library()
    for kinds in ("reference", "scale,tilt_neg,tilt_pos,jitter,rot,mirror,t7"):
        k = Recipe.parse(kinds).codes()
        t = np.full((len(k), 8), -9, dtype=np.int32)
        stride = ctypes.c_int32(-9)
        assert lib.facl_view_recipe_table(k.ctypes.data, len(k), t.ctypes.data, ctypes.addressof(stride)) == 0
        tk, tt, ts = torch.from_numpy(k.copy()), torch.full((len(k), 8), -9, dtype=torch.int32), torch.full((1,), -9, dtype=torch.int32)
        assert _lib.call("facl_view_recipe_table", tk, len(k), tt, ts) == 0
        np.testing.assert_array_equal(tt.numpy(), t)
        assert int(ts) == stride.value
    # None stays NULL (FACL_E_NULL), a raw address goes through as it is
    with pytest.raises(RuntimeError, match=r"facl_view_recipe_table failed: NULL pointer \(code -2\)"):
        _lib.call("facl_view_recipe_table", None, 1, tt, ts)
    assert _lib.call("facl_view_recipe_table", tk.data_ptr(), len(k), tt.data_ptr(), ts) == 0


def test_the_stream_slot(streams):
    """(b) one argument short: the current stream is appended; `stream=` names another; any other count is a TypeError."""
    from facl_amd import _lib
    assert _lib.call("facl_cls_gather_norm_fwd", *REFUSED, accept=(_lib.E_SHAPE,)) == _lib.E_SHAPE
    assert len(streams) == 1
    assert _lib.call("facl_cls_gather_norm_fwd", *REFUSED, stream=0, accept=(_lib.E_SHAPE,)) == _lib.E_SHAPE
    assert len(streams) == 1                                            # an explicit stream: the current one is not asked for
    for args in (REFUSED[:-1], REFUSED + (None, None)):
        with pytest.raises(TypeError, match="facl_cls_gather_norm_fwd"):
            _lib.call("facl_cls_gather_norm_fwd", *args)
    with pytest.raises(TypeError, match="facl_view_recipe_table"):      # no stream slot: nothing is appended
        _lib.call("facl_view_recipe_table", None, 1, None)
    assert len(streams) == 1


def test_return_codes(streams):
    """(c) a refusal raises under the entry's name with the detail; a code listed in `accept` is returned instead."""
    from facl_amd import _lib
    with pytest.raises(RuntimeError) as e:
        _lib.call("facl_cls_gather_norm_fwd", *REFUSED, detail="G=2, B=3, C=96")
    assert str(e.value) == "facl_cls_gather_norm_fwd(G=2, B=3, C=96) failed: unsupported shape (code -1)"
    with pytest.raises(RuntimeError, match=r"^facl_cls_gather_norm_fwd failed: unsupported shape \(code -1\)$"):
        _lib.call("facl_cls_gather_norm_fwd", *REFUSED, accept=(_lib.E_CONFIG,))
    assert _lib.call("facl_cls_gather_norm_fwd", *REFUSED, accept=(_lib.E_SHAPE,)) == _lib.E_SHAPE
    assert _lib.call("facl_cls_gather_norm_fwd", None, 2, 3, 512, None, None, accept=(_lib.E_SHAPE, _lib.E_NULL)) == _lib.E_NULL


def test_size_entries():
    """(d) call_size gives the value inside the domain and raises the entry's refusal outside."""
    from facl_amd import _lib
    lib = _lib.load_library()
    assert _lib.call_size("facl_knn_ws_bytes", 10, 10, 5) == lib.facl_knn_ws_bytes(10, 10, 5) > 0
    assert _lib.call_size("facl_ws_bytes") == lib.facl_ws_bytes() > 0
    with pytest.raises(RuntimeError) as e:
        _lib.call_size("facl_knn_ws_bytes", 10, 10, 65, detail="nq=10, nb=10, k=65")
    assert str(e.value) == "facl_knn_ws_bytes(nq=10, nb=10, k=65) failed: unsupported shape (code -1)"
    with pytest.raises(TypeError, match="facl_knn_ws_bytes"):
        _lib.call_size("facl_knn_ws_bytes", 10, 10)


def test_stream_marks_match_the_header():
    """(e) the last slot of SIGNATURES[name] is c_s exactly for the entries whose last declared parameter is `void* stream`;
    c_s appears nowhere else."""
    from facl_amd import _lib
    txt = open(os.path.join(ROOT, "include", "facl_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    decls = dict(re.findall(r"(?:int|int64_t)\s+(facl_\w+)\s*\(([^)]*)\)", txt))
    assert sorted(decls) == sorted(_lib.SIGNATURES)
    marked = 0
    for name, params in decls.items():
        last = params.split(",")[-1].strip()
        has_stream = re.fullmatch(r"void\s*\*\s*stream", last) is not None
        sig = _lib.SIGNATURES[name]
        assert (bool(sig) and sig[-1] is _lib.c_s) == has_stream, name
        assert _lib.c_s not in sig[:-1], name
        marked += has_stream
    assert marked >= 100 and issubclass(_lib.c_s, ctypes.c_void_p)


class _Calls:
    """The library with every call's name recorded (the proxy of tests/test_gpu_optim_recipe.py: its callables carry no
    argtypes)."""

    def __init__(self, lib):
        self.lib, self.names = lib, []

    def __getattr__(self, name):
        fn = getattr(self.lib, name)

        def call(*a):
            self.names.append(name)
            return fn(*a)
        setattr(self, name, call)
        return call


def test_the_library_is_looked_up_at_call_time(streams, monkeypatch):
    """(f) a stand-in for `load_library` sees the entry of every call that goes through the launch layer."""
    from facl_amd import _lib
    calls = _Calls(_lib.load_library())
    with monkeypatch.context() as m:
        m.setattr(_lib, "load_library", lambda: calls)
        _lib.call("facl_cls_gather_norm_fwd", *REFUSED, accept=(_lib.E_SHAPE,))
        _lib.call_size("facl_knn_ws_bytes", 10, 10, 5)
    _lib.call_size("facl_knn_ws_bytes", 10, 10, 5)                      # the stand-in is gone: not recorded
    assert calls.names == ["facl_cls_gather_norm_fwd", "facl_knn_ws_bytes"]
