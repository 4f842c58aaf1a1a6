"""Per-call host cost of facl_amd._lib.call against the written-out ctypes form, without a device:
facl_gather_rows, 12 arguments, refuses on its shape before anything else.  Prints one JSON line.

    python tools/time_host_call.py [calls per round, default 200000]
"""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from facl_amd import _lib  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 200000
ROUNDS = 5
_lib.stream = lambda: 0            # no device here; the same stand-in serves both forms
feat, idx, xyz, out = (torch.zeros(16) for _ in range(4))


def direct():
    lib = _lib.load_library()
    t = time.perf_counter()
    for _ in range(N):
        rc = lib.facl_gather_rows(_lib.ptr(feat), 0, 1, 1, 0, _lib.ptr(idx), 1, _lib.ptr(xyz), _lib.ptr(out), 0, 0, _lib.stream())
        if rc != _lib.E_SHAPE:
            _lib.check(rc, "facl_gather_rows")
    return (time.perf_counter() - t) / N * 1e6


def wrapped():
    acc = (_lib.E_SHAPE,)
    t = time.perf_counter()
    for _ in range(N):
        _lib.call("facl_gather_rows", feat, 0, 1, 1, 0, idx, 1, xyz, out, 0, 0, accept=acc)       # C = 0: FACL_E_SHAPE
    return (time.perf_counter() - t) / N * 1e6


d, w = [], []
for _ in range(ROUNDS):
    d.append(direct())
    w.append(wrapped())
d, w = sorted(d), sorted(w)
print(json.dumps({"entry": "facl_gather_rows", "arguments": 12, "calls": N, "rounds": ROUNDS,
                  "direct_us": [round(x, 3) for x in d], "call_us": [round(x, 3) for x in w],
                  "direct_us_median": round(d[ROUNDS // 2], 3), "call_us_median": round(w[ROUNDS // 2], 3),
                  "delta_us": round(w[ROUNDS // 2] - d[ROUNDS // 2], 3)}))
