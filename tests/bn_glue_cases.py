"""The cases of tests/test_gpu_bn_glue.py: seeded NumPy inputs for the small fp64 kernels between the heavy BatchNorm passes
(csrc/finalize.hip and the finalize / constants kernels of csrc/fchead.hip), called through `_lib`.  `run_group(name)` returns
{"<group>/<case>/<output>": ndarray}; tools/make_bn_glue_goldens.py records the same dictionary as tests/golden/bn_glue_parent.npz.
Every output buffer starts from a pattern (NaN floats, 0x01010101 words) so that a word a kernel stops writing, or starts
writing, shows."""
import numpy as np
import torch

from facl_amd import _lib

EPS, MOM = 1e-5, 0.1
WORDS = _lib.AMAX_WORDS
DEV = "cuda:0"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _nan(shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def _words(fill=0x01010101):
    return torch.full((WORDS,), fill, dtype=torch.int32, device=DEV)


def _np(t):
    a = t.cpu().numpy()
    return a.view(np.uint32) if a.dtype == np.int32 else a


def _call(name, *args):
    lib = _lib.load_library()
    args = [_lib.ptr(a) if a is None or isinstance(a, torch.Tensor) else a for a in args]
    _lib.check(getattr(lib, name)(*args, _lib.stream()), name)


def _affine(r, C):
    """gamma with one negative and one zero entry, beta"""
    g = (r.rand(C) + 0.5).astype(np.float32)
    g[2], g[3] = -g[2], 0.0
    return g, r.randn(C).astype(np.float32)


def _bn_sums(r, C, count):
    """(C, 2) fp64 (sum, sumsq) of `count` numbers per channel; channel 1's sumsq / count - mean^2 comes out slightly negative"""
    mean, var = r.randn(C), r.rand(C) + 0.1
    var[1] = 0
    if count == 1:
        var[:] = 0
    sums = np.stack([mean * count, (var + mean * mean) * count], 1)
    sums[1, 1] *= 1 - 8e-16
    m = sums[1, 0] / count
    assert sums[1, 1] / count - m * m < 0
    return sums


def _bnc(r, C):
    """(5, C) constants of a finished layer"""
    g, b = _affine(r, C)
    mean, inv = r.randn(C), 1 / np.sqrt(r.rand(C) + 0.1)
    return np.stack([mean, inv, g * inv, b - mean * g * inv, np.where(g < 0, -1.0, 1.0)]).astype(np.float32)


def _prev(r, kind, n):
    if kind == "null":
        return None
    p = r.randn(n).astype(np.float32)
    if kind == "inf":
        p[n // 3] = np.inf
    if kind == "nan":                                   # an amax buffer whose flag word facl_absmax raised
        p = np.abs(p)
        p[1] = np.nan
    return p


def finalize():
    out = {}
    variants = [(C, count, "base") for C in (64, 68, 1100) for count in (1, 2, 49152)]
    variants += [(68, 49152, v) for v in ("no_running", "no_aamax", "no_zamax", "prev_finite", "prev_inf")]
    variants += [(1100, 2, "prev_finite"), (1100, 2, "prev_inf"), (1100, 49152, "no_running")]
    for C, count, v in variants:
        r = np.random.RandomState(1000 + C + count % 97)
        sums, (g, b) = _dev(_bn_sums(r, C, count)), map(_dev, _affine(r, C))
        rm, rv = (None, None) if v == "no_running" else (_dev(r.randn(C).astype(np.float32)), _dev((r.rand(C) + 0.5).astype(np.float32)))
        aamax, zamax = None if v == "no_aamax" else _words(), None if v == "no_zamax" else _words()
        prev = _prev(r, v[5:] if v.startswith("prev_") else "null", 2 * C)
        bnc = _nan((5, C))
        _call("facl_bn_finalize_after", sums, C, float(count), g, b, EPS, MOM, rm, rv, bnc, aamax, zamax,
              None if prev is None else _dev(prev), 0 if prev is None else prev.size)
        for k, t in (("bnc", bnc), ("rm", rm), ("rv", rv), ("aamax", aamax), ("zamax", zamax)):
            if t is not None:
                out[f"finalize/C{C}_n{count}_{v}/{k}"] = _np(t)
    return out


def eval_consts():
    out = {}
    for C in (64, 68, 1100):
        for kind in ("null", "finite", "nan"):
            r = np.random.RandomState(2000 + C)
            (g, b) = map(_dev, _affine(r, C))
            rm, rv = _dev(r.randn(C).astype(np.float32)), _dev((r.rand(C) + 0.5).astype(np.float32))
            prev = _prev(r, kind, WORDS)
            bnc = _nan((5, C))
            _call("facl_bn_eval_consts_after", C, g, b, rm, rv, EPS, bnc, None if prev is None else _dev(prev),
                  0 if prev is None else prev.size)
            out[f"eval_consts/C{C}_prev_{kind}/bnc"] = _np(bnc)
    return out


def _layer1(r, D, P=1000):
    x = r.randn(P, D)
    mom = np.concatenate([x.sum(0), (x.T @ x).reshape(-1)])
    return mom, (r.randn(64, D) * 0.5).astype(np.float32), r.randn(64).astype(np.float32), float(P)


def bn1():
    out = {}
    for D in (3, 4, 5, 8):
        r = np.random.RandomState(3000 + D)
        mom, W1, b1, P = _layer1(r, D)
        mom, W1, b1 = _dev(mom), _dev(W1), _dev(b1)
        g, b = map(_dev, _affine(r, 64))
        L = _lib.sa_l1_cols(D)
        sums = _nan((64, 2), torch.float64)
        _call("facl_bn1_sums_from_moments", mom, P, D, W1, b1, sums)
        out[f"bn1/D{D}/sums_from_moments"] = _np(sums)
        for v in ("full", "bare"):                                  # bare: no running buffers, no activation bound
            rm, rv = (_dev(r.randn(64).astype(np.float32)), _dev((r.rand(64) + 0.5).astype(np.float32))) if v == "full" else (None, None)
            aamax = _words() if v == "full" else None
            sums, bnc, tab = _nan((64, 2), torch.float64), _nan((5, 64)), _nan((64, L))
            _call("facl_sa_bn1_chain", mom, P, D, W1, b1, g, b, EPS, MOM, rm, rv, sums, bnc, aamax, tab)
            for k, t in (("sums", sums), ("bnc", bnc), ("tab", tab), ("rm", rm), ("rv", rv), ("aamax", aamax)):
                if t is not None:
                    out[f"bn1/D{D}/chain_{v}/{k}"] = _np(t)
        c = _bnc(r, 64)
        xamax = torch.zeros(WORDS, dtype=torch.int32, device=DEV)
        xamax[::WORDS // 64] = _dev(np.abs(r.randn(64)).astype(np.float32).view(np.int32))
        for affine in (False, True):
            for bound in (False, True):
                tab, a1amax = _nan((64, L)), _words() if bound else None
                _call("facl_sa_l1tab", W1, b1, D, _dev(c[2]) if affine else None, _dev(c[3]) if affine else None, tab,
                      xamax if bound else None, a1amax)
                out[f"bn1/D{D}/l1tab_affine{int(affine)}_bound{int(bound)}/tab"] = _np(tab)
                if bound:
                    out[f"bn1/D{D}/l1tab_affine{int(affine)}_bound1/a1amax"] = _np(a1amax)
    return out


def bwd_consts():
    out = {}
    for C in (64, 300):
        for P in (1, 49152):
            r = np.random.RandomState(4000 + C + P % 89)
            sl, sg = _dev(r.randn(C, 2) * 30), _dev(r.randn(C, 2) * 60)          # local sums != global sums
            dbeta, dgamma, kk = _nan((C,)), _nan((C,)), _nan((2, C))
            _call("facl_bn_bwd_consts", sl, sg, C, float(P), dbeta, dgamma, kk)
            for k, t in (("dbeta", dbeta), ("dgamma", dgamma), ("kk", kk)):
                out[f"bwd_consts/C{C}_P{P}/{k}"] = _np(t)
        r = np.random.RandomState(4500 + C)
        sums, bnc = _dev(r.randn(C, 2) * 30), _dev(_bnc(r, C))
        dbeta, dgamma, dbias, kk = _nan((C,)), _nan((C,)), _nan((C,)), _nan((2, C))
        _call("facl_bn_bwd_consts_frozen", sums, bnc, C, dbeta, dgamma, dbias, kk)
        for k, t in (("dbeta", dbeta), ("dgamma", dgamma), ("dbias", dbias), ("kk", kk)):
            out[f"bwd_consts/C{C}_frozen/{k}"] = _np(t)
    return out


def sa_consts():
    r = np.random.RandomState(5000)
    P = 49152.0
    sums0, bnc3 = _dev(r.randn(256, 2) * 30), _dev(_bnc(r, 256))
    W3, b3 = _dev((r.randn(256, 64) * 0.2).astype(np.float32)), _dev(r.randn(256).astype(np.float32))
    sums1, bnc2 = _dev(r.randn(64, 2) * 30), _dev(_bnc(r, 64))
    out = {}
    for frozen in (False, True):
        G3, h3, bw2 = _nan((64, 64)), _nan((64,)), _nan((4, 64))
        if frozen:
            _call("facl_sa_bwd_consts3_frozen", G3, h3)
            _call("facl_sa_bwd_consts2_frozen", bnc2, bw2)
        else:
            _call("facl_sa_bwd_consts3", sums0, bnc3, W3, b3, P, G3, h3)
            _call("facl_sa_bwd_consts2", sums1, bnc2, P, bw2)
        tag = "sa_consts/frozen" if frozen else "sa_consts/train"
        out.update({f"{tag}/G3": _np(G3), f"{tag}/h3": _np(h3), f"{tag}/bw2": _np(bw2)})
    return out


def sa_final():
    out = {}
    r = np.random.RandomState(6000)                     # the D-independent inputs are shared by the four D
    P = 49152.0
    out3 = _dev(r.randn(256 * 64 + 64 * 64 + 64) * 20)
    s0g, s0l, bnc3 = _dev(r.randn(256, 2) * 60), _dev(r.randn(256, 2) * 30), _dev(_bnc(r, 256))
    W3, b3 = _dev((r.randn(256, 64) * 0.2).astype(np.float32)), _dev(r.randn(256).astype(np.float32))
    dW2_sums, s1, bnc2 = r.randn(4096) * 20, _dev(r.randn(64, 2) * 30), _dev(_bnc(r, 64))
    for D in (3, 4, 5, 8):
        r = np.random.RandomState(6000 + D)
        L = _lib.sa_l1_cols(D)
        mom, W1, b1, _ = _layer1(r, D)
        mom, W1, b1, bnc1 = _dev(mom), _dev(W1), _dev(b1), _dev(_bnc(r, 64))
        R1_l = r.randn(L, 64) * 20
        R1_l[D + 1:] = 0
        R1_g = r.randn(L, 64) * 40                      # R1 after the all-reduce != the local one
        R1_g[D + 1:] = 0
        out2, R1_g = _dev(np.concatenate([dW2_sums, R1_l.reshape(-1)])), _dev(R1_g)
        f = lambda *s: _nan(s)
        o = dict(dW3=f(256, 64), dg3=f(256), dbe3=f(256), dW2=f(64, 64), dg2=f(64), dbe2=f(64), dW1=f(64, D), dg1=f(64), dbe1=f(64))
        _call("facl_sa_bwd_final", out3, s0g, s0l, bnc3, W3, b3, out2, s1, R1_g, mom, bnc1, W1, b1, D, P, *o.values())
        out.update({f"sa_final/D{D}_train/{k}": _np(t) for k, t in o.items()})
        o = dict(dW3=f(256, 64), dg3=f(256), dbe3=f(256), db3=f(256), dW2=f(64, 64), dg2=f(64), dbe2=f(64), db2=f(64),
                 dW1=f(64, D), dg1=f(64), dbe1=f(64), db1=f(64))
        _call("facl_sa_bwd_final_frozen", out3, s0l, bnc3, out2, s1, bnc2, bnc1, W1, b1, D, *o.values())
        out.update({f"sa_final/D{D}_frozen/{k}": _np(t) for k, t in o.items()})
    return out


def fc_head():
    from facl_amd.sa_mlp import _Workspace
    out = {}
    ws = _Workspace.get(torch.device(DEV))
    for M, B, C in ((32, 4, 64), (160, 40, 68)):
        R = M + B
        r = np.random.RandomState(7000 + M)
        y, dact = _dev(r.randn(R, C).astype(np.float32)), _dev(r.randn(R, C).astype(np.float32))
        g, b = map(_dev, _affine(r, C))
        rm0, rv0 = r.randn(C).astype(np.float32), (r.rand(C) + 0.5).astype(np.float32)
        for given in (False, True):                     # statistics from the slice workspace | from given (2, C, 2) totals
            world = 2.0 if given else 1.0
            rm, rv = _dev(rm0), _dev(rv0)
            sums2 = _nan((2, C, 2), torch.float64) if given else None
            _call("facl_fc_bn_stats", y, M, R, C, sums2, ws)
            sums2_g = sums2 * 2 if given else None      # two ranks with the same rows
            bnc2, a = _nan((2, 5, C)), _nan((R, C))
            _call("facl_fc_bn_apply", y, M, R, C, sums2_g, None if given else ws, 0 if given else M // 32, 0 if given else (B + 31) // 32,
                  M * world, B * world, g, b, EPS, MOM, rm, rv, bnc2, a)
            bsums2 = _nan((2, C, 2), torch.float64) if given else None
            _call("facl_fc_bn_bwd_stats", dact, y, M, R, C, bnc2, bsums2, ws)
            bsums2_g = bsums2 * 2 + 0.125 if given else None                     # global sums != local sums
            dgamma, dbeta, kk2, dy = _nan((C,)), _nan((C,)), _nan((2, 2, C)), _nan((R, C))
            _call("facl_fc_bn_bwd_apply", dact, y, M, R, C, bnc2, bsums2_g, ws, M * world, B * world, dgamma, dbeta, kk2, dy)
            for k, t in (("sums2", sums2), ("bnc2", bnc2), ("a", a), ("rm", rm), ("rv", rv), ("bwd_sums2", bsums2), ("dgamma", dgamma),
                         ("dbeta", dbeta), ("kk2", kk2), ("dy", dy)):
                if t is not None:
                    out[f"fc_head/M{M}_B{B}_C{C}_{'given' if given else 'slices'}/{k}"] = _np(t)
    return out


def amax():
    out = {}
    r = np.random.RandomState(8000)
    x = r.randn(1000).astype(np.float32)
    x[17], x[700] = np.inf, np.nan
    for tag, a in (("n1", x[:1] * 3), ("n1000_inf_nan", x)):
        am = torch.zeros(WORDS, dtype=torch.int32, device=DEV)
        _call("facl_absmax", _dev(a), a.size, am)
        out[f"amax/absmax_{tag}/amax"] = _np(am)
    y, sc, sh = r.randn(3, 8).astype(np.float32), r.randn(8).astype(np.float32), r.randn(8).astype(np.float32)
    am = torch.zeros(WORDS, dtype=torch.int32, device=DEV)
    _call("facl_rows_act_amax", _dev(y), 3, 8, _dev(sc), _dev(sh), am)
    out["amax/rows_act_R3_C8/amax"] = _np(am)
    return out


GROUPS = {f.__name__: f for f in (finalize, eval_consts, bn1, bwd_consts, sa_consts, sa_final, fc_head, amax)}


def run_group(name):
    out = GROUPS[name]()
    torch.cuda.synchronize()
    return out
