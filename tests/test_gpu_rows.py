"""GPU tests of the BatchNorm row kernels of the encoder tail (csrc/rows.hip) through the C ABI, at the smallest shapes at which
they can go wrong: a channel tail inside a block, fewer rows than row phases, one row, and the one-channel-per-lane fallback,
reached both through C % 4 != 0 and through a tensor that starts one float past a 16-byte boundary."""
import pytest
import torch

from helpers import bn_consts, clear_of_the_relu_edge
from poison import poisoned_scratch  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
E_ALIGN = -3
U32, U64 = 2.0 ** -24, 2.0 ** -52


def _env():
    from facl_amd import _lib
    from facl_amd.sa_mlp import _Workspace
    return _lib, _lib.load_library(), _lib.ptr, _Workspace.get(torch.device(DEV))


def _off16(t):
    """A copy of `t` that starts one float past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


def _rows_case(R, C, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    bnc = bn_consts(C, g)
    y = clear_of_the_relu_edge(torch.randn(R, C, device=DEV, generator=g), bnc)
    dout = torch.randn(R, C, device=DEV, generator=g)
    kk = torch.randn(2, C, device=DEV, generator=g) * 0.1
    return g, bnc, y, dout, kk


def _segmax_case(M, S, C, seed):
    """y (M*S, C), bnc with gammas of both signs, and what the forward keeps: ymax = max_s sgn*y, arg = its first row, xpre."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    bnc = bn_consts(C, g)
    sgn = torch.where(torch.rand(C, device=DEV, generator=g) < 0.4, -1.0, 1.0)
    bnc[4] = sgn
    bnc[2] = bnc[2].abs() * sgn
    y = torch.randn(M * S, C, device=DEV, generator=g)
    sy = (y * sgn).view(M, S, C)
    ymax = sy.max(dim=1).values.contiguous()
    arg = (sy == ymax[:, None, :]).int().argmax(dim=1).to(torch.int32).contiguous()
    xpre = torch.relu(bnc[2].abs() * ymax + bnc[3]).contiguous()
    dxpre = torch.randn(M, C, device=DEV, generator=g)
    kk = torch.randn(2, C, device=DEV, generator=g) * 0.1
    return g, bnc, y, ymax, arg, xpre, dxpre, kk


def _dy_bound(bnc, dz, yhat, kk):
    """Six fp32 roundings in scale * (dz - k1 - yhat * k2)."""
    return 6 * U32 * bnc[2].double().abs() * (dz.abs() + kk[0].double().abs() + yhat.abs() * kk[1].double().abs())


@pytest.mark.parametrize("R,C", [(1, 4), (5, 8), (37, 260), (5, 6)])
def test_rows_bwd_apply_vector_form_equals_scalar_form(R, C):
    """facl_rows_bwd_apply[_amax]: four channels per lane (aligned, C % 4 == 0) and one channel per lane (y one float off
    alignment) give the same bits; the published maximum is max|dy| exactly; the maximum needs the vector form (FACL_E_ALIGN
    otherwise).  C = 6 runs the scalar form in both calls (there the comparison is scalar against scalar).  Every shape is held
    to the fp64 value of the formula: ReLU gate = the sign of the exact scale*y + shift (the sign of the fp32 FMA,
    _lib.tap_relu), bound = six fp32 roundings."""
    _lib, lib, p, ws = _env()
    g, bnc, y, dout, kk = _rows_case(R, C, 100 * R + C)
    dy = _lib.empty(R, C, device=DEV)
    _lib.check(lib.facl_rows_bwd_apply(p(dout), p(y), R, C, p(bnc), p(kk), p(dy), _lib.stream()), "rows_bwd_apply")
    dz = torch.where(y.double() * bnc[2].double() + bnc[3].double() > 0, dout.double(), torch.zeros_like(dout, dtype=torch.float64))
    yhat = (y.double() - bnc[0].double()) * bnc[1].double()
    ref = bnc[2].double() * (dz - kk[0].double() - yhat * kk[1].double())
    err, bound = (dy.double() - ref).abs(), _dy_bound(bnc, dz, yhat, kk)
    print("rows_bwd_apply (%d,%d): max err / bound = %.3f" % (R, C, float((err / bound.clamp_min(1e-300)).max())))
    assert bool((err <= bound).all())
    yo, dy_s = _off16(y), _lib.empty(R, C, device=DEV)
    _lib.check(lib.facl_rows_bwd_apply(p(dout), p(yo), R, C, p(bnc), p(kk), p(dy_s), _lib.stream()), "rows_bwd_apply scalar")
    assert torch.equal(dy, dy_s)
    amax = torch.zeros(_lib.AMAX_WORDS, dtype=torch.int32, device=DEV)
    assert lib.facl_rows_bwd_apply_amax(p(dout), p(yo), R, C, p(bnc), p(kk), p(dy_s), p(amax), _lib.stream()) == E_ALIGN
    dy_a = _lib.empty(R, C, device=DEV)
    rc = lib.facl_rows_bwd_apply_amax(p(dout), p(y), R, C, p(bnc), p(kk), p(dy_a), p(amax), _lib.stream())
    if C % 4:
        assert rc == E_ALIGN
    else:
        _lib.check(rc, "rows_bwd_apply_amax")
        assert torch.equal(dy, dy_a)
        assert float(amax.view(torch.float32).max()) == float(dy.abs().max())


@pytest.mark.parametrize("M,S,C", [(3, 5, 8), (2, 64, 260), (3, 5, 6)])
def test_segmax_bwd_apply_vector_form_equals_scalar_form(M, S, C):
    """facl_segmax_bwd_apply[_amax]: the same properties as the rows entry; dz lives at the argmax row only."""
    _lib, lib, p, ws = _env()
    g, bnc, y, ymax, arg, xpre, dxpre, kk = _segmax_case(M, S, C, 100 * M + C)
    dy = _lib.empty(M * S, C, device=DEV)
    args = lambda y_, dy_: (p(dxpre), p(xpre), p(y_), p(arg), M, S, C, p(bnc), p(kk), p(dy_))
    _lib.check(lib.facl_segmax_bwd_apply(*args(y, dy), _lib.stream()), "segmax_bwd_apply")
    d = torch.where(xpre > 0, dxpre, torch.zeros_like(dxpre)).double()
    at = torch.arange(S, device=DEV).view(1, S, 1) == arg.long().view(M, 1, C)
    dz = (at * d.view(M, 1, C)).view(M * S, C)
    yhat = (y.double() - bnc[0].double()) * bnc[1].double()
    ref = bnc[2].double() * (dz - kk[0].double() - yhat * kk[1].double())
    err, bound = (dy.double() - ref).abs(), _dy_bound(bnc, dz, yhat, kk)
    print("segmax_bwd_apply (%d,%d,%d): max err / bound = %.3f" % (M, S, C, float((err / bound.clamp_min(1e-300)).max())))
    assert bool((err <= bound).all())
    yo, dy_s = _off16(y), _lib.empty(M * S, C, device=DEV)
    _lib.check(lib.facl_segmax_bwd_apply(*args(yo, dy_s), _lib.stream()), "segmax_bwd_apply scalar")
    assert torch.equal(dy, dy_s)
    amax = torch.zeros(_lib.AMAX_WORDS, dtype=torch.int32, device=DEV)
    assert lib.facl_segmax_bwd_apply_amax(*args(yo, dy_s), p(amax), _lib.stream()) == E_ALIGN
    dy_a = _lib.empty(M * S, C, device=DEV)
    rc = lib.facl_segmax_bwd_apply_amax(*args(y, dy_a), p(amax), _lib.stream())
    if C % 4:
        assert rc == E_ALIGN
    else:
        _lib.check(rc, "segmax_bwd_apply_amax")
        assert torch.equal(dy, dy_a)
        assert float(amax.view(torch.float32).max()) == float(dy.abs().max())


def _assert_sums(name, got, terms, n):
    """The kernels add exact fp32 x fp32 products in fp64, so only the summation order separates them from the fp64 sum of the
    same terms (n rows x ... per column): |got - ref| <= n * 2^-52 * sum |term|."""
    ref, bound = terms.sum(0), n * U64 * terms.abs().sum(0)
    err = (got - ref).abs()
    print("%s: max err / bound = %.3f" % (name, float((err / bound.clamp_min(1e-300)).max())))
    assert bool((err <= bound).all()), name


@pytest.mark.parametrize("R,C", [(1, 4), (3, 8), (130, 260), (5, 6)])
def test_rows_statistics_against_fp64(R, C):
    """facl_rows_stats (sum, sum of squares) and facl_rows_bwd_stats (sum dz, sum dz * yhat) per column, the latter in the vector
    form and in the scalar form (C % 4 != 0, or y one float off alignment).  yhat = (y - mean) * invstd is evaluated in torch fp32:
    the kernel's two roundings."""
    _lib, lib, p, ws = _env()
    g, bnc, y, dout, kk = _rows_case(R, C, 7 * R + C)
    sums = _lib.empty(C, 2, dtype=torch.float64, device=DEV)
    _lib.check(lib.facl_rows_stats(p(y), R, C, p(sums), p(ws), _lib.stream()), "rows_stats")
    _assert_sums("rows_stats sum", sums[:, 0], y.double(), R)
    _assert_sums("rows_stats sumsq", sums[:, 1], y.double() * y.double(), R)
    d = torch.where(y.double() * bnc[2].double() + bnc[3].double() > 0, dout, torch.zeros_like(dout)).double()
    yhat = ((y - bnc[0]) * bnc[1]).double()
    for form, y_ in (("aligned", y), ("off16", _off16(y))):
        sums = _lib.empty(C, 2, dtype=torch.float64, device=DEV)
        _lib.check(lib.facl_rows_bwd_stats(p(dout), p(y_), R, C, p(bnc), p(sums), p(ws), _lib.stream()), "rows_bwd_stats")
        _assert_sums("rows_bwd_stats %s sum dz" % form, sums[:, 0], d, R)
        _assert_sums("rows_bwd_stats %s sum dz*yhat" % form, sums[:, 1], d * yhat, R)


@pytest.mark.parametrize("M,S,C", [(3, 5, 6), (7, 64, 256)])
def test_segmax_statistics_against_fp64(M, S, C):
    """facl_segmax_bwd_stats (y gathered through arg) and facl_segmax_bwd_stats_ymax (from the kept maxima): bit-equal to each
    other and within the summation-order bound of the fp64 sums."""
    _lib, lib, p, ws = _env()
    g, bnc, y, ymax, arg, xpre, dxpre, kk = _segmax_case(M, S, C, 13 * M + C)
    s1, s2 = _lib.empty(C, 2, dtype=torch.float64, device=DEV), _lib.empty(C, 2, dtype=torch.float64, device=DEV)
    _lib.check(lib.facl_segmax_bwd_stats(p(dxpre), p(xpre), p(y), p(arg), M, S, C, p(bnc), p(s1), p(ws), _lib.stream()),
               "segmax_bwd_stats")
    _lib.check(lib.facl_segmax_bwd_stats_ymax(p(dxpre), p(xpre), p(ymax), M, C, p(bnc), p(s2), p(ws), None, 0, _lib.stream()),
               "segmax_bwd_stats_ymax")
    assert torch.equal(s1, s2)
    d = torch.where(xpre > 0, dxpre, torch.zeros_like(dxpre)).double()
    v = torch.gather(y.view(M, S, C), 1, arg.long().view(M, 1, C)).squeeze(1)
    yhat = ((v - bnc[0]) * bnc[1]).double()
    _assert_sums("segmax_bwd_stats sum dz", s1[:, 0], d, M)
    _assert_sums("segmax_bwd_stats sum dz*yhat", s1[:, 1], d * yhat, M)
    assert float(s1.abs().sum()) > 0


@pytest.mark.parametrize("R,C", [(5, 8), (130, 260)])
def test_rows_center_wgrad_against_fp64(R, C):
    """facl_rows_center_wgrad: dWc[c][j] = sum_r dy[r][c] * centers[r][j]."""
    _lib, lib, p, ws = _env()
    g = torch.Generator(device=DEV).manual_seed(R + C)
    dy = torch.randn(R, C, device=DEV, generator=g)
    ctr = torch.randn(R, 3, device=DEV, generator=g)
    dWc = _lib.empty(C, 3, dtype=torch.float64, device=DEV)
    _lib.check(lib.facl_rows_center_wgrad(p(dy), p(ctr), R, C, p(dWc), p(ws), _lib.stream()), "rows_center_wgrad")
    terms = dy.double().view(R, C, 1) * ctr.double().view(R, 1, 3)
    _assert_sums("rows_center_wgrad", dWc, terms, R)
    assert lib.facl_rows_center_wgrad(p(_off16(dy)), p(ctr), R, C, p(dWc), p(ws), _lib.stream()) == E_ALIGN


@pytest.mark.parametrize("M,S,C", [(3, 5, 6), (2, 64, 260)])
def test_rows_segmax_first_maximum_wins_and_nan_stays(M, S, C):
    """facl_rows_segmax: x_pre = relu(|scale| * max_s(sgn * y) + shift) with the FIRST row that attains the maximum as arg
    (values drawn from three levels: most columns have ties); strictly greater, or NaN, replaces, so in a column that holds NaNs
    the LAST NaN wins and x_pre is NaN.  The value is the fp32 FMA, restated as the fp64 expression rounded once."""
    _lib, lib, p, ws = _env()
    g = torch.Generator(device=DEV).manual_seed(M * S + C)
    bnc = bn_consts(C, g)
    sgn = torch.where(torch.rand(C, device=DEV, generator=g) < 0.4, -1.0, 1.0)
    bnc[4] = sgn
    bnc[2] = bnc[2].abs() * sgn
    y = torch.randint(0, 3, (M * S, C), device=DEV, generator=g).float()
    nan_col, nan_rows = C - 2, [1, S - 2]
    y.view(M, S, C)[:, nan_rows, nan_col] = float("nan")
    out = _lib.empty(M, C, device=DEV)
    arg = _lib.empty(M, C, dtype=torch.int32, device=DEV)
    _lib.check(lib.facl_rows_segmax(p(y), M, S, C, p(bnc), p(out), p(arg), _lib.stream()), "rows_segmax")
    sy = (y * sgn).view(M, S, C)
    clean = torch.nan_to_num(sy, nan=-1e30)
    best = clean.max(dim=1).values
    first = (clean == best[:, None, :]).int().argmax(dim=1)
    assert int((clean == best[:, None, :]).sum(1).max()) > 1                     # ties really occurred
    first[:, nan_col] = nan_rows[-1]
    best[:, nan_col] = float("nan")
    assert torch.equal(arg.long(), first)
    want = torch.relu((bnc[2].abs().double() * best.double() + bnc[3].double()).float())
    assert bool(torch.isnan(out[:, nan_col]).all())
    assert torch.equal(torch.nan_to_num(out, nan=-1.0), torch.nan_to_num(want, nan=-1.0))
