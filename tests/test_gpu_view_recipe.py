"""The view recipe on the device (csrc/views_point.inc through csrc/views_philox.hip and csrc/views_resident.hip; the
rule and the arithmetic are restated by facl_amd/philox.py): the default recipe is the _gp entries' output bit for bit, every
kind equals the NumPy restatement, the new kinds have the properties their definitions promise without leaning on it, a clip's
views stay local to (seed, epoch, clip id), every refusal comes without a launch, a temporal kind is void at any position,
the resident path equals the disk path, and the training / extraction entries run a recipe end to end."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from helpers import synth_clip
from view_helpers import _Packed, _Pool, _call, _clips, _host, _index, _train_args, _tree

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ULP1 = np.spacing(np.float32(1.0))
FACL_E_SHAPE, FACL_E_NULL = -1, -2
IDS = [5, 17, 4000]
A = "scale,tilt_neg,tilt_pos,jitter,rot,mirror,t7"
B_KINDS = ",".join(["mirror,key_mirror,rot,scale"] * 3)
B_STRENGTHS = dict(jitter_sigma=0.02, jitter_clip=0.03, rot_range=2.0, scale_lo=0.8, scale_hi=1.25, tilt_angle=0.1)
C = "res10,t4,key,raw,res30"


def _recipe(kinds="reference", **kw):
    from facl_amd.philox import Recipe
    return Recipe.parse(kinds, **kw)


def _c_table(recipe):
    from facl_amd import _lib
    k = recipe.codes()
    t = np.full((len(k), _lib.VIEW_TABLE_COLS), -9, dtype=np.int32)
    stride = ctypes.c_int32(-9)
    rc = _lib.load_library().facl_view_recipe_table(k.ctypes.data, len(k), t.ctypes.data, ctypes.addressof(stride))
    assert rc == 0
    return t, stride.value


# ---- 1. the default recipe is today's output ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("G,P", [(10, 512), (13, 640)])
def test_the_default_recipe_is_the_gp_entries_output(G, P, dt):
    clips = _clips(dt)
    pk, pool = _Packed(clips, IDS), _Pool(clips, IDS)
    rc, old, old_idx = pk.call(99, 4, G, P)
    assert rc == 0 and np.isfinite(old).all() and (old_idx >= 0).all()
    rc, new, new_idx = _call(pk, _recipe(), 99, 4, G, P)
    assert rc == 0 and int(pk.err.item()) == 0
    np.testing.assert_array_equal(new, old)
    np.testing.assert_array_equal(new_idx, old_idx)
    rc, rold, rold_idx = pool.call(None, 99, 4, G, P, entry="gp")
    assert rc == 0
    rc, rnew, rnew_idx = pool.call(_recipe(), 99, 4, G, P)
    assert rc == 0 and pool.err.cpu().tolist() == [0, 2 ** 31 - 1]
    np.testing.assert_array_equal(rnew, rold)
    np.testing.assert_array_equal(rnew_idx, rold_idx)
    np.testing.assert_array_equal(rnew, old)                                   # and resident = disk
    # The launchers run the default recipe as a compile-time specialisation.  The reference's list with a strength that none of
    # its kinds reads is NOT the default, so it runs the table-driven code: the same views, bit for bit.
    unread = _recipe("reference", tilt_angle=0.3, scale_hi=1.6)
    assert not unread.is_default()
    rc, tab, tab_idx = _call(pk, unread, 99, 4, G, P)
    assert rc == 0
    np.testing.assert_array_equal(tab, old)
    np.testing.assert_array_equal(tab_idx, old_idx)
    rc, rtab, rtab_idx = pool.call(unread, 99, 4, G, P)
    assert rc == 0
    np.testing.assert_array_equal(rtab, old)
    np.testing.assert_array_equal(rtab_idx, rold_idx)
    if (G, P) == (10, 512):                                                    # the entries without _gp
        rc, first, first_idx = pk.call(99, 4)
        np.testing.assert_array_equal(new, first)
        np.testing.assert_array_equal(new_idx, first_idx)


# ---- 2. every kind against the restatement -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("kinds,kw,G,P,stride", [(A, {}, 9, 640, 32), (B_KINDS, B_STRENGTHS, 14, 64, 64), (C, {}, 5, 128, 32)])
def test_every_kind_equals_the_restatement(kinds, kw, G, P, stride, dt):
    from facl_amd import philox as ph
    recipe = _recipe(kinds, **kw)
    table, st = recipe.table()
    assert st == stride
    ctab, cst = _c_table(recipe)
    np.testing.assert_array_equal(ctab, table)
    assert cst == st
    clips = _clips(dt)
    pk, pool = _Packed(clips, IDS), _Pool(clips, IDS)
    rc, out, idx = _call(pk, recipe, 99, 4, G, P)
    assert rc == 0 and int(pk.err.item()) == 0 and np.isfinite(out).all() and (idx >= 0).all()
    rc, rout, ridx = pool.call(recipe, 99, 4, G, P)
    assert rc == 0
    np.testing.assert_array_equal(rout, out)                                   # one implementation, two kernels
    L = len(table)
    for b, clip in enumerate(clips):
        want, rows = ph.views(recipe, 99, 4, IDS[b], clip, G, P)
        for v in range(G):
            t = table[v % L]
            cloud = int(t[ph.T_SRC]) if t[ph.T_SRC] < 4 else 0
            np.testing.assert_array_equal(idx[b, v] - pk.meta_np[b, cloud], rows[v])
            np.testing.assert_array_equal(ridx[b, v] - pool.table_np[b, cloud], rows[v])
            worst = float(np.abs(out[v, b].astype(np.float64) - want[v]).max())
            print("%s clip %d view %d (%s): max |diff| %.3g" % (np.dtype(dt).name, b, v, recipe.kinds[v % L], worst))
            if t[ph.T_OP] in (ph.OP_ROT, ph.OP_TILT_NEG, ph.OP_TILT_POS):      # the rotation's sum: one float32 spacing
                np.testing.assert_allclose(out[v, b], want[v], rtol=0, atol=ULP1)
            else:
                np.testing.assert_array_equal(out[v, b], want[v])
            if t[ph.T_SRC] >= 4:                                               # temporal rows come from the non-zero rows
                assert (clip[0][rows[v], int(t[ph.T_CH])] != 0).all()


def test_the_c_rule_equals_the_python_rule_for_the_default_and_the_edges():
    for kinds in ("reference", "rot", ",".join(["mirror"] * 12), ",".join(["scale"] * 12), "t4,t7", "raw"):
        r = _recipe(kinds)
        t, s = _c_table(r)
        np.testing.assert_array_equal(t, r.table()[0])
        assert s == r.table()[1]


# ---- 3. properties that do not lean on the restatement -------------------------------------------------------------------------
def _gathered(pk, idx):
    """src[idx] as float64 (B, G, P, 8): the rows the kernel says it drew."""
    return pk.src.cpu().numpy()[idx].astype(np.float64)


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_scale_tilt_and_rot_without_jitter(dt):
    clips = _clips(dt)
    pk = _Packed(clips, IDS)
    lo, hi, tilt = 0.8, 1.25, 0.1
    recipe = _recipe("scale,tilt_neg,tilt_pos,rot", jitter_sigma=0.0, rot_range=0.0, scale_lo=lo, scale_hi=hi, tilt_angle=tilt)
    G, P = 8, 128                                                              # two rounds
    rc, out, idx = _call(pk, recipe, 99, 4, G, P)
    assert rc == 0 and np.isfinite(out).all()
    src = _gathered(pk, idx)                                                   # (B, G, P, 8)
    src32 = src.astype(np.float32)
    M = float(np.abs(src[..., :3]).max())
    sp = float(np.spacing(np.float32(M)))
    factors = {}
    for b in range(3):
        for v in range(G):
            o, x = out[v, b].astype(np.float64), src[b, v]
            np.testing.assert_array_equal(out[v, b, :, 3], src32[b, v, :, 3])  # channel 3 is copied
            if v % 4 == 0:
                # out = x * s * (1 + e), |e| <= 3 * 2^-24: s rounded to S, the product rounded in S, the cast to float32 (each
                # at most 2^-24 relative; S = float64 only makes two of them smaller).  The estimate of s below, a ratio of
                # such a value, carries the same 3 * 2^-24, so |out - s_est x| <= 6 * 2^-24 |s_est x| to first order: 7.
                k = np.unravel_index(np.abs(x[:, :3]).argmax(), (P, 3))
                s = float(o[k] / x[k])
                assert lo * (1 - 2.0 ** -22) <= s < hi * (1 + 2.0 ** -22), (b, v, s)
                err = np.abs(o[:, :3] - s * x[:, :3])
                print("%s clip %d view %d: s %.9f, worst |out - s x| / |s x| %.3g" % (
                    np.dtype(dt).name, b, v, s, float((err / np.maximum(np.abs(s * x[:, :3]), 1e-300)).max())))
                assert (err <= 7 * 2.0 ** -24 * np.abs(s * x[:, :3])).all(), (b, v)
                factors[(b, v)] = s
            elif v % 4 in (1, 2):
                np.testing.assert_array_equal(out[v, b, :, 1], src32[b, v, :, 1])   # y is untouched, exactly
                # radius about y.  Three roundings: the source coordinate cast to float32 (at most sp / 2 per coordinate,
                # sp = the float32 spacing at the cloud's largest coordinate M; none for a float32 source) and the two output
                # coordinates rounded to float32 at a magnitude up to sqrt(2) M, i.e. at most 2 sp / 2 each.  A coordinate
                # error e moves the radius by at most sqrt(2) e (|dr| <= (|x| ex + |z| ez) / r), so |dr| <= sqrt(2) (1/2 + 1)
                # sp = 2.13 sp: 3 spacings.  The rotation itself is fp64.
                r_in = np.hypot(x[:, 0], x[:, 2])
                r_out = np.hypot(o[:, 0], o[:, 2])
                print("%s clip %d view %d: worst |dr| %.3g = %.2f spacings" % (np.dtype(dt).name, b, v,
                                                                               float(np.abs(r_out - r_in).max()),
                                                                               float(np.abs(r_out - r_in).max()) / sp))
                assert (np.abs(r_out - r_in) <= 3 * sp).all()
                assert (np.abs(o[:, 0] - x[:, 0]) > 100 * sp).any()            # and it did turn
                # turning it back by the opposite angle returns the gathered rows within the same bound
                a = np.pi * tilt * (1.0 if v % 4 == 1 else -1.0)              # tilt_neg turned by -pi t: back by +pi t
                c, s_ = np.cos(a), np.sin(a)
                bx, bz = o[:, 0] * c + o[:, 2] * (-s_), o[:, 0] * s_ + o[:, 2] * c
                assert (np.abs(bx - x[:, 0]) <= 3 * sp).all() and (np.abs(bz - x[:, 2]) <= 3 * sp).all()
            else:
                np.testing.assert_array_equal(out[v, b, :, :3], src32[b, v, :, :3])  # rot at rot_range 0: the gathered rows
    # one s per (clip, view): different between clips, between rounds and between epochs
    assert len({round(s, 6) for s in factors.values()}) == len(factors) == 6, factors
    rc, out2, idx2 = _call(pk, recipe, 99, 5, G, P)
    src2 = _gathered(pk, idx2)
    k = np.unravel_index(np.abs(src2[0, 0, :, :3]).argmax(), (P, 3))
    s_next = float(out2[0, 0].astype(np.float64)[k] / src2[0, 0][k])
    assert abs(s_next - factors[(0, 0)]) > 1e-6


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_the_jitter_kind_stays_inside_the_clip(dt):
    pk = _Packed(_clips(dt), IDS)
    rc, out, idx = _call(pk, _recipe("jitter"), 99, 4, 2, 256)
    assert rc == 0
    src = _gathered(pk, idx)
    d = out.transpose(1, 0, 2, 3).astype(np.float64)[..., :3] - src[..., :3]
    sp = float(np.spacing(np.float32(np.abs(src[..., :3]).max() + 0.05)))
    print("%s: |jitter| max %.6f, mean %.6f" % (np.dtype(dt).name, float(np.abs(d).max()), float(np.abs(d).mean())))
    assert (np.abs(d) <= 0.05 + sp).all() and (np.abs(d) > 1e-4).mean() > 0.9
    np.testing.assert_array_equal(out.transpose(1, 0, 2, 3)[..., 3], src[..., 3].astype(np.float32))


# ---- 4. independence -----------------------------------------------------------------------------------------------------------
def test_a_recipes_views_are_local_to_seed_epoch_and_clip_id():
    from facl_amd.views import build_views
    recipe = _recipe(A)
    clips = [synth_clip(10 + b, np.float64, 600 + 50 * b) for b in range(5)]
    small = build_views([clips[2]], philox=(7, 1, [42]), num_crop=9, num_point=640, recipe=recipe).cpu().numpy()
    big = build_views([clips[2]], philox=(7, 1, [42]), num_crop=23, num_point=1280, recipe=recipe).cpu().numpy()
    assert small.shape == (9, 640, 4) and big.shape == (23, 1280, 4) and np.isfinite(big).all()
    np.testing.assert_array_equal(small, big[:9, :640])
    batch = build_views([clips[0], clips[1], clips[3], clips[2], clips[4]], philox=(7, 1, [0, 1, 3, 42, 4]), num_crop=9,
                        num_point=640, recipe=recipe).cpu().numpy()
    np.testing.assert_array_equal(batch.reshape(9, 5, 640, 4)[:, 3], small)
    for other in ((8, 1, [42]), (7, 2, [42]), (7, 1, [43])):                   # seed, epoch, clip id
        o = build_views([clips[2]], philox=other, num_crop=9, num_point=640, recipe=recipe).cpu().numpy()
        for v in range(9):
            assert not np.array_equal(o[v], small[v]), (other, v)
    # and a recipe is not the default: the first view of A is a scale view, not the raw one
    default = build_views([clips[2]], philox=(7, 1, [42]), num_crop=9, num_point=640).cpu().numpy()
    assert not np.array_equal(default[0], small[0])


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_a_bad_recipe_is_refused_without_a_launch(dt):
    clips = _clips(dt)[:2]
    pk, pool = _Packed(clips, [3, 4]), _Pool(clips, [3, 4])
    good = _recipe(A)
    k, s = good.codes(), good.strengths()
    nan, inf = float("nan"), float("inf")

    def st(i, v):
        x = s.copy()
        x[i] = v
        return x

    cases = [("null kinds", FACL_E_NULL, (None, 7, s.ctypes.data)), ("null strengths", FACL_E_NULL, (k.ctypes.data, 7, None)),
             ("no kind", FACL_E_SHAPE, (k.ctypes.data, 0, s.ctypes.data)),
             ("13 kinds", FACL_E_SHAPE, _host(good, kinds=[0] * 13)[1]), ("-1 kinds", FACL_E_SHAPE, (k.ctypes.data, -1, s.ctypes.data))]
    backing = []
    for name, kinds in (("kind 13", [0, 13]), ("kind -1", [-1]), ("kind 99", [4, 99, 0])):
        h = _host(good, kinds=kinds)
        backing.append(h[0])
        cases.append((name, FACL_E_SHAPE, h[1]))
    for name, i, v in (("sigma < 0", 0, -0.01), ("sigma nan", 0, nan), ("clip 0", 1, 0.0), ("clip < 0", 1, -0.05),
                       ("clip inf", 1, inf), ("rot < 0", 2, -0.1), ("rot > 2", 2, 2.01), ("rot nan", 2, nan),
                       ("lo 0", 3, 0.0), ("lo < 0", 3, -1.0), ("lo > hi", 3, 1.6), ("hi inf", 4, inf), ("hi nan", 4, nan),
                       ("tilt nan", 5, nan), ("tilt inf", 5, -inf)):
        h = _host(good, strengths=st(i, v))
        backing.append(h[0])
        cases.append((name, FACL_E_SHAPE, h[1]))
    G, P = 9, 640
    sel = torch.tensor([1, 0], dtype=torch.int32, device=DEV)
    for name, code, extra in cases:
        out = torch.full((G * 2, P, 4), 12345.0, dtype=torch.float32, device=DEV)
        idx = torch.full((2, G, P), -7, dtype=torch.int32, device=DEV)
        rc, o, i = _call(pk, good, 5, 1, G, P, out=out, idx=idx, host=((), extra))
        assert rc == code, name
        assert (o == 12345.0).all() and (i == -7).all(), name                  # poisoned buffers stay as they were
        idx64 = torch.full((2, G, P), -7, dtype=torch.int64, device=DEV)
        rc, o, i = pool.call(good, 5, 1, G, P, sel=sel, out=out, idx=idx64, host=((), extra))
        assert rc == code, name
        assert (o == 12345.0).all() and (i == -7).all() and pool.err.cpu().tolist() == [0, 2 ** 31 - 1], name
    # a size outside the domain is still refused, and the good recipe and the edges of the strengths are accepted
    rc, _, _ = _call(pk, good, 5, 1, 65, 640, out=out, idx=idx)
    assert rc == FACL_E_SHAPE and (out == 12345.0).all()
    for ok in (s, st(0, 0.0), st(2, 0.0), st(2, 2.0), np.array([0.0, 1e-9, 2.0, 1.0, 1.0, -3.0])):
        h = _host(good, strengths=ok)
        rc, o, i = _call(pk, good, 5, 1, G, P, host=h)
        assert rc == 0 and np.isfinite(o).all() and (i >= 0).all()
    # the Python layer refuses before any launch
    from facl_amd.philox import Recipe
    with pytest.raises(ValueError, match="--jitter_clip"):
        Recipe.parse(A, jitter_clip=0.0)


# ---- 6. void temporal views at a non-default position --------------------------------------------------------------------------
def test_a_temporal_kind_is_void_at_any_position():
    good = synth_clip(5, np.float64)
    bad = list(synth_clip(4, np.float64))
    bad[0] = bad[0].copy()
    bad[0][:, 4] = 0
    recipe = _recipe("raw,t4,scale")
    G, P = 7, 128                                                              # three rounds, the last one ragged
    pk = _Packed([good, tuple(bad)], [0, 1], check=False)
    assert int(pk.err.item()) == 1                                             # raised by the compaction
    rc, out, idx = _call(pk, recipe, 1, 0, G, P)
    assert rc == 0
    void = [v for v in range(G) if v % 3 == 1]
    rest = [v for v in range(G) if v % 3 != 1]
    assert void == [1, 4]
    assert (out[void, 1] == 0).all() and (idx[1][void] == -1).all()
    assert np.isfinite(out).all() and (idx[1][rest] >= 0).all() and (idx[0] >= 0).all()
    assert (out[void, 0] != 0).any() and (good[0][idx[0][void] - pk.meta_np[0, 0], 4] != 0).all()   # the other clip's t4 views
    # resident: the ingest raises the word for the clip; built anyway, its t4 views are void in every round
    pool = _Pool([good, tuple(bad)], [0, 1])
    assert pool.err.cpu().tolist() == [1, 1]
    rc, rout, ridx = pool.call(recipe, 1, 0, G, P)
    assert rc == 0
    np.testing.assert_array_equal(rout, out)
    assert (ridx[1][void] == -1).all() and (ridx[1][rest] >= 0).all() and (ridx[0] >= 0).all()


# ---- 7. resident = disk --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kinds,kw,G,P", [(A, {}, 9, 640), (B_KINDS, B_STRENGTHS, 14, 64)])
def test_resident_batches_equal_disk_batches_for_a_recipe(tmp_path, kinds, kw, G, P):
    from facl_amd.dataset import DiskBatches
    from facl_amd.resident import ResidentBatches, ResidentClips
    recipe = _recipe(kinds, **kw)
    _tree(tmp_path, dt=np.float64)
    index, split = _index(tmp_path)
    assert len(split) == 16
    res = ResidentClips(index, str(tmp_path), "0", split, DEV)
    s = np.asarray(split)
    vids = [s[[3, 7, 3, 3, 0]], s[::-1].copy(), s[[15]]]
    it = ResidentBatches(res, vids, seed=2000, epoch=1, num_crop=G, num_point=P, recipe=recipe)
    got = [(v.cpu().numpy(), nm, lb) for v, nm, lb in it]
    it.close()
    want = [(v.cpu().numpy(), nm, lb) for v, nm, lb in
            DiskBatches(index, str(tmp_path), "0", vids, "philox", DEV, seed=2000, epoch=1, prefetch=False, num_crop=G,
                        num_point=P, recipe=recipe)]
    default = [v.cpu().numpy() for v, _, _ in
               DiskBatches(index, str(tmp_path), "0", vids[:1], "philox", DEV, seed=2000, epoch=1, prefetch=False, num_crop=G,
                           num_point=P)]
    assert len(got) == len(want) == 3
    for (a, an, al), (w, wn, wl), v in zip(got, want, vids):
        assert a.dtype == np.float32 and a.shape == w.shape == (G * len(v), P, 4) and np.isfinite(a).all()
        np.testing.assert_array_equal(a, w)
        assert an == wn and al == wl
    assert not np.array_equal(default[0], want[0][0])


# ---- 8. entries ----------------------------------------------------------------------------------------------------------------
def test_entries_train_save_extract_and_refuse_another_recipe(tmp_path, capsys):
    from facl_amd import cn3d_train_motion_GL as train, extract_motion_feature as ext
    names = _tree(tmp_path / "d", rows=(2048, 512, 1024, 256))
    kinds = "scale,tilt_neg,tilt_pos,raw,key,t4"
    rec = ["--view_kinds", kinds, "--jitter_sigma", "0.02", "--save_state_every", "1"]
    sds = {}
    for tag, extra in (("r1", rec + ["--resident", "1"]), ("r0", rec + ["--resident", "0"]), ("def", ["--resident", "0"])):
        ck = tmp_path / ("ck_" + tag)
        net = train.main(_train_args(tmp_path / "d", ck, 13, 640, *extra))
        sds[tag] = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
        printed = capsys.readouterr().out
        loss = [float(x) for x in re.findall(r"--loss: (\S+) \|", printed)]
        assert len(loss) == 1 and np.isfinite(loss[0]), (tag, loss)
        assert os.path.exists(os.path.join(str(ck), "corr_GL_0.pth"))
        if tag == "def":
            assert "view recipe: raw,mirror,key,key_mirror,rot,rot,t4,t7,res30,res10 | jitter_sigma 0.01" in printed
        else:
            assert printed.count("view recipe: %s | jitter_sigma 0.02 jitter_clip 0.05" % kinds) == 1
    for k, v in sds["r1"].items():
        assert torch.isfinite(v.float()).all(), k
        assert torch.equal(v, sds["r0"][k]), k                                 # resident = from disk, bit for bit
    assert any(not torch.equal(v, sds["def"][k]) for k, v in sds["r1"].items() if v.is_floating_point())
    a = torch.load(str(tmp_path / "ck_r1" / "corr_GL_0.pth"), map_location="cpu", weights_only=True)
    b = torch.load(str(tmp_path / "ck_r0" / "corr_GL_0.pth"), map_location="cpu", weights_only=True)
    assert all(torch.equal(a[k], b[k]) for k in a) and set(a) == set(b)
    state = torch.load(str(tmp_path / "ck_r1" / "state_0.pth"), map_location="cpu", weights_only=True)
    want = dict(view_kinds=kinds, jitter_sigma=0.02, jitter_clip=0.05, rot_range=0.8, scale_lo=0.5, scale_hi=1.5, tilt_angle=0.25)
    assert {k: state["flags"][k] for k in want} == want
    # extraction with the recipe: (13 + 1) * 512 floats per clip
    out = tmp_path / "f"
    feats = ext.main(["--synthetic", "0", "--data_root", str(tmp_path / "d"), "--dataset", "ntu120", "--view_rng", "philox",
                      "--num_crop", "13", "--SAMPLE_NUM", "640", "--batchSize", "5", "--view_kinds", kinds, "--jitter_sigma",
                      "0.02", "--checkpoint", str(tmp_path / "ck_r1" / "corr_GL_0.pth"), "--save_path", str(out) + "/"])
    assert feats.shape == (24, 14 * 512) and np.isfinite(feats).all()
    assert "view recipe: %s | jitter_sigma 0.02" % kinds in capsys.readouterr().out
    for n in names:
        assert np.load(str(out / (n + ".npy"))).shape == (14 * 512,)
    # a resumed run must repeat the recipe
    with pytest.raises(RuntimeError, match=r"--jitter_sigma 0\.01 \(the state: 0\.02\)"):
        train.main(_train_args(tmp_path / "d", tmp_path / "ck_r1", 13, 640, "--view_kinds", kinds, "--jitter_sigma", "0.01",
                               "--save_state_every", "1", "--resume", "auto", "--nepoch", "2"))
