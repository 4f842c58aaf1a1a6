"""The view recipe of --view_rng philox, host side (facl_amd/philox.py: Recipe, counters, views; train_common's flags; the
state flags): parsing and refusals, the default table in literals, no counter word shared inside a clip's views, the NumPy
restatement against the oracle's get_data_train at the default recipe, the new kinds' arithmetic against the reference's own
transforms (tests/golden/view_kinds.npz, tools/make_view_kind_goldens.py), and the seven flags in the training state."""
import numpy as np
import pytest

from helpers import load_golden, synth_clip

ULP1 = np.spacing(np.float32(1.0))
FLAGS = ("view_kinds", "jitter_sigma", "jitter_clip", "rot_range", "scale_lo", "scale_hi", "tilt_angle")
BASE = ["--synthetic", "2", "--view_rng", "philox", "--INPUT_FEATURE_NUM", "4"]


def test_header_constants_match_the_python_binding():
    """The kind codes and the recipe's sizes (include/facl_hip.h) against facl_amd/_lib.py, and the three host-only arguments."""
    import os
    import re
    from facl_amd import _lib
    txt = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "facl_hip.h")).read()
    value = lambda name: int(re.search(r"#define\s+FACL_VIEW_%s\s+(\d+)" % name, txt).group(1))
    for code, name in enumerate(_lib.VIEW_KINDS):
        assert value(name.upper()) == code, name
    assert value("NKINDS") == len(_lib.VIEW_KINDS) == 13
    assert value("POS_MAX") == _lib.VIEW_POS_MAX == 12 and value("NSTRENGTH") == _lib.VIEW_NSTRENGTH == 6
    assert value("TABLE_COLS") == _lib.VIEW_TABLE_COLS == 8
    assert "HOST POINTERS, READ BEFORE THE LAUNCH" in txt
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for sfx in ("f32", "f64"):
        for stem, gp in (("facl_build_views_philox_recipe_", "facl_build_views_philox_gp_"),
                         ("facl_build_views_resident_recipe_", "facl_build_views_resident_gp_")):
            args = re.search(re.escape(stem + sfx) + r"\s*\(([^)]*)\)", code).group(1)
            assert re.search(r"const\s+int32_t\s*\*\s*kinds\s*,\s*int\s+n_kinds\s*,\s*const\s+double\s*\*\s*strengths", args)
            assert len(_lib.SIGNATURES[stem + sfx]) == len(_lib.SIGNATURES[gp + sfx]) + 3 == len(args.split(","))


def test_the_c_rule_refuses_without_a_device():
    """facl_view_recipe_table is host only: it runs here, and equals Recipe.table() for the default and the edges."""
    import ctypes
    from facl_amd import _lib
    from facl_amd.philox import Recipe
    lib = _lib.load_library()
    for kinds in ("reference", "rot", ",".join(["mirror"] * 12), "scale,tilt_neg,tilt_pos,jitter,rot,mirror,t7", "t4,raw,scale"):
        r = Recipe.parse(kinds)
        k = r.codes()
        t = np.full((len(k), 8), -9, dtype=np.int32)
        stride = ctypes.c_int32(-9)
        assert lib.facl_view_recipe_table(k.ctypes.data, len(k), t.ctypes.data, ctypes.addressof(stride)) == 0
        np.testing.assert_array_equal(t, r.table()[0])
        assert stride.value == r.table()[1]
    k = np.array([0, 13], dtype=np.int32)
    t = np.zeros((13, 8), dtype=np.int32)
    stride = ctypes.c_int32(0)
    assert lib.facl_view_recipe_table(k.ctypes.data, 2, t.ctypes.data, ctypes.addressof(stride)) == -1       # FACL_E_SHAPE
    assert lib.facl_view_recipe_table(k.ctypes.data, 0, t.ctypes.data, ctypes.addressof(stride)) == -1
    assert lib.facl_view_recipe_table(k.ctypes.data, 13, t.ctypes.data, ctypes.addressof(stride)) == -1
    assert lib.facl_view_recipe_table(None, 1, t.ctypes.data, ctypes.addressof(stride)) == -2                 # FACL_E_NULL
    assert lib.facl_view_recipe_table(k.ctypes.data, 1, None, ctypes.addressof(stride)) == -2


# ---- 1. parsing ----------------------------------------------------------------------------------------------------------------
def test_names_and_the_reference_alias_parse():
    from facl_amd import _lib
    from facl_amd.philox import DEFAULT_STRENGTHS, KIND_NAMES, REFERENCE_KINDS, Recipe
    assert KIND_NAMES == _lib.VIEW_KINDS and len(KIND_NAMES) == 13
    r = Recipe.parse("reference")
    assert r.kinds == REFERENCE_KINDS == ("raw", "mirror", "key", "key_mirror", "rot", "rot", "t4", "t7", "res30", "res10")
    assert r.is_default() and r == Recipe() and tuple(r.strengths()) == DEFAULT_STRENGTHS == (0.01, 0.05, 0.8, 0.5, 1.5, 0.25)
    assert Recipe.parse(",".join(REFERENCE_KINDS)).is_default()
    r = Recipe.parse("scale, tilt_neg,tilt_pos,jitter", jitter_sigma=0.02)
    assert r.kinds == ("scale", "tilt_neg", "tilt_pos", "jitter") and not r.is_default()
    assert list(r.codes()) == [10, 11, 12, 9] and r.codes().dtype == np.int32 and r.strengths()[0] == 0.02
    assert not Recipe(jitter_sigma=0.02).is_default() and "jitter_sigma 0.02" in Recipe(jitter_sigma=0.02).describe()
    for name in KIND_NAMES:
        assert Recipe.parse(name).kinds == (name,)
    assert len(Recipe.parse(",".join(["mirror"] * 12)).kinds) == 12


@pytest.mark.parametrize("kw,flag", [
    (dict(view_kinds=""), "view_kinds"), (dict(view_kinds=","), "view_kinds"), (dict(view_kinds=",".join(["raw"] * 13)), "view_kinds"),
    (dict(view_kinds="reference,raw,raw,raw"), "view_kinds"), (dict(view_kinds="raw,flip"), "view_kinds"),
    (dict(jitter_sigma=-0.01), "jitter_sigma"), (dict(jitter_sigma=float("nan")), "jitter_sigma"),
    (dict(jitter_clip=0.0), "jitter_clip"), (dict(jitter_clip=-1.0), "jitter_clip"), (dict(jitter_clip=float("inf")), "jitter_clip"),
    (dict(rot_range=-0.1), "rot_range"), (dict(rot_range=2.5), "rot_range"), (dict(rot_range=float("nan")), "rot_range"),
    (dict(scale_lo=0.0), "scale_lo"), (dict(scale_lo=-1.0), "scale_lo"), (dict(scale_lo=2.0), "scale_lo"),
    (dict(scale_hi=0.4), "scale_hi"), (dict(scale_hi=float("inf")), "scale_hi"), (dict(tilt_angle=float("nan")), "tilt_angle")])
def test_a_recipe_outside_its_domain_is_refused_with_the_flag_named(kw, flag):
    from facl_amd.philox import Recipe
    from facl_amd.train_common import build_parser, view_recipe
    kinds = kw.pop("view_kinds", "reference")
    with pytest.raises(ValueError, match="--" + flag):
        Recipe.parse(kinds, **kw)
    args = BASE + ["--view_kinds", kinds] + [a for k, v in kw.items() for a in ("--" + k, repr(v))]
    with pytest.raises(RuntimeError, match="--" + flag):
        view_recipe(build_parser('0').parse_args(args))


def test_the_edges_of_the_domain_are_accepted():
    from facl_amd.philox import Recipe
    Recipe(jitter_sigma=0.0, rot_range=0.0, scale_lo=1.0, scale_hi=1.0, tilt_angle=0.0)
    Recipe(rot_range=2.0, tilt_angle=-3.0, jitter_clip=1e-9)


def test_a_non_default_recipe_needs_the_counter_based_draws_on_clips(monkeypatch):
    from facl_amd import cn3d_train_motion_GL, extract_motion_feature
    from facl_amd.train_common import build_parser, check_view_flags, view_recipe
    p = build_parser('0')
    assert view_recipe(p.parse_args([])).is_default()                                      # --synthetic 1 --view_rng numpy
    assert view_recipe(p.parse_args(["--synthetic", "0", "--view_rng", "numpy", "--view_kinds", "reference"])).is_default()
    assert view_recipe(p.parse_args(BASE + ["--view_kinds", "raw,scale"])).kinds == ("raw", "scale")
    for extra, flag in ((["--view_kinds", "raw,mirror"], "view_kinds"), (["--jitter_sigma", "0.02"], "jitter_sigma"),
                        (["--jitter_clip", "0.1"], "jitter_clip"), (["--rot_range", "1"], "rot_range"),
                        (["--scale_lo", "0.8"], "scale_lo"), (["--scale_hi", "2"], "scale_hi"), (["--tilt_angle", "0.1"], "tilt_angle")):
        for stream in (["--synthetic", "0", "--view_rng", "numpy"], ["--synthetic", "2", "--view_rng", "device"],
                       ["--synthetic", "1", "--view_rng", "philox"], ["--synthetic", "1"]):
            opt = p.parse_args(stream + ["--INPUT_FEATURE_NUM", "4"] + extra)
            with pytest.raises(RuntimeError, match=r"--%s .*the reference's stream defines its ten views only" % flag):
                view_recipe(opt)
            with pytest.raises(RuntimeError, match="its ten views only"):
                check_view_flags(opt)
    # the entries refuse before the device is touched: torch.cuda is never asked
    import torch
    monkeypatch.setattr(torch.cuda, "set_device", lambda *a, **k: pytest.fail("the device was touched"))
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(RuntimeError, match="its ten views only"):
        cn3d_train_motion_GL.main(["--synthetic", "1", "--jitter_sigma", "0.02"])
    with pytest.raises(RuntimeError, match="its ten views only"):
        cn3d_train_motion_GL.main(["--synthetic", "0", "--view_rng", "numpy", "--INPUT_FEATURE_NUM", "4", "--view_kinds", "raw"])
    with pytest.raises(RuntimeError, match="its ten views only"):
        extract_motion_feature.main(["--synthetic", "1", "--view_kinds", "raw"])
    with pytest.raises(RuntimeError, match="--view_kinds: unknown kind 'flip'"):
        cn3d_train_motion_GL.main(BASE + ["--view_kinds", "flip"])
    # the host layers refuse too
    from facl_amd.philox import Recipe
    from facl_amd.views import build_views
    with pytest.raises(ValueError, match="its ten views only"):
        build_views([synth_clip(1, np.float32)], rng=np.random.RandomState(0), recipe=Recipe.parse("raw"))


# ---- 2. the default table ------------------------------------------------------------------------------------------------------
def test_the_default_table_is_the_layout_the_kernels_always_had():
    from facl_amd import philox as ph
    table, stride = ph.Recipe().table()
    assert stride == 32 == ph.ROUND_SLOTS and table.shape == (10, 8) and table.dtype == np.int32
    jitter = {1: (0, 1), 2: (2,), 3: (3, 4), 4: (5,), 5: (6,)}
    scalar = {4: 24, 5: 25}
    source = (0, 0, 1, 1, 0, 0, 4, 5, 2, 3)                   # points, key points, temporal rows of channel 4 / 7, res1, res2
    channel = (3, 3, 3, 3, 3, 3, 4, 7, 3, 3)
    for i in range(10):
        t = table[i]
        assert (t[ph.T_ROW_SLOT], t[ph.T_ROW_WORD]) == (i >> 2, i & 3)
        assert tuple(j for j in (t[ph.T_JIT0], t[ph.T_JIT1]) if j >= 0) == jitter.get(i, ())
        assert t[ph.T_SCALAR] == scalar.get(i, -1)
        assert (t[ph.T_SRC], t[ph.T_CH]) == (source[i], channel[i])
    assert ph.counters() == ph.counters(recipe=ph.Recipe())
    assert ph.counters(24, 128) == ph.counters(24, 128, recipe=ph.Recipe.parse("reference"))


# ---- 3. no shared counters -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kinds,J,A", [("reference", 7, 2), ("rot", 1, 1),
                                       ("scale,tilt_neg,tilt_pos,jitter,rot,mirror,t7", 7, 2),
                                       (",".join(["mirror"] * 12), 24, 0),
                                       (",".join(["mirror,key_mirror,rot,scale"] * 3), 18, 6)])
def test_no_counter_word_is_shared_inside_a_clips_views(kinds, J, A):
    from facl_amd.philox import Recipe, counters
    r = Recipe.parse(kinds)
    table, stride = r.table()
    assert stride == 32 * -(-(3 + 3 * max(7, J) + A) // 32)
    assert sum(int(j >= 0) for t in table for j in (t[5], t[6])) == J and int((table[:, 7] >= 0).sum()) == A
    users = counters(64, 64, recipe=r)                        # G = 64: every round a size can reach; the slots do not depend on P
    assert len({v for v, _ in users}) == 64
    seen = {}
    for user, words in users.items():
        for w in words:
            assert w not in seen, "counter word %r is read by %r and %r" % (w, seen[w], user)
            seen[w] = user
    assert max(s for _, s, _ in seen) < stride * -(-64 // len(table))


def test_the_stride_of_twelve_mirrors_is_96():
    from facl_amd.philox import Recipe
    assert Recipe.parse(",".join(["mirror"] * 12)).table()[1] == 96
    assert Recipe.parse(",".join(["mirror,key_mirror,rot,scale"] * 3)).table()[1] == 64


# ---- 4. the restatement against the oracle at the default recipe ----------------------------------------------------------------
class _Replay:
    """A stand-in for np.random.RandomState that hands the oracle the philox draws in the reference's call order."""

    def __init__(self, rows, noise, us):
        self.rows, self.noise, self.us = list(rows), list(noise), list(us)

    def randint(self, lo, hi, size):
        r = self.rows.pop(0)
        assert lo == 0 and r.shape == (size,) and (r < hi).all()
        return r

    def randn(self, *shape):
        return self.noise.pop(0).reshape(shape)

    def rand(self):
        return self.us.pop(0)


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_the_restatement_equals_the_oracle_fed_the_same_draws(dt):
    from facl_amd import philox as ph
    from oracle import views as OV
    seed, epoch, cid = 99, 4, 17
    clip = synth_clip(2, dt, 777, 513, 400, 64)
    got, rows = ph.views(None, seed, epoch, cid, clip, 10, 512)
    assert got.dtype == np.float32 and got.shape == (10, 512, 4) and (rows >= 0).all()
    idx, noise, _ = ph.draws(seed, epoch, cid, *clip, base=(0, 0, 0, 0))
    np.testing.assert_array_equal(rows, idx)
    nz = [np.flatnonzero(clip[0][:, t] != 0) for t in (4, 7)]
    temporal = [np.searchsorted(nz[k], idx[6 + k]) for k in range(2)]         # positions in the list of non-zero rows
    us = []
    for k in range(2):
        w = ph._words(seed, 24 + k, cid, epoch, n=[0])[0]
        us.append(float(ph.uniform53(w[0:1], w[1:2])[0]))
    # the call order of __getitem__: two temporal draws, then get_data_train (cn3D_data_set.py:285-350)
    order = temporal + [idx[v].astype(np.int64) for v in (0, 1, 2, 3, 4, 5, 8, 9)]
    rng = _Replay(order, noise, us)
    want = OV.get_item(rng, *clip)
    assert not rng.rows and not rng.noise and not rng.us                       # every draw was consumed
    want = want.astype(np.float32)
    for v in range(10):
        worst = float(np.abs(got[v].astype(np.float64) - want[v]).max())
        print("%s view %d: max |diff| %.3g" % (np.dtype(dt).name, v, worst))
        if v in (4, 5):                                                      # np.dot's summation order: one float32 spacing
            np.testing.assert_allclose(got[v], want[v], rtol=0, atol=ULP1)
        else:
            np.testing.assert_array_equal(got[v], want[v])


# ---- 5. the new kinds against the reference's own transforms --------------------------------------------------------------------
@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_scale_tilt_and_jitter_reproduce_the_reference(dt):
    from facl_amd import philox as ph
    g, tag = load_golden("view_kinds.npz"), np.dtype(dt).name
    pts = g[tag + "/in"]
    assert pts.dtype == dt and pts.shape[0] == 1 and pts.shape[2] == 4
    x = pts[0, :, :3]
    np.testing.assert_array_equal(pts, synth_clip(6, dt)[0][:pts.shape[1], :4][None])
    for name in ("default", "strong"):
        sigma, clip = g["%s/jitter_%s_strengths" % (tag, name)]
        want = g["%s/jitter_%s_out" % (tag, name)][0]
        assert want.dtype == np.float64 and (np.abs(want - x) > 0).any()
        got = ph.jitter_op(x, g["%s/jitter_%s_noise" % (tag, name)][0], sigma, clip)
        assert got.dtype == dt
        np.testing.assert_array_equal(got, want.astype(dt))                  # the loader stores it back into the S array
    assert (float(sigma), float(clip)) == (0.02, 0.03)
    factors = []
    for seed in g["scale_seeds"]:
        f = float(g["%s/scale_%d_factor" % (tag, seed)])
        want = g["%s/scale_%d_out" % (tag, seed)][0]
        assert want.dtype == dt and 0.5 <= f < 1.5
        np.testing.assert_array_equal(ph.scale_op(x, f), want[:, :3].astype(np.float32))
        np.testing.assert_array_equal(want[:, 3], pts[0, :, 3])
        factors.append(f)
    assert len(set(factors)) == len(factors)
    c, s = ph.tilt_cos_sin(0.25)
    for name, sign in (("tilt_neg", -1.0), ("tilt_pos", 1.0)):
        want = g["%s/%s_out" % (tag, name)][0]
        assert want.dtype == np.float32
        got = ph.rotate_y_op(x, c, sign * s)
        print("%s %s: max |diff| %.3g" % (tag, name, float(np.abs(got.astype(np.float64) - want[:, :3]).max())))
        np.testing.assert_allclose(got, want[:, :3], rtol=0, atol=ULP1)
        np.testing.assert_array_equal(got[:, 1], want[:, 1])
        np.testing.assert_array_equal(want[:, 3], pts[0, :, 3].astype(np.float32))


def test_views_of_the_new_kinds_are_what_their_operations_give():
    """philox.views wires the operations to the table's slots: a scale view is scale_op of the jittered rows with the factor of
    its scalar slot, and so on, at non-default strengths in a second round."""
    from facl_amd import philox as ph
    r = ph.Recipe.parse("raw,scale,tilt_pos,jitter", jitter_sigma=0.02, jitter_clip=0.03, scale_lo=0.8, scale_hi=1.25, tilt_angle=0.1)
    table, stride = r.table()
    clip = synth_clip(3, np.float64)
    out, rows = ph.views(r, 5, 1, 9, clip, 8, 64)
    n = np.arange(64, dtype=np.uint64)
    for v in (5, 6, 7):
        t, s0 = table[v % 4], stride * (v // 4)
        z = np.stack([ph.normal(*(ph._words(5, s0 + 3 + 3 * int(t[5]) + d, 9, 1, n)[:, :2].T)) for d in range(3)], -1)
        x = ph.jitter_op(clip[0][rows[v], :3], z, 0.02, 0.03)
        if v == 5:
            w = ph._words(5, s0 + int(t[7]), 9, 1, n=[0])[0]
            f = 0.8 + (1.25 - 0.8) * float(ph.uniform53(w[0:1], w[1:2])[0])
            assert 0.8 <= f < 1.25
            x = ph.scale_op(x, f)
        elif v == 6:
            x = ph.rotate_y_op(x, *ph.tilt_cos_sin(0.1))
        np.testing.assert_array_equal(out[v, :, :3], x.astype(np.float32))
        np.testing.assert_array_equal(out[v, :, 3], clip[0][rows[v], 3].astype(np.float32))
    np.testing.assert_array_equal(out[4, :, :3], clip[0][rows[4], :3].astype(np.float32))


# ---- 6. state flags ------------------------------------------------------------------------------------------------------------
def test_the_seven_flags_are_trajectory_flags_with_the_parser_defaults():
    from facl_amd import train_state as ts
    from facl_amd.philox import DEFAULT_STRENGTHS
    from facl_amd.train_common import VIEW_RECIPE_DEFAULTS, VIEW_RECIPE_FLAGS, build_parser
    assert VIEW_RECIPE_FLAGS == FLAGS and VIEW_RECIPE_DEFAULTS[1:] == DEFAULT_STRENGTHS
    o = build_parser('0').parse_args([])
    for k, d in zip(FLAGS, VIEW_RECIPE_DEFAULTS):
        assert k in ts.TRAJECTORY_FLAGS and ts.LATER_FLAG_DEFAULTS[k] == d == getattr(o, k)
    assert ts.FORMAT == 1


def test_a_state_from_before_the_flags_resumes_as_the_default_recipe(tmp_path):
    import torch
    from facl_amd import train_state as ts
    from facl_amd.train_common import build_parser, view_recipe
    p = build_parser('0')
    base = ["--batchSize", "4"] + BASE
    opt = p.parse_args(base)
    old = {k: v for k, v in ts.flags_of(opt).items() if k not in FLAGS}
    path = ts.state_path(str(tmp_path), 1)
    ts.write_atomic(ts.assemble(1, 16, old, {}, {}, {"queue": None, "key_encoder": None, "swav": None}, ts.capture_rng()), path)
    assert not set(FLAGS) & set(torch.load(path, weights_only=True)["flags"])
    back = ts.load_state(path)
    assert back["format"] == 1 and back["flags"]["view_kinds"] == "reference"
    assert view_recipe(type("O", (), dict(back["flags"]))).is_default()
    ts.check_compatible(back["flags"], opt)
    with pytest.raises(RuntimeError, match=r"--jitter_sigma 0\.02 \(the state: 0\.01\)"):
        ts.check_compatible(back["flags"], p.parse_args(base + ["--jitter_sigma", "0.02"]))
    with pytest.raises(RuntimeError, match=r"--view_kinds 'raw,scale' \(the state: 'reference'\)"):
        ts.check_compatible(back["flags"], p.parse_args(base + ["--view_kinds", "raw,scale"]))
    # a state of today holds the seven and pins each of them
    saved = ts.flags_of(p.parse_args(base + ["--view_kinds", "raw,scale", "--jitter_sigma", "0.02"]))
    assert saved["view_kinds"] == "raw,scale" and saved["jitter_sigma"] == 0.02 and set(FLAGS) <= set(saved)
    ts.write_atomic(ts.assemble(0, 4, saved, {}, {}, {"queue": None, "key_encoder": None, "swav": None}, ts.capture_rng()), path)
    again = ts.load_state(path)["flags"]
    assert {k: again[k] for k in FLAGS} == {k: saved[k] for k in FLAGS}
    with pytest.raises(RuntimeError, match=r"--jitter_sigma 0\.01 \(the state: 0\.02\); --scale_hi 2\.0 \(the state: 1\.5\)"):
        ts.check_compatible(again, p.parse_args(base + ["--view_kinds", "raw,scale", "--scale_hi", "2"]))
