"""Philox views at any view count G and cloud size P (csrc/views_philox.hip, csrc/views_resident.hip; the recipe is in
facl_amd/philox.py): the 10 x 512 block of every size is the existing entries' output bit for bit, every (round, chunk) block
equals the NumPy restatement fed through the NumPy-mode kernel, the resident path equals the disk path bit for bit, a clip's
views are local to (seed, epoch, clip id), void views and the domain behave as the header says, and the training,
extraction and probe entries run at 24 x 2048 and 13 x 640."""
import os
import re

import numpy as np
import pytest
import torch

from helpers import synth_clip
from view_helpers import _Packed, _clips, _index, _train_args, _tree

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 2000
ULP1 = np.spacing(np.float32(1.0))
FACL_E_SHAPE = -1
SIZES = [(10, 512), (24, 2048), (13, 640), (1, 64)]


# ---- 1. prefix, disk path ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_every_size_holds_the_existing_output_as_its_first_block(dt):
    pk = _Packed(_clips(dt), [5, 17, 4000])
    rc, old, old_idx = pk.call(99, 4)
    assert rc == 0 and int(pk.err.item()) == 0 and np.isfinite(old).all() and (old_idx >= 0).all()
    got = {}
    for G, P in SIZES:
        rc, out, idx = pk.call(99, 4, G, P)
        assert rc == 0 and out.shape == (G, 3, P, 4) and idx.shape == (3, G, P)
        assert np.isfinite(out).all() and (idx >= 0).all()                 # every element was written
        g, p = min(G, 10), min(P, 512)
        np.testing.assert_array_equal(out[:g, :, :p], old[:g, :, :p])
        np.testing.assert_array_equal(idx[:, :g, :p], old_idx[:, :g, :p])
        got[(G, P)] = (out, idx)
    np.testing.assert_array_equal(got[(10, 512)][0], old)
    # sub-prefixes beyond the first block: P = 64 against P = 2048 is covered above (both inside 512); views 10.. and
    # points 512.. of (13, 640) against (24, 2048); G = 1 against G = 24
    a, b = got[(13, 640)], got[(24, 2048)]
    np.testing.assert_array_equal(a[0], b[0][:13, :, :640])
    np.testing.assert_array_equal(a[1], b[1][:, :13, :640])
    np.testing.assert_array_equal(got[(1, 64)][0], b[0][:1, :, :64])
    np.testing.assert_array_equal(got[(1, 64)][1], b[1][:, :1, :64])
    rc, one, one_idx = pk.call(99, 4, 1, 2048)
    assert rc == 0
    np.testing.assert_array_equal(one, b[0][:1])
    np.testing.assert_array_equal(one_idx, b[1][:, :1])
    rc, few, few_idx = pk.call(99, 4, 24, 64)
    assert rc == 0
    np.testing.assert_array_equal(few, b[0][:, :, :64])
    np.testing.assert_array_equal(few_idx, b[1][:, :, :64])


# ---- 2. against the pinned NumPy-mode kernel, every round and chunk ------------------------------------------------------------
def _restated_block(pk, clips, seed, epoch, ids, G, P, r, first):
    """philox.draws of round r, points first.. fed through facl_build_views_* (pinned to the reference by views.npz)."""
    from facl_amd import _lib
    from facl_amd.philox import draws
    d = [draws(seed, epoch, ids[b], *c, base=pk.meta_np[b, :4], num_crop=G, num_point=P, round=r, first_point=first)
         for b, c in enumerate(clips)]
    idx, noise, cs = (torch.from_numpy(np.stack([x[k] for x in d])).to(DEV) for k in range(3))
    out = torch.empty((10 * len(clips), 512, 4), dtype=torch.float32, device=DEV)
    fn = pk.lib.facl_build_views_f64 if pk.f64 else pk.lib.facl_build_views_f32
    _lib.check(fn(_lib.ptr(pk.src), pk.rows, 8, _lib.ptr(idx), _lib.ptr(noise), _lib.ptr(cs), len(clips), _lib.ptr(out),
                  _lib.stream()), "facl_build_views")
    return out.cpu().numpy().reshape(10, len(clips), 512, 4), idx.cpu().numpy()


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("G,P", [(24, 2048), (13, 640)])
def test_every_round_and_chunk_equals_the_restatement(G, P, dt):
    clips, ids = _clips(dt), [5, 17, 4000]
    pk = _Packed(clips, ids)
    rc, out, idx = pk.call(99, 4, G, P)
    assert rc == 0 and int(pk.err.item()) == 0
    blocks = 0
    for r in range((G + 9) // 10):
        for c in range((P + 511) // 512):
            want, want_idx = _restated_block(pk, clips, 99, 4, ids, G, P, r, 512 * c)
            kn, pn = min(10, G - 10 * r), min(512, P - 512 * c)          # ragged last round / chunk: the valid part
            assert kn >= 1 and pn >= 1
            a = out[10 * r:10 * r + kn, :, 512 * c:512 * c + pn]
            w = want[:kn, :, :pn]
            np.testing.assert_array_equal(idx[:, 10 * r:10 * r + kn, 512 * c:512 * c + pn], want_idx[:, :kn, :pn])
            worst = float(np.abs(a.astype(np.float64) - w).max())
            print("G %d P %d %s round %d chunk %d: max |diff| %.3g" % (G, P, np.dtype(dt).name, r, c, worst))
            for k in range(kn):
                if k in (4, 5):                                        # rotated kinds: one float32 ulp
                    np.testing.assert_allclose(a[k], w[k], rtol=0, atol=ULP1)
                else:
                    np.testing.assert_array_equal(a[k], w[k])
            blocks += 1
    assert blocks == ((G + 9) // 10) * ((P + 511) // 512)
    # the temporal views of every round draw from the rows with a non-zero channel
    for b, cl in enumerate(clips):
        rows = idx[b] - pk.meta_np[b, 0]
        for v in range(G):
            if v % 10 in (6, 7):
                assert (cl[0][rows[v], 4 if v % 10 == 6 else 7] != 0).all()


# ---- 3. resident = disk --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("G,P", [(24, 2048), (13, 640)])
def test_resident_views_equal_the_disk_views_at_other_sizes(tmp_path, G, P, dt):
    from facl_amd.dataset import DiskBatches, load_clip
    from facl_amd.resident import ResidentBatches, ResidentClips, build_views_resident
    from facl_amd.views import build_views_philox, pack_clips
    _tree(tmp_path, dt=dt)
    index, split = _index(tmp_path)
    assert len(split) == 16
    res = ResidentClips(index, str(tmp_path), "0", split, DEV)
    s = np.asarray(split)
    vids = [s[[3, 7, 3, 3, 0]], s[::-1].copy(), s[[15]]]        # a clip repeated, the split reversed, a batch of one
    it = ResidentBatches(res, vids, seed=SEED, epoch=1, num_crop=G, num_point=P)
    got = [(v.cpu().numpy(), nm, lb) for v, nm, lb in it]
    it.close()
    want = [(v.cpu().numpy(), nm, lb) for v, nm, lb in
            DiskBatches(index, str(tmp_path), "0", vids, "philox", DEV, seed=SEED, epoch=1, prefetch=False, num_crop=G,
                        num_point=P)]
    assert len(got) == len(want) == 3
    for (a, an, al), (w, wn, wl), v in zip(got, want, vids):
        assert a.dtype == np.float32 and a.shape == w.shape == (G * len(v), P, 4)
        np.testing.assert_array_equal(a, w)
        assert an == wn and al == wl
    # idx_out: the pool rows are the packed batch's rows, clip by clip
    table = res.table.cpu().numpy()
    order = [5, 0, 15, 5]
    out, idx = build_views_resident(res, torch.tensor(order, dtype=torch.int32, device=DEV), 77, 2, return_idx=True,
                                    num_crop=G, num_point=P)
    out, idx = out.view(G, len(order), P, 4).cpu().numpy(), idx.cpu().numpy()
    assert idx.dtype == np.int64 and idx.shape == (len(order), G, P) and res.error_flags() == 0
    clips = [load_clip(str(tmp_path), index.v_name(split[p]), "0") for p in order]
    src, meta, sdt = pack_clips(clips, [split[p] for p in order])
    o1, i1, e1 = build_views_philox(torch.from_numpy(src).to(DEV), torch.from_numpy(meta).to(DEV), sdt, 77, 2,
                                    return_idx=True, num_crop=G, num_point=P)
    assert int(e1.item()) == 0
    np.testing.assert_array_equal(out, o1.view(G, len(order), P, 4).cpu().numpy())
    i1 = i1.cpu().numpy().astype(np.int64)
    for b, p in enumerate(order):
        np.testing.assert_array_equal(idx[b] - table[p, 0], i1[b] - meta[b, 0])


# ---- 4. locality ---------------------------------------------------------------------------------------------------------------
def test_a_clips_views_depend_on_seed_epoch_and_clip_id_only_at_24_by_2048():
    from facl_amd.views import build_views
    G, P = 24, 2048
    clips = [synth_clip(10 + b, np.float64, 600 + 50 * b) for b in range(5)]
    kw = dict(num_crop=G, num_point=P)
    alone = build_views([clips[2]], philox=(7, 1, [42]), **kw).cpu().numpy()
    batch = build_views([clips[0], clips[1], clips[3], clips[2], clips[4]], philox=(7, 1, [0, 1, 3, 42, 4]), **kw).cpu().numpy()
    again = build_views([clips[2]], philox=(7, 1, [42]), **kw).cpu().numpy()
    assert alone.shape == (G, P, 4) and batch.shape == (G * 5, P, 4)
    np.testing.assert_array_equal(batch.reshape(G, 5, P, 4)[:, 3], alone)
    np.testing.assert_array_equal(again, alone)
    for other in ((8, 1, [42]), (7, 2, [42]), (7, 1, [43])):                 # seed, epoch, clip id
        o = build_views([clips[2]], philox=other, **kw).cpu().numpy()
        for v in range(G):                                                    # every view of every round moves
            assert not np.array_equal(o[v], alone[v]), (other, v)


# ---- 5. void views -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G,P", [(24, 2048), (13, 640)])
def test_void_temporal_views_in_every_round(tmp_path, G, P):
    good = synth_clip(5, np.float64)
    bad = list(synth_clip(4, np.float64))
    bad[0] = bad[0].copy()
    bad[0][:, 7] = 0
    ok = _Packed([good, good], [0, 1])
    rc, want, want_idx = ok.call(1, 0, G, P)
    assert rc == 0 and int(ok.err.item()) == 0
    pk = _Packed([good, tuple(bad)], [0, 1], check=False)
    assert int(pk.err.item()) == 1                            # raised by the compaction
    rc, out, idx = pk.call(1, 0, G, P)
    assert rc == 0
    void = [v for v in range(G) if v % 10 == 7]
    rest = [v for v in range(G) if v % 10 != 7]
    assert len(void) == (G + 2) // 10
    assert (out[void, 1] == 0).all() and (idx[1][void] == -1).all()
    assert np.isfinite(out).all() and (idx[1][rest] >= 0).all() and (idx[0] >= 0).all()
    np.testing.assert_array_equal(out[:, 0], want[:, 0])                     # the other clip is untouched
    np.testing.assert_array_equal(idx[0], want_idx[0])
    # the other views of the clip: what it gives with channel 7 present (kind 7 apart, no view reads channel 7)
    fixed = list(bad)
    fixed[0] = bad[0].copy()
    fixed[0][:, 7] = 0.5
    rc, ref, ref_idx = _Packed([good, tuple(fixed)], [0, 1]).call(1, 0, G, P)
    np.testing.assert_array_equal(out[rest, 1], ref[rest, 1])
    np.testing.assert_array_equal(idx[1][rest], ref_idx[1][rest])
    # resident: the ingest raises the word and names the clip; built anyway (no host check is possible past the ingest),
    # the kind-7 views of every round are void
    from facl_amd import _lib
    from facl_amd.resident import REC, build_table
    clips = [good, tuple(bad)]
    rows = np.array([[a.shape[0] for a in c] for c in clips])
    table, total, total0 = build_table(rows, [0, 1])
    src = torch.from_numpy(np.concatenate([a[:, :8] for c in clips for a in c])).to(DEV)
    tab = torch.from_numpy(table).to(DEV)
    lists = torch.empty((2 * total0,), dtype=torch.int32, device=DEV)
    err = torch.tensor([0, 2 ** 31 - 1], dtype=torch.int32, device=DEV)
    lib = _lib.load_library()
    _lib.check(lib.facl_resident_temporal_rows_f64(_lib.ptr(src), _lib.ptr(tab), _lib.ptr(lists), 0, 2, _lib.ptr(err),
                                                   _lib.stream()), "facl_resident_temporal_rows")
    assert err.cpu().tolist() == [1, 1] and tab.shape[1] == REC
    sel = torch.tensor([0, 1], dtype=torch.int32, device=DEV)
    rout = torch.full((G * 2, P, 4), float("nan"), dtype=torch.float32, device=DEV)
    ridx = torch.full((2, G, P), -7, dtype=torch.int64, device=DEV)
    _lib.check(lib.facl_build_views_resident_gp_f64(_lib.ptr(src), _lib.ptr(tab), _lib.ptr(lists), 2, _lib.ptr(sel), 2, G, P,
                                                    1, 0, _lib.ptr(rout), _lib.ptr(ridx), _lib.ptr(err), _lib.stream()),
               "facl_build_views_resident_gp")
    torch.cuda.synchronize()
    np.testing.assert_array_equal(rout.cpu().numpy().reshape(G, 2, P, 4), out)
    ridx = ridx.cpu().numpy()
    assert (ridx[1][void] == -1).all() and (ridx[1][rest] >= 0).all()
    np.testing.assert_array_equal(ridx[0], idx[0].astype(np.int64))


# ---- 6. domain -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_sizes_outside_the_domain_are_refused_without_a_launch(dt):
    from facl_amd import _lib
    from facl_amd.resident import build_table
    clips = [synth_clip(1, dt), synth_clip(2, dt, 700, 300, 400, 100)]
    pk = _Packed(clips, [3, 4])
    bad = [(0, 512), (65, 512), (10, 0), (10, 32), (10, 96), (10, 4160), (0, 0), (65, 4160), (-1, 512), (10, -64)]
    # resident pool of the same clips
    rows = np.array([[a.shape[0] for a in c] for c in clips])
    table, total, total0 = build_table(rows, [3, 4])
    src = torch.from_numpy(np.concatenate([a[:, :8] for c in clips for a in c])).to(DEV)
    tab = torch.from_numpy(table).to(DEV)
    lists = torch.empty((2 * total0,), dtype=torch.int32, device=DEV)
    err = torch.tensor([0, 2 ** 31 - 1], dtype=torch.int32, device=DEV)
    sfx = "f64" if dt == np.float64 else "f32"
    _lib.check(getattr(pk.lib, "facl_resident_temporal_rows_" + sfx)(_lib.ptr(src), _lib.ptr(tab), _lib.ptr(lists), 0, 2,
                                                                     _lib.ptr(err), _lib.stream()), "rows")
    sel = torch.tensor([1, 0], dtype=torch.int32, device=DEV)
    for G, P in bad:
        n = 65 * 2 * 4160 * 4                                                  # room for the largest refused size
        out = torch.full((n,), 12345.0, dtype=torch.float32, device=DEV)
        idx = torch.full((n // 4,), -7, dtype=torch.int32, device=DEV)
        rc, o, i = pk.call(5, 1, G, P, out=out, idx=idx)
        assert rc == FACL_E_SHAPE, (G, P)
        assert (o == 12345.0).all() and (i == -7).all(), (G, P)              # poisoned buffers stay as they were
        idx64 = torch.full((n // 4,), -7, dtype=torch.int64, device=DEV)
        rc = getattr(pk.lib, "facl_build_views_resident_gp_" + sfx)(
            _lib.ptr(src), _lib.ptr(tab), _lib.ptr(lists), 2, _lib.ptr(sel), 2, G, P, 5, 1, _lib.ptr(out), _lib.ptr(idx64),
            _lib.ptr(err), _lib.stream())
        torch.cuda.synchronize()
        assert rc == FACL_E_SHAPE, (G, P)
        assert (out == 12345.0).all() and (idx64 == -7).all() and err.cpu().tolist() == [0, 2 ** 31 - 1], (G, P)
    # the edges of the domain are accepted
    for G, P in ((1, 64), (64, 64), (1, 4096)):
        rc, o, i = pk.call(5, 1, G, P)
        assert rc == 0 and np.isfinite(o).all() and (i >= 0).all(), (G, P)
    # and the Python layers refuse before any launch
    from facl_amd.views import build_views
    for G, P in bad[:6]:
        with pytest.raises(ValueError, match="num_crop"):
            build_views(clips, philox=(1, 0, [0, 1]), num_crop=G, num_point=P)


# ---- 7. entries ----------------------------------------------------------------------------------------------------------------
def test_entries_train_extract_and_probe_at_24_by_2048(tmp_path, capsys):
    """Graph and eager, resident and from disk: four runs, one set of weights (torch.equal).  Every differing tensor is
    printed with its largest difference before the assertion.  No figure is recorded here yet: this test had not run on a
    GPU when it was written."""
    from facl_amd import cn3d_train_motion_GL as train, extract_motion_feature as ext, linear_classify as LC
    names = _tree(tmp_path / "d", rows=(2048, 512, 1024, 256))
    sds, losses = {}, {}
    for gflag in ("1", "0"):
        for r in ("1", "0"):
            ck = tmp_path / ("ck" + gflag + r)
            net = train.main(_train_args(tmp_path / "d", ck, 24, 2048, "--graph", gflag, "--resident", r))
            sds[(gflag, r)] = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
            assert os.path.exists(os.path.join(str(ck), "corr_GL_0.pth"))
            printed = capsys.readouterr().out
            assert ("resident: 16 clips" in printed) == (r == "1")
            losses[(gflag, r)] = [float(x) for x in re.findall(r"--loss: (\S+) \|", printed)]
    first = sds[("1", "1")]
    assert int(first["net3DV_1.1.num_batches_tracked"]) == 16 // 4               # 16 train clips, B = 4, one epoch
    for key, ls in losses.items():
        assert len(ls) == 1 and np.isfinite(ls[0]), (key, ls)
    for key, sd in sds.items():
        for k, v in sd.items():
            assert torch.isfinite(v.float()).all(), (key, k)
            if v.is_floating_point() and not torch.equal(v, first[k]):
                print("graph %s resident %s %s: max |diff| %.3g" % (key + (k, float((v - first[k]).abs().max()))))
    for key, sd in sds.items():
        for k, v in sd.items():
            assert torch.equal(v, first[k]), (key, k)
    # extraction on that checkpoint: (G + 1) * 512 per clip, and the probe takes them as they are
    out = tmp_path / "f"
    feats = ext.main(["--synthetic", "0", "--data_root", str(tmp_path / "d"), "--dataset", "ntu120", "--view_rng", "philox",
                      "--num_crop", "24", "--SAMPLE_NUM", "2048", "--batchSize", "5",
                      "--checkpoint", str(tmp_path / "ck11" / "corr_GL_0.pth"), "--save_path", str(out) + "/"])
    assert feats.shape == (24, 25 * 512) and np.isfinite(feats).all()
    assert sorted(os.listdir(out)) == sorted(n + ".npy" for n in names)
    for n in names:
        assert np.load(str(out / (n + ".npy"))).shape == (25 * 512,)
    index, _ = _index(tmp_path / "d")
    order = [v for t in (False, True) for v in index.select("view", test=t)]
    labels = torch.tensor([index.label(v) for v in order], dtype=torch.long, device=DEV)
    model, top1 = LC.fit(torch.from_numpy(feats).to(DEV), labels, num_class=120, nepoch=2, batch=8)
    assert np.isfinite(top1)
    assert sum(p.numel() for p in model.parameters()) == 120 * 25 * 512 + 120


def test_entry_runs_one_step_at_13_by_640(tmp_path, capsys):
    from facl_amd import cn3d_train_motion_GL as train
    _tree(tmp_path / "d", rows=(2048, 512, 1024, 256))
    net = train.main(_train_args(tmp_path / "d", tmp_path / "ck", 13, 640, "--max_steps_per_epoch", "1"))
    assert int(net.state_dict()["net3DV_1.1.num_batches_tracked"]) == 1
    loss = [float(x) for x in re.findall(r"--loss: (\S+) \|", capsys.readouterr().out)]
    assert len(loss) == 1 and np.isfinite(loss[0])
    for k, v in net.state_dict().items():
        assert torch.isfinite(v.float()).all(), k
