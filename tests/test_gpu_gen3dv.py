"""3DV generation on the GPU (facl_amd/gen3dv.py, csrc/gen3dv.hip) against the reference's own results
(tests/golden/gen3dv.npz) and the NumPy restatement (tests/ref3dv.py).  Every comparison is equality."""
import os
import random
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref3dv as T                                          # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NP_SEED, PY_SEED = 20, 21                                   # tools/make_3dv_goldens.py


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(HERE, "golden", "gen3dv.npz"))


@pytest.fixture(scope="module")
def clips(gold):
    out = {c: T.make_clip(c) for c in T.CASES}
    for c, f in out.items():
        assert T.clip_crc(f) == int(gold[c + "/crc"])
    return out


def names_of(gold):
    return {str(c): str(n) for c, n in zip(gold["cases"], gold["names"])}


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


def check_digest(gold, key, a):
    a = np.ascontiguousarray(a)
    head = gold[key + "/head"]
    got = a.reshape(-1, a.shape[-1])[:head.shape[0]]
    assert same(got, head), "%s: first differing of the leading rows\n%r\n%r" % (key, got[(got != head).any(axis=1)][:2],
                                                                               head[(got != head).any(axis=1)][:2])
    assert T.digest(a) == str(gold[key + "/sha"]), key


def check_intermediates(frames, st):
    """The device's stages of one clip against the restatement run on the same chosen frames."""
    ref = T.prepare(frames, st["chosen"])
    assert same(st["mn"], ref["mn"]) and same(st["mx"], ref["mx"]) and tuple(st["dims"]) == tuple(ref["dims"])
    assert st["frame_counts"].tolist() == [p.shape[1] for p in ref["points"]]
    raw, key = T.rank_pool(ref["points"], ref["motion_points"], ref["mn"], ref["dims"])
    assert st["vol"].dtype == np.int32 and np.array_equal(st["vol"], raw)
    assert np.array_equal(st["key"], key[0])
    assert np.array_equal(st["vol0_filtered"], ref["vol"][0])
    assert np.array_equal(st["key_filtered"], ref["key_filtered"])
    hits, uniq = T.lists_of(ref["vol"])
    khits, kuniq = T.lists_of(T.key_volume(ref["vol"], ref["key_filtered"]))
    assert st["counts"].tolist() == [len(hits), len(uniq), len(khits), len(kuniq)]
    for k, want in (("hits", hits), ("unique", uniq), ("key_hits", khits), ("key_unique", kuniq)):
        assert same(st[k], want), k
    return ref


@pytest.mark.parametrize("batched", [False, True])
def test_intermediates_match_the_restatement(gold, clips, batched):
    from facl_amd import gen3dv
    nm = names_of(gold)
    order = sorted(clips)
    groups = [order] if batched else [[c] for c in order]
    for g in groups:
        rs, py = np.random.RandomState(1), random.Random(2)
        res = gen3dv.generate_clips([clips[c] for c in g], [nm[c] for c in g], rng=rs, py_random=py, device=DEV,
                                    intermediates=True)
        for c, (_, st) in zip(g, res):
            ref = check_intermediates(clips[c], st)
            # the fixture's stage goldens were made with another frame choice for the long clip; the others are comparable
            if clips[c].shape[0] <= T.K:
                assert same(ref["vol"][0], gold[c + "/vol0_filtered"]) and same(ref["key_filtered"], gold[c + "/key_filtered"])
                assert same(st["mn"], gold[c + "/min"]) and same(st["mx"], gold[c + "/max"])


@pytest.mark.parametrize("batched", [False, True])
def test_numpy_mode_reproduces_the_reference_files(gold, clips, batched):
    """Seeded as tools/make_3dv_goldens.py seeded the reference's main(): every array of every clip and resolution."""
    from facl_amd import gen3dv
    nm = names_of(gold)
    order = [str(c) for c in gold["cases"]]
    rs, py = np.random.RandomState(NP_SEED), random.Random(PY_SEED)
    for res in range(3):
        if batched:
            outs = gen3dv.generate_clips([clips[c] for c in order], [nm[c] for c in order], rng=rs, py_random=py, device=DEV)
        else:
            outs = [gen3dv.generate_clips([clips[c]], [nm[c]], rng=rs, py_random=py, device=DEV)[0] for c in order]
        for c, arrays in zip(order, outs):
            for kind, a in zip(("raw", "key", "app"), arrays):
                assert a.dtype == np.float64
                check_digest(gold, "main/%d/%s/%s" % (res, c, kind), a)
    assert rs.randint(0, 2 ** 31 - 1) == int(gold["main/np_next"])
    assert py.random() == float(gold["main/py_next"])


def _row_index(rows, table):
    """index in `table` of every row of `rows` (bytes equal); asserts membership."""
    key = {r.tobytes(): i for i, r in enumerate(np.ascontiguousarray(table))}
    idx = [key.get(r.tobytes(), -1) for r in np.ascontiguousarray(rows)]
    assert min(idx) >= 0, "a row that is not in the list it was drawn from"
    return np.array(idx)


def test_philox_mode(gold, clips):
    from facl_amd import gen3dv
    nm = names_of(gold)
    order = sorted(clips)
    fr, names = [clips[c] for c in order], [nm[c] for c in order]
    res = gen3dv.generate_clips(fr, names, mode="philox", seed=77, resolution=1, device=DEV, intermediates=True)
    for c, ((raw, key, app), st) in zip(order, res):
        ref = check_intermediates(clips[c], st)
        rows, hits = T.voxel_rows(ref["vol"])
        krows, khits = T.voxel_rows(T.key_volume(ref["vol"], ref["key_filtered"]))
        n = st["norm"]
        consts = (n[0:3], n[3], n[4:9], n[9:14])
        # the constants are those of the sampled motion cloud: recover the sample through the rows' positions in the list
        idx = _row_index(raw, T.normalise(rows, consts))
        got = T.norm_constants(rows[idx])
        assert all(same(np.asarray(a), np.asarray(b)) for a, b in zip(got, consts))
        if hits < T.SAMPLE:
            assert same(raw[:hits], T.normalise(rows, consts))      # the list itself (a voxel repeats per channel), then draws
        _row_index(key, T.normalise(krows, consts))
        if khits < T.SAMPLE:
            assert same(key[:khits], T.normalise(krows, consts))
        assert app.shape == (len(st["app_choice"]), T.SAMPLE, 4)
        assert st["app_choice"] == sorted(st["app_choice"]) and 0 <= min(st["app_choice"]) and max(st["app_choice"]) < len(st["chosen"])
        for j, f in enumerate(st["app_choice"]):
            _row_index(app[j], T.normalise_app(T.app_rows(ref["points"][f], ref["vol"][0], ref["mn"]), consts))
    outs = [r[0] for r in res]
    again = gen3dv.generate_clips(fr, names, mode="philox", seed=77, resolution=1, device=DEV)
    singly = [gen3dv.generate_clips([f], [n], mode="philox", seed=77, resolution=1, device=DEV)[0] for f, n in zip(fr, names)]
    back = gen3dv.generate_clips(fr[::-1], names[::-1], mode="philox", seed=77, resolution=1, device=DEV)[::-1]
    other = gen3dv.generate_clips(fr, names, mode="philox", seed=78, resolution=1, device=DEV)
    for a, b, c, d, e in zip(outs, again, singly, back, other):
        for k in range(3):
            assert same(a[k], b[k]) and same(a[k], c[k]) and same(a[k], d[k])
        assert not np.array_equal(a[0], e[0])


def test_ragged_batch_leaves_guard_bands_untouched(gold, clips, monkeypatch):
    """Clips of different frame counts and grid sizes in one launch; every buffer the kernels write sits between guard
    bands.  Results equal the unguarded run."""
    from facl_amd import gen3dv, _lib
    nm = names_of(gold)
    order = sorted(clips)
    fr, names = [clips[c] for c in order], [nm[c] for c in order]
    want = gen3dv.generate_clips(fr, names, mode="philox", seed=5, device=DEV)
    GUARD, held = 4096, []

    def guarded(size, dtype=None, device=None):
        n = int(np.prod(size))
        buf = torch.full((n * dtype.itemsize + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=device)
        held.append((buf, n * dtype.itemsize))
        return buf[GUARD:GUARD + n * dtype.itemsize].view(dtype).view(*size)

    monkeypatch.setattr(_lib, "empty", guarded)
    got = gen3dv.generate_clips(fr, names, mode="philox", seed=5, device=DEV)
    assert len(held) >= 12
    for buf, n in held:
        assert bool((buf[:GUARD] == 0xA5).all()) and bool((buf[GUARD + n:] == 0xA5).all())
    for a, b in zip(want, got):
        for k in range(3):
            assert same(a[k], b[k])


def test_generate_train_extract(tmp_path):
    """Depth clips -> dataset on disk -> two steps of the motion training entry -> the extraction entry."""
    from facl_amd import cn3d_train_motion_GL as train, extract_motion_feature as ext, generate_3dv
    from facl_amd.dataset import NTU60_END
    depth = tmp_path / "depth"
    depth.mkdir()
    names = ["S001C002P001R001A001", "S001C003P002R001A002", "S002C002P003R001A003", "S002C003P004R001A004",
             "S003C001P005R001A001", "S003C001P006R001A002", NTU60_END[:-4]]
    for i, n in enumerate(names):
        spec = dict(n=10 + i, parts=[(126, 120 + 2 * i, 60, 44, 2500 + 20 * i, 0, 1, 0, 90), (100, 80 + 3 * i, 16, 14, 2250, 2, 3, 30, 0)])
        np.save(str(depth / (n + ".npy")), T.make_clip(spec))
    root = tmp_path / "d"
    assert generate_3dv.main(["--depth_root", str(depth), "--out_root", str(root), "--seed", "3", "--batch_clips", "3",
                              "--extract_raw", "1"]) == 3 * len(names)
    for res in (60, 30, 10):
        for sub, suffix, shape in (("raw", ".npy", (2048, 8)), ("others", "_key.npy", (2048, 8))):
            a = np.load(str(root / "reslution" / ("Resolution%d" % res) / sub / (names[0] + suffix)))
            assert a.shape == shape and a.dtype == np.float64 and np.isfinite(a).all()
        assert np.load(str(root / "reslution" / ("Resolution%d" % res) / "app" / (names[0] + "_app.npy"))).shape == (10, 2048, 4)
    assert sorted(os.listdir(str(root / "raw"))) == sorted(n + ".npy" for n in names)
    assert generate_3dv.main(["--depth_root", str(depth), "--out_root", str(root), "--seed", "3"]) == 0     # all present: skipped
    ck = tmp_path / "ck"
    net = train.main(["--synthetic", "0", "--data_root", str(root), "--dataset", "ntu60", "--batchSize", "2", "--nepoch", "1",
                      "--max_steps_per_epoch", "2", "--num_crop", "10", "--SAMPLE_NUM", "512", "--INPUT_FEATURE_NUM", "4",
                      "--save_root_dir", str(ck), "--graph", "0"])
    for k, v in net.state_dict().items():
        assert torch.isfinite(v.float()).all(), k
    assert int(net.state_dict()["net3DV_1.1.num_batches_tracked"]) == 2
    out = tmp_path / "f"
    feats = ext.main(["--synthetic", "0", "--data_root", str(root), "--dataset", "ntu60", "--batchSize", "4",
                      "--checkpoint", str(ck / "corr_GL_0.pth"), "--save_path", str(out) + "/"])
    assert sorted(os.listdir(str(out))) == sorted(n + ".npy" for n in names[:-1])       # the sentinel is the ntu60 cut
    assert np.isfinite(feats).all()
