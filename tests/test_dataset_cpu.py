"""The 3DV dataset on disk (facl_amd/dataset.py) against tests/golden/dataset.npz -- the outputs of the reference's own
NTU_RGBD_new (training_code/cn3D_data_set.py) on generated names and clips (tools/make_dataset_goldens.py) -- and the
NumPy restatement of the philox draws (facl_amd/philox.py) against the published Philox4x32-10 known-answer vectors."""
import os

import numpy as np
import pytest

from helpers import load_golden

MODES = {"subject_train": dict(mode="subject"), "subject_trainval": dict(mode="subject", full_train=False),
         "subject_validation": dict(mode="subject", validation=True), "subject_test": dict(mode="subject", test=True),
         "view_train": dict(mode="view"), "view_test": dict(mode="view", test=True),
         "set_train": dict(mode="set"), "set_test": dict(mode="set", test=True)}


@pytest.fixture(scope="module")
def golden():
    return load_golden("dataset.npz")


@pytest.mark.parametrize("names", ["with", "without"])
@pytest.mark.parametrize("dataset", ["ntu60", "ntu120"])
def test_index_and_splits_equal_the_reference(golden, names, dataset, tmp_path):
    from facl_amd.dataset import ClipIndex
    lst = [str(n) for n in golden["names_" + names]]
    for n in lst[::-1]:                                      # listdir order is arbitrary: the index sorts
        (tmp_path / n).write_bytes(b"")
    if f"{names}/{dataset}/view_train/raises" in golden:
        with pytest.raises(ValueError, match="S017C003P020R002A060"):
            ClipIndex.from_dir(str(tmp_path), dataset)
        return
    index = ClipIndex.from_dir(str(tmp_path), dataset)
    for mode, kw in MODES.items():
        key = f"{names}/{dataset}/{mode}"
        vids = index.select(**kw)
        assert vids == golden[key + "/vid_ids"].tolist(), mode
        assert [index.label(v) for v in vids] == golden[key + "/labels"].tolist(), mode
        assert [index.v_name(v) for v in vids] == [str(s) for s in golden[key + "/v_names"]], mode


def test_names_that_do_not_match_raise():
    from facl_amd.dataset import ClipIndex
    with pytest.raises(ValueError, match="notes.txt"):
        ClipIndex(["S001C001P001R001A001.npy", "notes.txt"], "ntu120")


@pytest.mark.parametrize("n,B,W", [(100, 4, 1), (100, 4, 3), (37, 5, 2), (64, 8, 8)])
def test_train_shards_are_disjoint_and_equal(n, B, W):
    from facl_amd.dataset import train_batches
    shards = [train_batches(n, B, W, r, seed=1, epoch=3) for r in range(W)]
    steps = n // (B * W)
    assert all(s.shape == (steps, B) for s in shards)
    allpos = np.concatenate([s.ravel() for s in shards])
    assert len(set(allpos.tolist())) == allpos.size and set(allpos.tolist()) <= set(range(n))
    again = train_batches(n, B, W, 0, seed=1, epoch=3)
    assert np.array_equal(again, shards[0])                              # seeded: the same on every rank
    if steps:
        assert not np.array_equal(train_batches(n, B, W, 0, seed=1, epoch=4), shards[0])


def test_extraction_order_covers_the_split_once():
    from facl_amd.dataset import ordered_batches
    b = ordered_batches(23, 5)
    assert [len(x) for x in b] == [5, 5, 5, 5, 3]
    assert np.concatenate(b).tolist() == list(range(23))


def _write_items(golden, root, dtype=np.float64):
    from facl_amd.dataset import clip_paths
    for i, n in enumerate(golden["item_names"]):
        for k, p in enumerate(clip_paths(str(root), str(n), "0")):
            os.makedirs(os.path.dirname(p), exist_ok=True)
            np.save(p, golden[f"item{i}/cloud{k}"].astype(dtype))


def test_host_draws_from_disk_keep_the_stream_in_step(golden, tmp_path):
    """Loading the fixture's clips from a tree in the reference layout and drawing their views on the host consumes the
    generator exactly like the reference's three __getitem__ calls: the next rand() agrees."""
    from facl_amd.dataset import ClipIndex, load_clip
    from facl_amd.views import draw_clip
    _write_items(golden, tmp_path)
    index = ClipIndex.from_dir(str(tmp_path / "reslution" / "Resolution60" / "raw"), "ntu120")
    vids = index.select("view")
    assert [index.v_name(v) for v in vids] == [str(n) for n in golden["item_names"]]
    for s in (3, 11):
        rng = np.random.RandomState(s)
        for v in vids:
            c = load_clip(str(tmp_path), index.v_name(v), "0")
            assert c[0].dtype == np.float64
            draw_clip(rng, *c, base=[0, 0, 0, 0])
        assert rng.rand() == float(golden[f"seed{s}/next_rand"])
    assert [index.label(v) for v in vids] == [int(golden[f"item{i}/label"]) for i in range(3)]


def test_clips_without_temporal_rows_and_3d_appearance_files_are_refused(golden, tmp_path):
    from facl_amd.dataset import clip_paths, load_clip
    _write_items(golden, tmp_path)
    n = str(golden["item_names"][0])
    p = clip_paths(str(tmp_path), n, "0")[0]
    a = np.load(p)
    a[:, 7] = 0
    np.save(p, a)
    with pytest.raises(ValueError, match=n + ".*channel 7"):
        load_clip(str(tmp_path), n, "0")
    for k, q in enumerate(clip_paths(str(tmp_path), n, "1")):
        os.makedirs(os.path.dirname(q), exist_ok=True)
        np.save(q, np.zeros((3, 64, 4)) if k != 1 else np.load(clip_paths(str(tmp_path), n, "0")[1]))
    with pytest.raises(ValueError, match="generate_NTU.py:249-266"):
        load_clip(str(tmp_path), n, "1")


def test_philox_known_answers():
    """Random123's published Philox4x32-10 known-answer vectors."""
    from facl_amd.philox import philox4x32_10
    cases = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
             ((0xffffffff,) * 4, (0xffffffff, 0xffffffff), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
             ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
              (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in cases:
        assert philox4x32_10(np.array(ctr), key).tolist() == list(want)


def test_philox_draws_have_the_reference_distributions():
    from facl_amd.philox import draws
    r = np.random.RandomState(0)
    pts = r.rand(900, 8) - 0.5
    pts[::3, 4] = 0
    clip = (pts, r.rand(300, 8), r.rand(500, 8), r.rand(200, 8))
    idx, noise, cs = draws(7, 2, 41, *clip, base=[0, 900, 1200, 1700])
    assert idx.shape == (10, 512) and idx[:2].max() < 900 and 900 <= idx[2:4].min() and idx[2:4].max() < 1200
    assert (pts[idx[6], 4] != 0).all() and idx[9].min() >= 1700
    assert abs(noise.mean()) < 0.02 and abs(noise.std() - 1) < 0.02
    assert np.allclose(cs[:, 0] ** 2 + cs[:, 1] ** 2, 1) and (cs[:, 0] > np.cos(0.4 * np.pi) - 1e-12).all()
    idx2, noise2, _ = draws(7, 3, 41, *clip, base=[0, 900, 1200, 1700])
    assert not np.array_equal(idx, idx2) and not np.array_equal(noise, noise2)
