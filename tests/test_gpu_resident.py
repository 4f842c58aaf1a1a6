"""The training split resident in device memory (facl_amd/resident.py, csrc/views_resident.hip): its views are the disk
path's philox views bit for bit, selection is by index, the refusals do not fault the device, the ingest holds no second
copy of the data and does not depend on its chunking, and the training entry reaches the same weights with --resident 1."""
import functools
import os

import numpy as np
import pytest
import torch

from ranks import rank_env, run_ranks
from synth_tree import train_argv, tree_clip, write_clip, write_tree

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 2000


def _clip(seed, P=900, Kp=300, R1=500, R2=200, dt=np.float64):
    return tree_clip(seed, P, Kp, R1, R2, dt)                # this module's default sizes


# every clip has its own row count in all four clouds; `clips`: {i: clip} replaces clip i
_tree = functools.partial(write_tree, scale=1, listed=("res10",))


def _index(root):
    from facl_amd.dataset import ClipIndex
    index = ClipIndex.from_dir(os.path.join(str(root), "reslution", "Resolution60", "raw"), "ntu120")
    return index, index.select("view")


def _disk(index, root, vids, epoch):
    from facl_amd.dataset import DiskBatches
    return [(v.cpu().numpy(), nm, lb) for v, nm, lb in
            DiskBatches(index, str(root), "0", vids, "philox", DEV, seed=SEED, epoch=epoch, prefetch=False)]


def _resident(res, vids, epoch):
    from facl_amd.resident import ResidentBatches
    it = ResidentBatches(res, vids, seed=SEED, epoch=epoch)
    got = [(v.cpu().numpy(), nm, lb) for v, nm, lb in it]
    it.close()
    return got


def _same(got, want):
    assert len(got) == len(want) > 0
    for (a, an, al), (w, wn, wl) in zip(got, want):
        assert a.dtype == np.float32 and a.shape == w.shape
        np.testing.assert_array_equal(a, w)
        assert an == wn and al == wl


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_resident_views_equal_the_disk_views_bit_for_bit(tmp_path, dt):
    from facl_amd.dataset import train_batches
    from facl_amd.resident import ResidentClips
    _tree(tmp_path, dt=dt)
    index, split = _index(tmp_path)
    assert len(split) == 16
    res = ResidentClips(index, str(tmp_path), "0", split, DEV)
    assert res.dtype == np.dtype(dt) and res.n == 16
    for epoch in (0, 3):
        for B in (4, 5):                                   # 5 does not divide 16: one clip is left out, as on disk
            pos = train_batches(len(split), B, 1, 0, 1, epoch)
            vids = [np.asarray(split)[p] for p in pos]
            _same(_resident(res, vids, epoch), _disk(index, tmp_path, vids, epoch))
    s = np.asarray(split)
    vids = [s[[3, 7, 3, 3, 0]], s[::-1].copy(), s[[15]]]     # a clip repeated, the split reversed, a batch of one
    _same(_resident(res, vids, 1), _disk(index, tmp_path, vids, 1))


def test_resident_source_rows(tmp_path):
    from facl_amd.dataset import load_clip
    from facl_amd.resident import ResidentClips, build_views_resident
    from facl_amd.views import build_views_philox, pack_clips
    _tree(tmp_path)
    index, split = _index(tmp_path)
    res = ResidentClips(index, str(tmp_path), "0", split, DEV)
    table = res.table.cpu().numpy()
    order = [5, 0, 15, 9]
    sel = torch.tensor(order, dtype=torch.int32, device=DEV)
    out, idx = build_views_resident(res, sel, 77, 2, return_idx=True)
    idx = idx.cpu().numpy()
    assert idx.dtype == np.int64 and res.error_flags() == 0
    for b, p in enumerate(order):
        vid = split[p]
        clip = load_clip(str(tmp_path), index.v_name(vid), "0")
        rel = idx[b] - table[p, 0]                             # pool rows -> clip-relative rows
        assert (rel >= 0).all() and (rel < table[p, 4:8].sum()).all()
        assert (rel[6] < clip[0].shape[0]).all() and (rel[7] < clip[0].shape[0]).all()
        assert (clip[0][rel[6], 4] != 0).all() and (clip[0][rel[7], 7] != 0).all()
        src, meta, dt = pack_clips([clip], [vid])              # the same clip alone in a packed batch: rows are clip-relative
        o1, i1, e1 = build_views_philox(torch.from_numpy(src).to(DEV), torch.from_numpy(meta).to(DEV), dt, 77, 2,
                                        return_idx=True)
        assert int(e1.item()) == 0
        np.testing.assert_array_equal(rel, i1.cpu().numpy()[0].astype(np.int64))
        np.testing.assert_array_equal(out.view(10, len(order), 512, 4)[:, b].cpu().numpy(),
                                      o1.view(10, 512, 4).cpu().numpy())


def test_resident_cloud_sizes_at_the_edges(tmp_path):
    from facl_amd.resident import ResidentClips
    _tree(tmp_path, n=6, clips={0: _clip(3, P=1), 1: _clip(3, P=5000), 3: _clip(4, 2, 1, 1, 1)})
    index, split = _index(tmp_path)
    res = ResidentClips(index, str(tmp_path), "0", split, DEV)
    table = res.table.cpu().numpy()
    assert sorted(table[:, 4]) == [1, 2, 600 + 7 * 4, 5000]
    one = int(np.flatnonzero(table[:, 4] == 1)[0])
    assert table[one, 10] == 1 and table[one, 11] == 1
    vids = [np.asarray(split), np.asarray(split)[[1, 0]]]
    _same(_resident(res, vids, 0), _disk(index, tmp_path, vids, 0))


def test_resident_refusals_do_not_fault_the_device(tmp_path):
    from facl_amd.resident import ResidentClips, build_views_resident, ERR_BAD_SELECTION
    # a clip without a non-zero channel 7: the host's check names it, and so does the device's word on its own
    bad = list(_clip(4))
    bad[0] = bad[0].copy()
    bad[0][:, 7] = 0
    names = _tree(tmp_path / "a", n=6, clips={3: tuple(bad)})
    index, split = _index(tmp_path / "a")
    for host_check in (True, False):
        with pytest.raises(ValueError, match=names[3] + ".*channel 7"):
            ResidentClips(index, str(tmp_path / "a"), "0", split, DEV, host_check=host_check)
    bad[0][:, 7] = 0.5
    bad[0][:, 4] = 0
    write_clip(tmp_path / "a", names[3], tuple(bad))
    with pytest.raises(ValueError, match=names[3] + ".*channel 4"):
        ResidentClips(index, str(tmp_path / "a"), "0", split, DEV, host_check=False, chunk_clips=1)
    # a selection outside the table: the error word, zero views for that clip, its neighbours untouched
    _tree(tmp_path / "b", n=6)
    index, split = _index(tmp_path / "b")
    res = ResidentClips(index, str(tmp_path / "b"), "0", split, DEV)
    good = torch.tensor([2, 1, 0, 3], dtype=torch.int32, device=DEV)
    want = build_views_resident(res, good, 5, 1).view(10, 4, 512, 4).cpu().numpy()
    assert res.error_flags() == 0
    for wrong in (-1, res.n):
        res.err.zero_()
        sel = torch.tensor([2, wrong, 0, 3], dtype=torch.int32, device=DEV)
        out, idx = build_views_resident(res, sel, 5, 1, return_idx=True)
        torch.cuda.synchronize()
        out, idx = out.view(10, 4, 512, 4).cpu().numpy(), idx.cpu().numpy()
        assert res.error_flags() == ERR_BAD_SELECTION
        assert (out[:, 1] == 0).all() and (idx[1] == -1).all()
        np.testing.assert_array_equal(out[:, [0, 2, 3]], want[:, [0, 2, 3]])
        assert (idx[[0, 2, 3]] >= 0).all()
    res.err.zero_()
    # mixed dtypes: refused in the header pass; a bound below the need: refused before anything is allocated
    write_clip(tmp_path / "b", index.v_name(split[2]), _clip(9, dt=np.float32))
    before = torch.cuda.memory_allocated()
    with pytest.raises(ValueError, match="mixes float32 and float64"):
        ResidentClips(index, str(tmp_path / "b"), "0", split, DEV)
    assert torch.cuda.memory_allocated() == before
    write_clip(tmp_path / "b", index.v_name(split[2]), _clip(9))
    del res
    need = None
    from facl_amd.resident import header_pass, pool_bytes
    rows, dt = header_pass(index, str(tmp_path / "b"), "0", split)
    need = pool_bytes(rows, dt.itemsize)["total"]
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    with pytest.raises(RuntimeError, match=str(need)):
        ResidentClips(index, str(tmp_path / "b"), "0", split, DEV, max_gb=(need - 1) / 2 ** 30)
    assert torch.cuda.memory_allocated() == before and torch.cuda.max_memory_allocated() == before
    assert ResidentClips(index, str(tmp_path / "b"), "0", split, DEV, max_gb=(need + 1) / 2 ** 30).n == len(split)


def test_resident_ingest_holds_no_second_copy(tmp_path):
    from facl_amd.resident import ResidentClips, chunk_ranges
    _tree(tmp_path, scale=4)                                   # 16 resident clips of ~6,000 rows: a pool of ~6 MB
    index, split = _index(tmp_path)
    ResidentClips(index, str(tmp_path), "0", split[:2], DEV)    # the library, the streams and the allocator are warm
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    res = ResidentClips(index, str(tmp_path), "0", split, DEV, chunk_clips=3)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    pool = res.src.numel() * 8 + res.lists.numel() * 4 + res.table.numel() * 8
    assert pool == res.bytes["total"] > 4 << 20
    assert len(chunk_ranges(res.rows, 8, 3)) == 6
    print("ingest peak %d bytes, pool %d bytes" % (peak, pool))
    assert peak <= pool + (1 << 20)


def test_resident_chunking_is_invisible(tmp_path):
    from facl_amd.resident import ResidentClips
    _tree(tmp_path)
    index, split = _index(tmp_path)
    pools = []
    for chunk in (1, 5, len(split)):
        res = ResidentClips(index, str(tmp_path), "0", split, DEV, chunk_clips=chunk)
        # lists: only the first n4 / n7 entries of a clip's two slots are defined
        t = res.table.cpu().numpy()
        lists = res.lists.cpu().numpy()
        kept = np.concatenate([np.concatenate((lists[2 * L:2 * L + n4], lists[2 * L + P:2 * L + P + n7]))
                               for L, P, n4, n7 in t[:, [9, 4, 10, 11]]])
        pools.append((res.src.cpu().numpy(), t, kept))
    assert (pools[0][1][:, 10:12] > 0).all()
    for p in pools[1:]:
        for a, b in zip(pools[0], p):
            np.testing.assert_array_equal(a, b)


def _train_args(root, ck, *extra):
    return train_argv(root, ck, *extra, after_batch=("--nepoch", "2"))


@pytest.mark.parametrize("gflag", ["1", "0"])
def test_resident_training_reaches_the_disk_path_weights(tmp_path, capsys, gflag):
    from facl_amd import cn3d_train_motion_GL as train
    _tree(tmp_path / "d")
    sds = []
    for r in ("1", "0"):
        ck = tmp_path / ("ck" + r)
        net = train.main(_train_args(tmp_path / "d", ck, "--view_rng", "philox", "--graph", gflag, "--resident", r))
        sds.append({k: v.detach().cpu().clone() for k, v in net.state_dict().items()})
        assert os.path.exists(os.path.join(str(ck), "corr_GL_0.pth"))
        printed = capsys.readouterr().out
        assert ("resident: 16 clips" in printed) == (r == "1")
    assert int(sds[0]["net3DV_1.1.num_batches_tracked"]) == 2 * (16 // 4)            # 16 train clips, B = 4, two epochs
    for k, v in sds[0].items():
        assert torch.isfinite(v.float()).all(), k
        if v.is_floating_point():
            assert torch.allclose(v, sds[1][k], rtol=1e-5, atol=1e-7), k
        else:
            assert torch.equal(v, sds[1][k]), k


def test_resident_entry_refuses_numpy_draws_and_synthetic_input(tmp_path):
    from facl_amd import cn3d_train_motion_GL as train
    _tree(tmp_path / "d")
    with pytest.raises(RuntimeError, match="--view_rng philox.*on the host"):
        train.main(_train_args(tmp_path / "d", tmp_path / "ck", "--view_rng", "numpy", "--resident", "1"))
    with pytest.raises(RuntimeError, match="needs --synthetic 0"):
        train.main(["--synthetic", "1", "--view_rng", "philox", "--resident", "1", "--save_root_dir", str(tmp_path / "ck")])
    with pytest.raises(RuntimeError, match="--resident_max_gb"):
        train.main(_train_args(tmp_path / "d", tmp_path / "ck", "--view_rng", "philox", "--resident", "1",
                               "--resident_max_gb", "0.0001"))


def _ddp_worker(rank, world, port, q, root, ck):
    rank_env(rank, world, port, FACL_DIST_BACKEND="gloo", LOCAL_RANK="0")
    import torch.distributed as dist
    from facl_amd import cn3d_train_motion_GL as train
    net = train.main(_train_args(root, ck + str(rank), "--nepoch", "1", "--graph", "0", "--view_rng", "philox",
                                 "--resident", "1"))
    q.put((rank, int(net.state_dict()["net3DV_1.1.num_batches_tracked"])))
    dist.barrier()
    dist.destroy_process_group()


def test_resident_training_two_ranks_run_equal_step_counts(tmp_path):
    _tree(tmp_path / "d", n=27)                               # 18 train clips: 2 steps of 4 per rank, 2 clips left over
    port = 31700 + (os.getpid() % 2000)
    res = run_ranks(_ddp_worker, 2, port, args=(str(tmp_path / "d"), str(tmp_path / "ck")), timeout=600)
    assert res == [(0, 2), (1, 2)]
