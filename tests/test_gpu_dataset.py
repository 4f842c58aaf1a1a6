"""The dataset on disk through the GPU: --view_rng numpy views from files equal the reference's __getitem__ (fixture
tests/golden/dataset.npz), the counter-based philox views (csrc/views_philox.hip) equal their NumPy restatement
(facl_amd/philox.py) fed through the NumPy-mode kernel, and the training / extraction / probe entries run on a small tree."""
import functools
import os

import numpy as np
import pytest
import torch

from helpers import load_golden
from ranks import rank_env, run_ranks
from synth_tree import train_argv, tree_clip, write_clip, write_tree

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ULP1 = np.spacing(np.float32(1.0))


def _clip(seed, P=900, Kp=300, R1=500, R2=200, dt=np.float64):
    return tree_clip(seed, P, Kp, R1, R2, dt)                # this module's default sizes


@pytest.mark.parametrize("prefetch", [False, True])
def test_numpy_views_from_disk_equal_the_reference(tmp_path, prefetch):
    from facl_amd.dataset import ClipIndex, DiskBatches
    g = load_golden("dataset.npz")
    names = [str(n) for n in g["item_names"]]
    for i, n in enumerate(names):
        write_clip(tmp_path, n, [g[f"item{i}/cloud{k}"] for k in range(4)])
    index = ClipIndex.from_dir(str(tmp_path / "reslution" / "Resolution60" / "raw"), "ntu120")
    vids = np.array(index.select("view"))
    for s in (3, 11):
        rng = np.random.RandomState(s)
        for bs in ((vids[:2], vids[2:]),):                 # two batches, one generator, sampler order
            got = [(v.cpu().numpy(), nm) for v, nm, _ in DiskBatches(index, str(tmp_path), "0", list(bs), "numpy", DEV,
                                                                     rng=rng, prefetch=prefetch)]
        i = 0
        for out, nm in got:
            B = len(nm)
            want = np.stack([g[f"seed{s}/item{i + b}"] for b in range(B)], 0).transpose(1, 0, 2, 3).reshape(10 * B, 512, 4)
            for v in range(10):
                a, w = out[v * B:(v + 1) * B], want[v * B:(v + 1) * B]
                if v in (4, 5):                              # rotated views: one float32 ulp (tests/test_views.py)
                    np.testing.assert_allclose(a, w, rtol=0, atol=ULP1)
                    assert (a == w).mean() > 0.999
                else:
                    np.testing.assert_array_equal(a, w)
            i += B
        assert rng.rand() == float(g[f"seed{s}/next_rand"])


def _restated(clips, seed, epoch, ids):
    """The philox draws of facl_amd/philox.py fed through the NumPy-mode kernel: the restatement of the philox views."""
    from facl_amd import _lib
    from facl_amd.philox import draws
    from facl_amd.views import pack_clips
    src, meta, dt = pack_clips(clips, ids)
    d = [draws(seed, epoch, ids[b], *c, base=meta[b, :4]) for b, c in enumerate(clips)]
    idx, noise, cs = (torch.from_numpy(np.stack([x[k] for x in d])).to(DEV) for k in range(3))
    s = torch.from_numpy(src).to(DEV)
    out = torch.empty((10 * len(clips), 512, 4), dtype=torch.float32, device=DEV)
    lib = _lib.load_library()
    fn = lib.facl_build_views_f32 if dt == np.float32 else lib.facl_build_views_f64
    _lib.check(fn(_lib.ptr(s), s.shape[0], 8, _lib.ptr(idx), _lib.ptr(noise), _lib.ptr(cs), len(clips), _lib.ptr(out),
                  _lib.stream()), "facl_build_views")
    return out.cpu().numpy(), idx.cpu().numpy()


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_philox_views_equal_the_restatement(dt):
    from facl_amd.views import build_views_philox, pack_clips
    clips = [_clip(1, dt=dt), _clip(2, 777, 513, 400, 64, dt=dt), _clip(3, 2048, 1024, dt=dt)]
    ids = [5, 17, 4000]
    src, meta, _ = pack_clips(clips, ids)
    out, idx, err = build_views_philox(torch.from_numpy(src).to(DEV), torch.from_numpy(meta).to(DEV), np.dtype(dt), 99, 4,
                                       return_idx=True)
    want, want_idx = _restated(clips, 99, 4, ids)
    assert int(err.item()) == 0
    np.testing.assert_array_equal(idx.cpu().numpy(), want_idx)
    for b, c in enumerate(clips):
        rows = idx.cpu().numpy()[b] - meta[b, 0]
        assert (c[0][rows[6], 4] != 0).all() and (c[0][rows[7], 7] != 0).all()
    np.testing.assert_allclose(out.cpu().numpy(), want, rtol=0, atol=ULP1)


def test_philox_views_depend_on_seed_epoch_and_clip_id_only():
    from facl_amd.views import build_views
    clips = [_clip(10 + b, 600 + 50 * b) for b in range(5)]
    alone = build_views([clips[2]], philox=(7, 1, [42])).cpu().numpy()
    batch = build_views([clips[0], clips[1], clips[3], clips[2], clips[4]], philox=(7, 1, [0, 1, 3, 42, 4])).cpu().numpy()
    again = build_views([clips[2]], philox=(7, 1, [42])).cpu().numpy()
    other = build_views([clips[2]], philox=(7, 2, [42])).cpu().numpy()
    np.testing.assert_array_equal(batch.reshape(10, 5, 512, 4)[:, 3], alone.reshape(10, 512, 4))
    np.testing.assert_array_equal(again, alone)
    assert not np.array_equal(other, alone)


def test_philox_views_any_cloud_size_and_missing_temporal_rows():
    from facl_amd.views import build_views, build_views_philox
    for P in (1, 5000):
        c = _clip(3, P=P)
        out = build_views([c], philox=(1, 0, [0])).cpu().numpy()
        want, _ = _restated([c], 1, 0, [0])
        np.testing.assert_allclose(out, want, rtol=0, atol=ULP1)
    bad = list(_clip(4))
    bad[0] = bad[0].copy()
    bad[0][:, 7] = 0
    with pytest.raises(ValueError, match="channel 7"):
        build_views([_clip(5), tuple(bad)], philox=(1, 0, [0, 1]))
    # the device's own check: the compaction raises the error word, the temporal view is written as zeros (void)
    src = np.concatenate([a[:, :8] for a in bad])
    sizes = [a.shape[0] for a in bad]
    meta = np.array([[0, sizes[0], sum(sizes[:2]), sum(sizes[:3])] + sizes + [0]], dtype=np.int32)
    out, idx, err = build_views_philox(torch.from_numpy(src).to(DEV), torch.from_numpy(meta).to(DEV), np.dtype(np.float64),
                                       1, 0, return_idx=True)
    assert int(err.item()) == 1
    assert (out[7].cpu().numpy() == 0).all() and (idx[0, 7].cpu().numpy() == -1).all()


# ---- entries on a small tree -------------------------------------------------------------------------------------------------
_tree = functools.partial(write_tree, listed=("raw", "res10"))     # listed under the training, extraction and probe folders


def _train_args(root, ck, *extra):
    return train_argv(root, ck, *extra, after_batch=("--nepoch", "2"))


def test_disk_training_eager_and_graph(tmp_path):
    from facl_amd import cn3d_train_motion_GL as train
    _tree(tmp_path / "d")
    sds = []
    for gflag in ("1", "0"):
        net = train.main(_train_args(tmp_path / "d", tmp_path / ("ck" + gflag), "--graph", gflag))
        sds.append({k: v.detach().cpu().clone() for k, v in net.state_dict().items()})
        assert os.path.exists(os.path.join(str(tmp_path / ("ck" + gflag)), "corr_GL_0.pth"))
    for k, v in sds[0].items():
        assert torch.isfinite(v.float()).all(), k
        if v.is_floating_point():
            assert torch.allclose(v, sds[1][k], rtol=1e-5, atol=1e-7), k
        else:
            assert torch.equal(v, sds[1][k]), k
    assert int(sds[0]["net3DV_1.1.num_batches_tracked"]) == 2 * (16 // 4)          # 16 train clips, B = 4
    net = train.main(_train_args(tmp_path / "d", tmp_path / "ckp", "--view_rng", "philox", "--max_steps_per_epoch", "2",
                                 "--nepoch", "1"))
    assert int(net.state_dict()["net3DV_1.1.num_batches_tracked"]) == 2


def test_disk_extraction_and_probe(tmp_path):
    from facl_amd import cn3d_train_motion_GL as train, extract_motion_feature as ext, linear_classify as LC
    from facl_amd.cn3d_model_conbag import PointNet_Plus
    from facl_amd.dataset import ClipIndex, DiskBatches, ordered_batches
    from facl_amd.extract_common import extract_batch
    from facl_amd.train_common import build_parser
    names = _tree(tmp_path / "d")
    train.main(_train_args(tmp_path / "d", tmp_path / "ck", "--nepoch", "1", "--max_steps_per_epoch", "1", "--graph", "0"))
    ck = str(tmp_path / "ck" / "corr_GL_0.pth")
    out = tmp_path / "f"
    args = ["--synthetic", "0", "--data_root", str(tmp_path / "d"), "--dataset", "ntu120", "--batchSize", "5",
            "--checkpoint", ck, "--save_path", str(out) + "/"]
    feats = ext.main(args)
    assert sorted(os.listdir(out)) == sorted(n + ".npy" for n in names)          # 16 train + 8 test, ragged batches
    assert feats.shape == (24, 11 * 512)
    # each file equals extract_batch on the same views (same generator, same order)
    opt = build_parser('0').parse_known_args(args)[0]
    net = PointNet_Plus(opt, gost=10)
    net.load_state_dict(torch.load(ck, map_location="cpu", weights_only=True))
    net = net.to(DEV).eval()
    index = ClipIndex.from_dir(str(tmp_path / "d" / "raw"), "ntu120")
    rng = np.random.RandomState(2000)
    with torch.no_grad():
        for split in (index.select("view"), index.select("view", test=True)):
            vids = [np.asarray(split)[p] for p in ordered_batches(len(split), 5)]
            for views, nm, _ in DiskBatches(index, str(tmp_path / "d"), "0", vids, "numpy", DEV, rng=rng, prefetch=False):
                f = extract_batch(net, views.view(10, len(nm), 512, 4).permute(1, 0, 2, 3), opt).cpu().numpy()
                for b, n in enumerate(nm):
                    np.testing.assert_array_equal(np.load(str(out / (n + ".npy"))), f[b])
    # the probe on features separable by label
    md, ad = tmp_path / "m", tmp_path / "a"
    md.mkdir(), ad.mkdir()
    r = np.random.RandomState(0)
    protos = r.randn(120, 2, 11 * 512).astype(np.float32)
    for n in names:
        y = int(n[-3:]) - 1
        np.save(str(md / (n + ".npy")), protos[y, 0] + 0.1 * r.randn(11 * 512).astype(np.float32))
        np.save(str(ad / (n + ".npy")), protos[y, 1] + 0.1 * r.randn(11 * 512).astype(np.float32))
    os.makedirs(str(tmp_path / "d" / "reslution" / "Resolution60" / "raw"), exist_ok=True)
    top1 = LC.main(["--data_root", str(tmp_path / "d"), "--motion_feature_dir", str(md), "--appearance_feature_dir", str(ad),
                    "--batchSize", "4", "--nepoch", "20", "--learning_rate", "0.01"])
    assert top1 == 100.0


def _ddp_worker(rank, world, port, q, root, ck):
    rank_env(rank, world, port, FACL_DIST_BACKEND="gloo", LOCAL_RANK="0")
    import torch.distributed as dist
    from facl_amd import cn3d_train_motion_GL as train
    net = train.main(_train_args(root, ck + str(rank), "--nepoch", "1", "--graph", "0", "--view_rng", "philox"))
    q.put((rank, int(net.state_dict()["net3DV_1.1.num_batches_tracked"])))
    dist.barrier()
    dist.destroy_process_group()


def test_disk_training_two_ranks_run_equal_step_counts(tmp_path):
    _tree(tmp_path / "d", n=27)                               # 18 train clips: 2 steps of 4 per rank, 2 clips left over
    port = 29700 + (os.getpid() % 2000)
    res = run_ranks(_ddp_worker, 2, port, args=(str(tmp_path / "d"), str(tmp_path / "ck")), timeout=600)
    assert res == [(0, 2), (1, 2)]
