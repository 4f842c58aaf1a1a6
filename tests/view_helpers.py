"""The harness of the GPU tests of the philox views (test_gpu_views_sizes.py, test_gpu_view_recipe.py): synthetic trees of
clips on disk, the clips every seam is tested on, and the C ABI's view entries called on a packed batch and on a resident pool."""
import os

import numpy as np
import torch

from helpers import synth_clip

DEV = "cuda:0"


def _write_clip(root, name, clip, branch="0"):
    from facl_amd.dataset import clip_paths
    for p, a in zip(clip_paths(str(root), name, branch), clip):
        os.makedirs(os.path.dirname(p), exist_ok=True)
        np.save(p, a)


def _names(n):
    return ["S%03dC%03dP%03dR001A%03d" % (1 + i % 4, (2, 3, 1)[i % 3], 1 + i, 1 + (i // 3) % 4) for i in range(n)]


def _tree(root, n=24, dt=np.float64, rows=None):
    """n clips: cameras 2 / 3 (cross-view train, 2 of every 3) and 1 (test); listed for training and for extraction.
    `rows`: (P, Kp, R1, R2) of every clip; default: every clip has its own row count in all four clouds."""
    names = _names(n)
    for i, nm in enumerate(names):
        r = rows or (600 + 7 * i, 300 + 3 * i, 400 + 5 * i, 150 + i)
        _write_clip(root, nm, synth_clip(200 + i, dt, *r))
        os.makedirs(os.path.join(str(root), "raw"), exist_ok=True)
        np.save(os.path.join(str(root), "raw", nm + ".npy"), np.zeros((1, 8)))
        os.makedirs(os.path.join(str(root), "reslution", "Resolution10", "raw"), exist_ok=True)
    return names


def _index(root):
    from facl_amd.dataset import ClipIndex
    index = ClipIndex.from_dir(os.path.join(str(root), "reslution", "Resolution60", "raw"), "ntu120")
    return index, index.select("view")


def _clips(dt):
    return [synth_clip(1, dt), synth_clip(2, dt, 777, 513, 400, 64), synth_clip(3, dt, 2048, 1024, 600, 300)]


def _signed(seed):
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return seed - (1 << 64) if seed >= 1 << 63 else seed


class _Packed:
    """A batch on the device in pack_clips' layout, its temporal rows compacted: what the disk entries take."""

    def __init__(self, clips, ids, check=True):
        from facl_amd import _lib
        from facl_amd.views import pack_clips
        if check:
            src, meta, dt = pack_clips(clips, ids)
        else:                                               # a clip pack_clips would refuse: the device's own checks
            src = np.concatenate([a[:, :8] for c in clips for a in c])
            sizes = np.array([[a.shape[0] for a in c] for c in clips])
            off = np.concatenate(([0], np.cumsum(sizes.reshape(-1))[:-1])).reshape(-1, 4)
            meta = np.concatenate((off, sizes, np.asarray(ids).reshape(-1, 1)), 1).astype(np.int32)
            dt = clips[0][0].dtype
        self.lib = _lib.load_library()
        self.f64 = dt == np.float64
        self.B, self.rows, self.meta_np = len(clips), src.shape[0], meta
        self.src, self.meta = torch.from_numpy(src).to(DEV), torch.from_numpy(meta).to(DEV)
        self.lists = torch.empty((2, self.rows), dtype=torch.int32, device=DEV)
        self.counts = torch.empty((self.B, 2), dtype=torch.int32, device=DEV)
        self.err = torch.zeros((1,), dtype=torch.int32, device=DEV)
        rt = self.lib.facl_views_temporal_rows_f64 if self.f64 else self.lib.facl_views_temporal_rows_f32
        _lib.check(rt(_lib.ptr(self.src), self.rows, 8, _lib.ptr(self.meta), self.B, _lib.ptr(self.lists),
                      _lib.ptr(self.counts), _lib.ptr(self.err), _lib.stream()), "facl_views_temporal_rows")

    def call(self, seed, epoch, G=None, P=None, out=None, idx=None):
        """The existing entry (G is None) or the _gp entry; returns (rc, out (G,B,P,4), idx (B,G,P)) as NumPy."""
        from facl_amd import _lib
        sfx = "f64" if self.f64 else "f32"
        g, p = (10, 512) if G is None else (G, P)
        if out is None:
            out = torch.full((max(g, 1) * self.B, max(p, 1), 4), float("nan"), dtype=torch.float32, device=DEV)
            idx = torch.full((self.B, max(g, 1), max(p, 1)), -7, dtype=torch.int32, device=DEV)
        head = (_lib.ptr(self.src), self.rows, 8, _lib.ptr(self.meta), _lib.ptr(self.lists), _lib.ptr(self.counts),
                _signed(seed), int(epoch), self.B)
        tail = (_lib.ptr(out), _lib.ptr(idx), _lib.stream())
        if G is None:
            rc = getattr(self.lib, "facl_build_views_philox_" + sfx)(*head, *tail)
        else:
            rc = getattr(self.lib, "facl_build_views_philox_gp_" + sfx)(*head, G, P, *tail)
        torch.cuda.synchronize()
        if rc != 0:
            return rc, out.cpu().numpy(), idx.cpu().numpy()
        return rc, out.cpu().numpy().reshape(g, self.B, p, 4), idx.cpu().numpy()


def _host(recipe, kinds=None, n_kinds=None, strengths=None):
    """The three host arguments of a recipe entry (overridable, for the refusals) and the arrays that back them."""
    k = recipe.codes() if kinds is None else np.asarray(kinds, dtype=np.int32)
    s = recipe.strengths() if strengths is None else np.asarray(strengths, dtype=np.float64)
    return (k, s), (k.ctypes.data if k.size or kinds is None else None, len(k) if n_kinds is None else n_kinds, s.ctypes.data)


def _call(pk, recipe, seed, epoch, G, P, out=None, idx=None, host=None):
    """facl_build_views_philox_recipe_* on a packed batch; (rc, out (G,B,P,4), idx (B,G,P)) as NumPy."""
    from facl_amd import _lib
    if out is None:
        out = torch.full((G * pk.B, P, 4), float("nan"), dtype=torch.float32, device=DEV)
        idx = torch.full((pk.B, G, P), -7, dtype=torch.int32, device=DEV)
    keep, extra = _host(recipe) if host is None else host
    rc = getattr(pk.lib, "facl_build_views_philox_recipe_" + ("f64" if pk.f64 else "f32"))(
        _lib.ptr(pk.src), pk.rows, 8, _lib.ptr(pk.meta), _lib.ptr(pk.lists), _lib.ptr(pk.counts), _signed(seed), int(epoch),
        pk.B, G, P, _lib.ptr(out), _lib.ptr(idx), *extra, _lib.stream())
    torch.cuda.synchronize()
    if rc != 0:
        return rc, out.cpu().numpy(), idx.cpu().numpy()
    return rc, out.cpu().numpy().reshape(G, pk.B, P, 4), idx.cpu().numpy()


class _Pool:
    """The same clips as a resident pool (build_table's layout), their temporal rows compacted."""

    def __init__(self, clips, ids):
        from facl_amd import _lib
        from facl_amd.resident import build_table
        self.lib = _lib.load_library()
        self.f64 = clips[0][0].dtype == np.float64
        rows = np.array([[a.shape[0] for a in c] for c in clips])
        self.table_np, total, total0 = build_table(rows, ids)
        self.n = len(clips)
        self.src = torch.from_numpy(np.concatenate([a[:, :8] for c in clips for a in c])).to(DEV)
        self.tab = torch.from_numpy(self.table_np).to(DEV)
        self.lists = torch.empty((2 * total0,), dtype=torch.int32, device=DEV)
        self.err = torch.tensor([0, 2 ** 31 - 1], dtype=torch.int32, device=DEV)
        fn = self.lib.facl_resident_temporal_rows_f64 if self.f64 else self.lib.facl_resident_temporal_rows_f32
        _lib.check(fn(_lib.ptr(self.src), _lib.ptr(self.tab), _lib.ptr(self.lists), 0, self.n, _lib.ptr(self.err),
                      _lib.stream()), "facl_resident_temporal_rows")

    def call(self, recipe, seed, epoch, G, P, sel=None, out=None, idx=None, host=None, entry="recipe"):
        from facl_amd import _lib
        sel = torch.arange(self.n, dtype=torch.int32, device=DEV) if sel is None else sel
        Bn = sel.shape[0]
        if out is None:
            out = torch.full((G * Bn, P, 4), float("nan"), dtype=torch.float32, device=DEV)
            idx = torch.full((Bn, G, P), -7, dtype=torch.int64, device=DEV)
        keep, extra = ((), ()) if entry == "gp" else (_host(recipe) if host is None else host)
        rc = getattr(self.lib, "facl_build_views_resident_%s_%s" % (entry, "f64" if self.f64 else "f32"))(
            _lib.ptr(self.src), _lib.ptr(self.tab), _lib.ptr(self.lists), self.n, _lib.ptr(sel), Bn, G, P, _signed(seed),
            int(epoch), _lib.ptr(out), _lib.ptr(idx), _lib.ptr(self.err), *extra, _lib.stream())
        torch.cuda.synchronize()
        if rc != 0:
            return rc, out.cpu().numpy(), idx.cpu().numpy()
        return rc, out.cpu().numpy().reshape(G, Bn, P, 4), idx.cpu().numpy()


def _train_args(root, ck, G, P, *extra):
    return ["--synthetic", "0", "--data_root", str(root), "--dataset", "ntu120", "--view_rng", "philox", "--batchSize", "4",
            "--nepoch", "1", "--num_crop", str(G), "--SAMPLE_NUM", str(P), "--INPUT_FEATURE_NUM", "4",
            "--save_root_dir", str(ck)] + list(extra)
