"""The 3DV point-cloud dataset on disk: clip index, splits, samplers, loading and the prefetching batch producer.

Restates the reference's dataset class (training_code/cn3D_data_set.py `NTU_RGBD_new`: `__init__` :36-92, `__getitem__`
:99-140, `get_pointdata` :803-818, `set_splits` :821-845) without pandas, and feeds its per-clip work to the GPU view
construction (facl_amd/views.py).  Paths are the reference's literal `../ntu/3DV_ntu60/...` with the prefix replaced by
`--data_root` (INTEGRATION.md lists the call sites).
"""
import os
import queue
import re
import threading
import zlib

import numpy as np
import torch

from . import views as V

TRAIN_IDS_60 = [1, 2, 4, 5, 8, 9, 13, 14, 15, 16, 17, 18, 19, 25, 27, 28, 31, 34, 35, 38]
TRAIN_IDS = [1, 2, 4, 5, 8, 9, 13, 14, 15, 16, 17, 18, 19, 25, 27, 28, 31, 34, 35, 38, 45, 46, 47, 49,
             50, 52, 53, 54, 55, 56, 57, 58, 59, 70, 74, 78, 80, 81, 82, 83, 84, 85, 86, 89, 91, 92, 93, 94, 95, 97, 98,
             100, 103]
TRAIN_VALID_IDS = ([1, 2, 5, 8, 9, 13, 14, 15, 16, 18, 19, 27, 28, 31, 34, 38], [4, 17, 25, 35])
TRAIN_SET = [2, 4, 6, 8, 10, 12, 14, 16, 18, 20, 22, 24, 26, 28, 30, 32]
TRAIN_CAMERAS = [2, 3]
NTU60_END = 'S017C003P020R002A060.npy'           # first clip of NTU-120 in sorted order: the ntu60 cut (:61)
NAME_RE = re.compile(r'.*S(\d{3})C(\d{3})P(\d{3})R(\d{3})A(\d{3}).*')
SPLIT_MODES = ('view', 'subject', 'set')

# folders the reference lists, relative to its literal prefix ../ntu/3DV_ntu60 (= --data_root)
TRAIN_LIST_DIR = {'0': 'reslution/Resolution60/raw', '1': 'reslution/Resolution10/raw'}   # cn3d_train_*_GL.py:161
EXTRACT_LIST_DIR = 'raw'                                                                    # extract_*_feature.py:112,127
PROBE_LIST_DIR = 'reslution/Resolution60/raw'                                               # linercls.py:40 default


class ClipIndex:
    """The sorted clip names of one folder and their (setup, camera, performer, replication, action) fields."""

    def __init__(self, names, dataset='ntu60'):
        names = sorted(names)
        self.train_ids = TRAIN_IDS
        if dataset == 'ntu60':
            if NTU60_END not in names:
                raise ValueError("--dataset ntu60 keeps the clips sorted before %s, which is not in the folder "
                                 "(cn3D_data_set.py:61)" % NTU60_END)
            names = names[:names.index(NTU60_END)]
            self.train_ids = TRAIN_IDS_60
        fields = []
        for n in names:
            m = NAME_RE.match(n)
            if m is None:
                raise ValueError("file name %r does not match S###C###P###R###A### (cn3D_data_set.py:33)" % n)
            fields.append([int(g) for g in m.groups()])
        self.names = names
        f = np.array(fields, dtype=np.int64).reshape(-1, 5)
        self.setup, self.camera, self.performer, self.replication, self.action = (f[:, i] for i in range(5))

    @classmethod
    def from_dir(cls, path, dataset='ntu60'):
        if not os.path.isdir(path):
            raise FileNotFoundError("dataset folder %s does not exist (see --data_root)" % path)
        return cls(os.listdir(path), dataset)

    def __len__(self):
        return len(self.names)

    def label(self, vid):
        return int(self.action[vid]) - 1

    def v_name(self, vid):
        return self.names[vid][:20]

    def splits(self):
        """set_splits (:821-845): the eight lists of clip indices, in index order."""
        def where(m):
            return [int(i) for i in np.flatnonzero(m)]
        perf, cam, setup = self.performer, self.camera, self.setup
        return {
            'train_subject': where(np.isin(perf, self.train_ids)),
            'train_subject_with_validation': where(np.isin(perf, TRAIN_VALID_IDS[0])),
            'validation_subject': where(np.isin(perf, TRAIN_VALID_IDS[1])),
            'test_subject': where(~np.isin(perf, self.train_ids)),
            'train_camera': where(np.isin(cam, TRAIN_CAMERAS)),
            'test_camera': where(~np.isin(cam, TRAIN_CAMERAS)),
            'train_set': where(np.isin(setup, TRAIN_SET)),
            'test_set': where(~np.isin(setup, TRAIN_SET)),
        }

    def select(self, mode='view', test=False, validation=False, full_train=True):
        """vid_ids of `__init__` (:71-92): mode view = DATA_CROSS_VIEW, subject = not DATA_CROSS_VIEW, set = DATA_CROSS_SET."""
        s = self.splits()
        if mode == 'set':
            return s['test_set'] if test else s['train_set']
        if mode == 'view':
            return s['test_camera'] if test else s['train_camera']
        if mode != 'subject':
            raise ValueError("split mode must be one of %s" % (SPLIT_MODES,))
        if test:
            return s['test_subject']
        if validation:
            return s['validation_subject']
        return s['train_subject'] if full_train else s['train_subject_with_validation']

    def crc(self):
        return zlib.crc32("\n".join(self.names).encode())


def clip_paths(data_root, v_name, branch):
    """The four files `__getitem__` loads (:105-116 motion, branch '0'; :122-132 appearance, '1')."""
    kind = 'raw' if branch == '0' else 'app'
    r = os.path.join(data_root, 'reslution')
    return (os.path.join(r, 'Resolution60', kind, v_name + '.npy'),
            os.path.join(r, 'Resolution60', 'others', v_name + '_key.npy'),
            os.path.join(r, 'Resolution30', kind, v_name + '.npy'),
            os.path.join(r, 'Resolution10', kind, v_name + '.npy'))


def load_clip(data_root, v_name, branch):
    arrs = tuple(np.load(p) for p in clip_paths(data_root, v_name, branch))
    if branch != '0' and arrs[0].ndim == 3:
        raise ValueError(
            "clip %s: %s is a 3-D (frames, points, channels) array. generate_NTU.py:249-266 writes the appearance clouds in "
            "that layout (as <name>_app.npy), but the reference's appearance branch (cn3D_data_set.py:122-138) indexes them "
            "as 2-D (rows, >=8) clouds and cannot consume them; no layout is invented here" % (v_name, clip_paths(data_root, v_name, branch)[0]))
    for a in arrs:
        if a.ndim != 2 or a.shape[1] < 8 or a.shape[0] < 1:
            raise ValueError("clip %s: every source cloud must be a (rows, >=8) array, got %s" % (v_name, a.shape))
        if a.dtype not in (np.float32, np.float64) or a.dtype != arrs[0].dtype:
            raise ValueError("clip %s: the four clouds must share one dtype, float32 or float64" % v_name)
    V.check_temporal_rows(arrs, v_name)
    V.check_finite_coordinates(arrs, v_name)
    return arrs


# ---- samplers -----------------------------------------------------------------------------------------------------------
def train_batches(n, B, world, rank, seed, epoch):
    """DataLoader(shuffle=True, drop_last=True) sharded over ranks: one seeded permutation of the split, the same on every
    rank; rank r takes the contiguous shard r of len // (B*W) batches.  Returns (steps, B) positions into the split."""
    perm = np.random.RandomState([seed & 0xFFFFFFFF, epoch]).permutation(n)
    steps = n // (B * world)
    return perm[rank * steps * B:(rank + 1) * steps * B].reshape(steps, B)


def ordered_batches(n, B):
    """DataLoader(shuffle=False, drop_last=False): in order, the last batch ragged."""
    return [np.arange(i, min(i + B, n)) for i in range(0, n, B)]


def check_same_index_on_all_ranks(index, device):
    """All ranks all-reduce (len(index), crc of the sorted names) and raise together on a mismatch, before the first step."""
    import torch.distributed as dist
    from . import dist as fdist
    if not fdist.is_distributed():
        return
    dev = device if dist.get_backend() == "nccl" else "cpu"
    v = [len(index), index.crc()]
    t = torch.tensor(v + [-x for x in v], dtype=torch.int64, device=dev)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    t = t.cpu().tolist()
    if t[0] != -t[2] or t[1] != -t[3]:
        raise RuntimeError("the ranks see different dataset folders (clip count / name checksum differ; this rank: %d clips, "
                           "crc %08x)" % (v[0], v[1]))


# ---- batch producer -------------------------------------------------------------------------------------------------------
class _Staged:
    """One batch on its way to the device: pinned host buffers, their device copies, the copy's event."""
    pass


class DiskBatches:
    """Batches of views from the clips on disk.  `vids`: list of (B_i,) arrays of dataset indices, in order.  mode 'numpy':
    the host draws each clip's random numbers from `rng` (np.random.RandomState) in sampler order, exactly as sequential
    loading would; 'philox': counter-based draws on the device keyed by (seed, epoch, dataset index).  With `prefetch` a
    producer thread loads and draws batch i+1 (np.load, host draws, packing into pinned staging, H2D on a side stream)
    while batch i is consumed; an event orders the copy before the views launch on the compute stream.  Iterating yields
    ((G*B, P, 4) float32 views, v_names, labels); G = `num_crop` views of P = `num_point` points: 10 x 512, the
    reference's loader, or with 'philox' any size of the kernels' domain (facl_amd/philox.py) and any view `recipe`
    (facl_amd.philox.Recipe; None = the reference's ten kinds at its strengths)."""

    def __init__(self, index, data_root, branch, vids, mode, device, rng=None, seed=0, epoch=0, prefetch=True,
                 num_crop=V.NUM_CROP, num_point=V.NUM_POINT, recipe=None):
        if mode not in ('numpy', 'philox'):
            raise ValueError("disk batches draw with --view_rng numpy or philox")
        if mode != 'philox' and recipe is not None and not recipe.is_default():
            raise ValueError("the reference's NumPy stream defines its ten views only; another view recipe needs "
                             "--view_rng philox")
        self.recipe = recipe
        if mode == 'philox':
            V.check_view_size(num_crop, num_point)
        elif (num_crop, num_point) != (V.NUM_CROP, V.NUM_POINT):
            raise ValueError("the reference's NumPy stream defines %d views of %d points only; other sizes need "
                             "--view_rng philox" % (V.NUM_CROP, V.NUM_POINT))
        self.num_crop, self.num_point = int(num_crop), int(num_point)
        self.index, self.root, self.branch, self.vids = index, data_root, branch, list(vids)
        self.mode, self.dev, self.rng, self.seed, self.epoch = mode, torch.device(device), rng, seed, epoch
        self.prefetch = prefetch
        self.hold_first = False        # True: the producer waits after batch 0 until batch 1 is asked for (a graph capture
        self.dtype = None              # of the step on batch 0 must not see another thread's allocations or copies)

    # host half: load, check, draw, pack into pinned memory, copy on `stream`
    def _produce(self, vids, stream):
        clips = [load_clip(self.root, self.index.v_name(int(v)), self.branch) for v in vids]
        dt = clips[0][0].dtype
        if self.dtype is None:
            self.dtype = dt
        for c, v in zip(clips, vids):
            if c[0].dtype != self.dtype:
                raise ValueError("the dataset mixes float32 and float64 clips (clip %s is %s, earlier clips %s): the views "
                                 "kernel rounds the jitter in the source dtype, so one dtype is required"
                                 % (self.index.v_name(int(v)), c[0].dtype, self.dtype))
        s = _Staged()
        rows = sum(a.shape[0] for c in clips for a in c)
        pin = torch.empty((rows, 8), dtype=torch.float64 if dt == np.float64 else torch.float32).pin_memory()
        src, meta, _ = V.pack_clips(clips, [int(v) for v in vids], out=pin.numpy())
        host = {'src': pin}
        if self.mode == 'numpy':
            draws = [V.draw_clip(self.rng, c[0], c[1], c[2], c[3], meta[b, :4]) for b, c in enumerate(clips)]
            host['idx'] = torch.from_numpy(np.stack([d[0] for d in draws])).pin_memory()
            host['noise'] = torch.from_numpy(np.stack([d[1] for d in draws])).pin_memory()
            host['cs'] = torch.from_numpy(np.stack([d[2] for d in draws])).pin_memory()
        else:
            host['meta'] = torch.from_numpy(meta).pin_memory()
        s.names = [self.index.v_name(int(v)) for v in vids]
        s.labels = [self.index.label(int(v)) for v in vids]
        s.dt = dt
        with torch.cuda.stream(stream):
            s.dev = {k: t.to(self.dev, non_blocking=True) for k, t in host.items()}
            s.event = torch.cuda.Event()
            s.event.record(stream)
        s.host = host                                     # kept alive until the copy has completed
        return s

    # device half: on the compute stream, after the copy
    def _views(self, s):
        cur = torch.cuda.current_stream(self.dev)
        cur.wait_event(s.event)
        for t in s.dev.values():
            t.record_stream(cur)
        d = s.dev
        B = len(s.names)
        if self.mode == 'philox':
            return V.build_views_philox(d['src'], d['meta'], s.dt, self.seed, self.epoch, num_crop=self.num_crop,
                                        num_point=self.num_point, recipe=self.recipe)
        from . import _lib
        out = _lib.empty((V.NUM_CROP * B, V.NUM_POINT, 4), dtype=torch.float32, device=self.dev)
        _lib.call("facl_build_views_f32" if s.dt == np.float32 else "facl_build_views_f64", d['src'], d['src'].shape[0], 8, d['idx'],
                  d['noise'], d['cs'], B, out)
        return out

    def __iter__(self):
        with torch.cuda.device(self.dev):
            if not self.prefetch:
                for vids in self.vids:
                    s = self._produce(vids, torch.cuda.current_stream())
                    yield self._views(s), s.names, s.labels
                return
            yield from self._prefetched()

    def _prefetched(self):
        q = queue.Queue(maxsize=1)
        stop = threading.Event()
        side = torch.cuda.Stream(device=self.dev)

        resume = threading.Event()

        def producer():
            try:
                with torch.cuda.device(self.dev):
                    for i, vids in enumerate(self.vids):
                        s = self._produce(vids, side)
                        while not stop.is_set():
                            try:
                                q.put(s, timeout=0.1)
                                break
                            except queue.Full:
                                pass
                        if i == 0 and self.hold_first:
                            side.synchronize()
                            while not stop.is_set() and not resume.wait(0.1):
                                pass
                        if stop.is_set():
                            return
                q.put(None)
            except BaseException as e:                    # handed to the consumer, raised there
                q.put(e)

        th = threading.Thread(target=producer, name="facl-disk-prefetch", daemon=True)
        th.start()
        try:
            while True:
                s = q.get()
                if s is None:
                    break
                if isinstance(s, BaseException):
                    raise s
                yield self._views(s), s.names, s.labels
                resume.set()
        finally:
            stop.set()
            while th.is_alive():
                try:
                    q.get_nowait()
                except queue.Empty:
                    pass
                th.join(timeout=0.05)
            side.synchronize()
