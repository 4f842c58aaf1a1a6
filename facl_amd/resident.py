"""The training split resident in device memory (--resident 1): load every clip once, build the philox views by index.

The philox views of a clip depend on (seed, epoch, dataset index) and on nothing else, and a whole training split fits
in the HBM of one device, so the per-batch host work of `dataset.DiskBatches` (np.load of 4 B files, packing, pinning, the
copy) happens ONCE, at the ingest.  After it a training step needs from the host only B table positions: one (B,) int32
copy and one launch (csrc/views_resident.hip).  The views are `DiskBatches(..., 'philox', ...)`'s bit for bit: both
kernels run one shared implementation of the draws and the arithmetic (csrc/views_point.inc).

Pool layout (include/facl_hip.h): `src` (rows_total, 8), `table` (n_clips, 12) int64, `lists` (2 * point-cloud rows,)
int32, `err` (2,) int32.  The header pass and the table builder below are pure NumPy (tests/test_resident_cpu.py).
"""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import views as V
from .dataset import clip_paths

REC = 12                       # include/facl_hip.h: FACL_RESIDENT_REC, int64 words per table record
CHANNELS = 8                   # pool rows keep channels 0..7, as pack_clips does
MAX_WORKERS = 16               # loader threads of the ingest: a fixed cap, never the machine's CPU count
STAGING_BYTES = 128 << 20      # target size of each of the two pinned staging buffers (default chunking)
ERR_NO_TEMPORAL_ROWS, ERR_BAD_SELECTION = 1, 2
INT32_MAX = (1 << 31) - 1

# Device memory left to the training step when --resident_max_gb is 0 (automatic).  MEASURED on an MI355X
# (tools/time_resident_entry.py, profiles/resident_entry.json): a --synthetic 0 --view_rng philox run at B = 32, 10 views,
# 512 points, --graph 1 peaks at 1,195,342,848 bytes of torch.cuda.max_memory_allocated() (step, graph capture and batch
# buffers; the same in every round).  The reserve is twice that.
STEP_PEAK_BYTES = 1195342848
STEP_RESERVE_BYTES = 2 * STEP_PEAK_BYTES
STEP_PEAK_AT = (32, 10, 512)   # the (B, G, P) of that measurement


def step_reserve_bytes(B, G=V.NUM_CROP, P=V.NUM_POINT):
    """The reserve for a step of B clips x G views x P points: STEP_RESERVE_BYTES scaled by the step's points over the
    measured step's, never below it.  An upper estimate by construction -- most of the step's memory (the grouped rows and
    the encoder's activations) grows with B * G and not with P -- so the automatic budget errs towards refusing;
    --resident_max_gb overrides it."""
    b0, g0, p0 = STEP_PEAK_AT
    return max(STEP_RESERVE_BYTES, -(-STEP_RESERVE_BYTES * int(B) * int(G) * int(P) // (b0 * g0 * p0)))


# ---- header pass and table: pure NumPy ---------------------------------------------------------------------------------------
def _npy_header(path):
    """(shape, dtype) of a .npy file without reading its data."""
    a = np.load(path, mmap_mode='r')
    return tuple(a.shape), a.dtype


def check_clip_shapes(name, shapes, dtypes, branch, path0=''):
    """`dataset.load_clip`'s checks from the headers alone."""
    if branch != '0' and len(shapes[0]) == 3:
        raise ValueError(
            "clip %s: %s is a 3-D (frames, points, channels) array. generate_NTU.py:249-266 writes the appearance clouds in "
            "that layout (as <name>_app.npy), but the reference's appearance branch (cn3D_data_set.py:122-138) indexes them "
            "as 2-D (rows, >=8) clouds and cannot consume them; no layout is invented here" % (name, path0))
    for s in shapes:
        if len(s) != 2 or s[1] < CHANNELS or s[0] < 1:
            raise ValueError("clip %s: every source cloud must be a (rows, >=8) array, got %s" % (name, tuple(s)))
    for d in dtypes:
        if d not in (np.float32, np.float64) or d != dtypes[0]:
            raise ValueError("clip %s: the four clouds must share one dtype, float32 or float64" % name)


def header_pass(index, data_root, branch, vids, workers=MAX_WORKERS):
    """Shapes and dtype of every clip of `vids` from the files' headers (no data is read).  Returns (rows (n, 4) int64,
    dtype); raises what `load_clip` / `DiskBatches` would raise for a malformed clip or a split of mixed dtypes."""
    vids = [int(v) for v in vids]

    def one(v):
        name = index.v_name(v)
        paths = clip_paths(data_root, name, branch)
        hs = [_npy_header(p) for p in paths]
        shapes, dtypes = [h[0] for h in hs], [h[1] for h in hs]
        check_clip_shapes(name, shapes, dtypes, branch, paths[0])
        return [s[0] for s in shapes], dtypes[0]

    with ThreadPoolExecutor(max_workers=max(1, min(int(workers), MAX_WORKERS))) as ex:
        res = list(ex.map(one, vids))
    if not res:
        raise ValueError("the split has no clip to keep resident")
    dt = res[0][1]
    for v, (_, d) in zip(vids, res):
        if d != dt:
            raise ValueError("the dataset mixes float32 and float64 clips (clip %s is %s, earlier clips %s): the views "
                             "kernel rounds the jitter in the source dtype, so one dtype is required"
                             % (index.v_name(v), d, dt))
    return np.array([r[0] for r in res], dtype=np.int64).reshape(-1, 4), np.dtype(dt)


def build_table(rows, cids):
    """The (n, 12) int64 table of csrc/views_resident.hip from the clips' row counts `rows` (n, 4) and dataset indices
    `cids` (n,): 64-bit row offsets of the four clouds, their counts, the clip id, the clip's slot in `lists`, and the two
    temporal-row counts (zero: the ingest pass writes them).  Returns (table, rows_total, rows0_total)."""
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 4)
    cids = np.asarray(cids, dtype=np.int64).reshape(-1)
    if rows.shape[0] != cids.shape[0] or rows.shape[0] < 1:
        raise ValueError("one dataset index per clip, at least one clip")
    if (rows < 1).any():
        raise ValueError("every source cloud needs at least one row")
    if (rows.sum(axis=1) > INT32_MAX).any():
        raise ValueError("a clip's four clouds together exceed 2^31 - 1 rows (temporal rows are clip-relative int32)")
    if rows.shape[0] > INT32_MAX or (cids < 0).any() or (cids > 0xFFFFFFFF).any():
        raise ValueError("table positions are int32 and clip ids one 32-bit philox counter word")
    n = rows.shape[0]
    flat = rows.reshape(-1)
    off = np.concatenate(([0], np.cumsum(flat, dtype=np.int64)[:-1])).reshape(n, 4)
    table = np.zeros((n, REC), dtype=np.int64)
    table[:, 0:4] = off
    table[:, 4:8] = rows
    table[:, 8] = cids
    table[:, 9] = np.concatenate(([0], np.cumsum(rows[:, 0], dtype=np.int64)[:-1]))
    return table, int(flat.sum(dtype=np.int64)), int(rows[:, 0].sum(dtype=np.int64))


def pool_bytes(rows, itemsize):
    """Exact device bytes of the pool for clips of `rows` (n, 4): {'src', 'lists', 'table', 'total'}."""
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 4)
    b = {'src': int(rows.sum(dtype=np.int64)) * CHANNELS * int(itemsize),
         'lists': 2 * int(rows[:, 0].sum(dtype=np.int64)) * 4,
         'table': rows.shape[0] * REC * 8}
    b['total'] = b['src'] + b['lists'] + b['table']
    return b


def check_budget(need, free, max_gb=0.0, reserve=STEP_RESERVE_BYTES):
    """Refuse a pool that does not fit: with --resident_max_gb G > 0 the bound is G GiB, otherwise (automatic) the free
    device memory minus the reserve kept for the training step.  No fall-back to batches from disk."""
    gib = float(1 << 30)
    if max_gb and max_gb > 0:
        if need > max_gb * gib:
            raise RuntimeError("--resident 1: the split needs %d bytes (%.3f GiB) of device memory, more than "
                               "--resident_max_gb %g; it is not kept resident and nothing falls back to batches from disk: "
                               "raise the bound or train with --resident 0" % (need, need / gib, max_gb))
        return
    if need > free - reserve:
        raise RuntimeError("--resident 1: the split needs %d bytes (%.3f GiB) of device memory, but %d bytes (%.3f GiB) "
                           "are free and %d bytes (%.3f GiB) stay reserved for the training step (twice the measured peak of "
                           "a 32 x 10 x 512 step, scaled by this step's clips x views x points); nothing falls back to "
                           "batches from disk: train with --resident 0 or set --resident_max_gb"
                           % (need, need / gib, free, free / gib, reserve, reserve / gib))


def chunk_ranges(rows, itemsize, chunk_clips=None, staging_bytes=STAGING_BYTES):
    """Consecutive [first, last) table ranges of the ingest: `chunk_clips` clips each, or (None) as many as fit
    `staging_bytes` of staging, at least one."""
    tot = np.asarray(rows, dtype=np.int64).reshape(-1, 4).sum(axis=1)
    n, out, a = tot.shape[0], [], 0
    while a < n:
        if chunk_clips:
            b = min(n, a + int(chunk_clips))
        else:
            b, acc = a, 0
            while b < n and (b == a or (acc + tot[b]) * CHANNELS * itemsize <= staging_bytes):
                acc += tot[b]
                b += 1
        out.append((a, b))
        a = b
    return out


def no_temporal_rows_message(name, channel):
    """The message of `views.check_temporal_rows`."""
    return ("clip %s: no row of its point cloud has a non-zero channel %d, so its temporal view cannot be "
            "drawn (cn3D_data_set.py:654-663)" % (name, channel))


# ---- the pool ---------------------------------------------------------------------------------------------------------------
class ResidentClips:
    """The clips `vids` (dataset indices, e.g. the training split) resident on `device`.

    Header pass (shapes and dtypes, no data; `load_clip`'s checks; one dtype), the exact byte need and the budget check come
    BEFORE anything is allocated.  Then the pool is allocated once at its final size and filled chunk by chunk: at most 16
    loader threads pack a chunk's clips into one of two reused pinned staging buffers, a side stream copies it straight
    into the chunk's slice of the pool and runs the temporal-rows pass on it while the threads load the next chunk.
    `host_check`: also look for clips without temporal rows while the chunk is in hand (names the clip at once); the
    device's error word, read once after the last chunk, is the backstop either way."""

    def __init__(self, index, data_root, branch, vids, device, max_gb=0.0, chunk_clips=None, workers=MAX_WORKERS,
                 host_check=True, reserve=STEP_RESERVE_BYTES):
        import torch
        from . import _lib
        self.index, self.root, self.branch = index, data_root, branch
        self.vids = [int(v) for v in vids]
        self.dev = torch.device(device)
        workers = max(1, min(int(workers), MAX_WORKERS))
        rows, self.dtype = header_pass(index, data_root, branch, self.vids, workers)
        self.rows = rows
        self.bytes = pool_bytes(rows, self.dtype.itemsize)
        check_budget(self.bytes['total'], torch.cuda.mem_get_info(self.dev)[0], max_gb, reserve)
        table, self.rows_total, self.rows0_total = build_table(rows, self.vids)
        self._pos = {v: i for i, v in enumerate(self.vids)}
        self.n = len(self.vids)
        tdt = torch.float64 if self.dtype == np.float64 else torch.float32
        rt = "facl_resident_temporal_rows_f64" if self.dtype == np.float64 else "facl_resident_temporal_rows_f32"
        chunks = chunk_ranges(rows, self.dtype.itemsize, chunk_clips)
        first_row = table[:, 0]
        end_row = np.append(first_row[1:], self.rows_total)
        stage_rows = max(int(end_row[b - 1] - first_row[a]) for a, b in chunks)
        with torch.cuda.device(self.dev):
            self.src = torch.empty((self.rows_total, CHANNELS), dtype=tdt, device=self.dev)
            self.lists = torch.empty((2 * self.rows0_total,), dtype=torch.int32, device=self.dev)
            self.table = torch.from_numpy(table).to(self.dev)
            self.err = torch.tensor([0, INT32_MAX], dtype=torch.int32, device=self.dev)
            _lib.require_cuda(self.src, self.lists, self.table, self.err)
            stage = [torch.empty((stage_rows, CHANNELS), dtype=tdt).pin_memory() for _ in range(min(2, len(chunks)))]
            done = [None] * len(stage)
            side = torch.cuda.Stream(device=self.dev)
            side.wait_stream(torch.cuda.current_stream())             # the table and the error word are in place

            def load_into(host, r0, i):
                name = index.v_name(self.vids[i])
                arrs = [np.load(p) for p in clip_paths(data_root, name, branch)]
                if [a.shape[0] for a in arrs] != list(rows[i]) or any(a.dtype != self.dtype or a.ndim != 2 or
                                                                      a.shape[1] < CHANNELS for a in arrs):
                    raise ValueError("clip %s changed on disk between the header pass and the ingest" % name)
                if host_check:
                    V.check_temporal_rows(arrs, name)
                V.check_finite_coordinates(arrs, name)         # always: no device-side check stands in for it
                for k, a in enumerate(arrs):
                    o = int(table[i, k] - r0)
                    host[o:o + a.shape[0]] = a[:, :CHANNELS]

            try:
                with ThreadPoolExecutor(max_workers=workers) as ex:
                    for c, (a, b) in enumerate(chunks):
                        s = c % len(stage)
                        if done[s] is not None:
                            done[s].synchronize()                     # the copy out of this staging buffer has finished
                        r0, r1 = int(first_row[a]), int(end_row[b - 1])
                        host = stage[s].numpy()
                        list(ex.map(lambda i: load_into(host, r0, i), range(a, b)))
                        with torch.cuda.stream(side):
                            self.src[r0:r1].copy_(stage[s][:r1 - r0], non_blocking=True)
                            _lib.call(rt, self.src, self.table, self.lists, a, b - a, self.err, stream=side.cuda_stream)
                            done[s] = torch.cuda.Event()
                            done[s].record(side)
            finally:
                side.synchronize()                                    # nothing of the ingest is in flight past this point
            torch.cuda.current_stream().wait_stream(side)
            flags, pos = (int(x) for x in self.err.cpu())
        if flags & ERR_NO_TEMPORAL_ROWS:
            n4 = int(self.table[pos, 10].item())
            raise ValueError(no_temporal_rows_message(index.v_name(self.vids[pos]), 4 if n4 == 0 else 7))

    def position_of(self, vid):
        """Dataset index -> table position."""
        try:
            return self._pos[int(vid)]
        except KeyError:
            raise KeyError("clip %d is not resident (not in the split that was ingested)" % int(vid)) from None

    def error_flags(self):
        """The device's error word (synchronises)."""
        return int(self.err[0].item())


def build_views_resident(res, sel, seed, epoch, return_idx=False, num_crop=V.NUM_CROP, num_point=V.NUM_POINT, recipe=None):
    """The (G*B, P, 4) float32 views (G = num_crop views of P = num_point points, facl_amd/philox.py's recipe) of the clips
    at table positions `sel` (device (B,) int32), one launch on the current stream.  With return_idx also the (B, G, P) int64
    pool rows.  A position outside the table raises the pool's error word and yields zeros for that clip.  `recipe`: a
    facl_amd.philox.Recipe, None = the default (the _gp entry)."""
    import torch
    from . import _lib
    V.check_view_size(num_crop, num_point)
    G, P = int(num_crop), int(num_point)
    B = sel.shape[0]
    if sel.dtype != torch.int32 or sel.dim() != 1 or not sel.is_contiguous():
        raise TypeError("sel must be a contiguous (B,) int32 tensor")
    _lib.require_cuda(sel, res.src)
    out = _lib.empty((G * B, P, 4), dtype=torch.float32, device=res.dev)
    idx = _lib.empty((B, G, P), dtype=torch.int64, device=res.dev) if return_idx else None
    V._call_view_entry("resident", res.dtype == np.float64, recipe, seed, lambda sd: (
        res.src, res.table, res.lists, res.n, sel, B, G, P, sd, int(epoch), out, idx, res.err))
    return (out, idx) if return_idx else out


class ResidentBatches:
    """What `DiskBatches(index, ..., vids, 'philox', device, seed=seed, epoch=epoch)` yields, from the resident pool:
    ((G*B, P, 4) float32 views, v_names, labels) per entry of `vids` (a list of (B_i,) arrays of dataset indices); G =
    `num_crop`, P = `num_point`, any size of the kernels' domain; `recipe`: the view recipe (None = the default).  Per batch: one (B,) int32 copy out of a reused pinned
    buffer and one launch, both on the current stream; no thread."""

    def __init__(self, resident, vids, seed=0, epoch=0, num_crop=V.NUM_CROP, num_point=V.NUM_POINT, recipe=None):
        import torch
        V.check_view_size(num_crop, num_point)
        self.num_crop, self.num_point, self.recipe = int(num_crop), int(num_point), recipe
        self.res, self.seed, self.epoch = resident, seed, epoch
        self.vids = [np.asarray(v).reshape(-1) for v in vids]
        bmax = max([len(v) for v in self.vids] + [1])
        self._pin = torch.empty((bmax,), dtype=torch.int32).pin_memory()
        self._sel = torch.empty((bmax,), dtype=torch.int32, device=resident.dev)
        self._copied = None
        self._i = 0

    def __iter__(self):
        return self

    def __next__(self):
        import torch
        if self._i >= len(self.vids):
            raise StopIteration
        vids = self.vids[self._i]
        self._i += 1
        res, B = self.res, len(vids)
        pos = np.fromiter((res.position_of(v) for v in vids), dtype=np.int32, count=B)
        with torch.cuda.device(res.dev):
            if self._copied is not None:
                self._copied.synchronize()                            # the previous copy has left the pinned buffer
            self._pin.numpy()[:B] = pos
            sel = self._sel[:B]
            sel.copy_(self._pin[:B], non_blocking=True)
            self._copied = torch.cuda.Event()
            self._copied.record()
            views = build_views_resident(res, sel, self.seed, self.epoch, num_crop=self.num_crop, num_point=self.num_point,
                                         recipe=self.recipe)
        names = [res.index.v_name(int(v)) for v in vids]
        labels = [res.index.label(int(v)) for v in vids]
        return views, names, labels

    def close(self):
        """Ends the iteration and reads the pool's error word once (the host maps every index through `position_of`, so a
        raised word means the table or the selection was corrupted)."""
        self._i = len(self.vids)
        flags = self.res.error_flags()
        if flags:
            raise RuntimeError("the resident views raised the device's error word (%d): the batches of this epoch are void"
                               % flags)
