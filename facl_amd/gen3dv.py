"""Depth frames -> the 3DV clouds of the reference's generate_data/generate_NTU.py, on the GPU (csrc/gen3dv.hip).

`generate_clips` takes the depth frames of a batch of clips (every file of each clip's folder, uint16) and returns per clip
what the reference saves: the motion cloud (2048, 8), the key cloud (2048, 8) and the appearance clouds (frames, 2048, 4),
float64.  The host keeps what is host work in the reference too: the choice of frames, the weight table, the bounding box
from the per-frame extents, and -- with mode 'numpy' -- the random draws, made from the given `np.random.RandomState` /
`random.Random` in the reference's order, so that a seeded run reproduces its files.  With mode 'philox' the rows are drawn
on the device by counter (seed, resolution, CRC of the clip's name): no draw depends on another clip or on the batch.

There is no CPU path: the NumPy restatement the tests compare with lives in tests/ref3dv.py.
"""
import zlib

import numpy as np
import torch

from . import _lib
from . import philox as PX

K = 60                      # generate_NTU.py:30
M = 5                       # :20
SAMPLE = 2048               # :27
APP_MIN = 10                # :52
TH_ALL, TH_KEY = 5, 6       # :190-191
MAX_FRAMES = 64             # include/facl_hip.h FACL_GEN3DV_MAX_FRAMES
MAX_PIXELS = 1 << 22        # FACL_GEN3DV_MAX_PIXELS
MAX_VOXELS = 1 << 24        # FACL_GEN3DV_MAX_VOXELS
MAX_VOXELS_TOTAL = 1 << 27  # FACL_GEN3DV_MAX_VOXELS_TOTAL
HOST_SLOT = 1               # philox counter slot of the draws the host makes (frame choices)
ERR_BITS = {1: "a point outside its clip's grid", 2: "pixel list overrun", 4: "bad frame table", 8: "an empty list or frame",
            16: "a drawn index out of range"}


def name_crc(name):
    return zlib.crc32(str(name).encode()) & 0xFFFFFFFF


# ---- host logic (no device) -------------------------------------------------------------------------------------------------
def weight_table(n):
    """(5, 64) int32: weight of chosen frame i in channel m (:409-438), zero outside the channel's window.  Channel 0 spans
    all frames, channels 1-4 the half-overlapping windows bounded by round(n * a / 5)."""
    if not 1 <= n <= MAX_FRAMES:
        raise ValueError("a clip is pooled from 1..%d frames, got %d" % (MAX_FRAMES, n))
    a = [round(n * j / 5) for j in range(6)]
    w = np.zeros((M, MAX_FRAMES), dtype=np.int32)
    for m, (lo, hi) in enumerate(((0, n), (0, a[2]), (a[1], a[3]), (a[2], a[4]), (a[3], n))):
        for i in range(lo, hi):
            w[m, i] = 2 * (i - lo) - (hi - lo) + 1
    return w


def _host_words(seed, resolution, crc, n):
    ctr = np.stack([np.arange(n, dtype=np.uint64), np.full(n, HOST_SLOT, dtype=np.uint64),
                    np.full(n, crc, dtype=np.uint64), np.full(n, resolution & 0xFFFFFFFF, dtype=np.uint64)], -1)
    return PX.philox4x32_10(ctr, PX.seed_key(seed))


def choose_frames(n, k=K, py_random=None, philox=None):
    """:121-132: every frame, or k of them drawn without replacement, ascending.  `py_random`: random.sample as the
    reference calls it; `philox` = (seed, resolution, crc): the k frames with the smallest 64-bit philox words."""
    if k > MAX_FRAMES:
        raise ValueError("at most %d frames per clip can be pooled (one bit each), k = %d" % (MAX_FRAMES, k))
    if n <= k:
        return list(range(n))
    if philox is not None:
        w = _host_words(philox[0], philox[1], philox[2], n).astype(np.uint64)
        order = np.argsort((w[:, 0] << np.uint64(32)) | w[:, 1], kind="stable")
        return sorted(int(i) for i in order[:k])
    return sorted(py_random.sample(list(range(n)), k))


def choose_app_frames(n, rng=None, philox=None):
    """:51-56: all n chosen frames, or 10 drawn with replacement when there are fewer than 10, ascending."""
    if n >= APP_MIN:
        return list(range(n))
    if philox is not None:
        w = _host_words(philox[0], philox[1], philox[2], APP_MIN)[:, 2]
        return sorted(PX.row_draw(w, n).tolist())
    return sorted(rng.randint(0, n, APP_MIN).tolist())


def draw_rows(rng, hits, rows):
    """:203-209 as indices into the row list: fewer than 2048 hits keep the list and append draws, otherwise 2048 draws."""
    if hits < SAMPLE:
        return np.concatenate((np.arange(hits), rng.randint(0, rows, size=SAMPLE - hits))).astype(np.int32)
    return rng.randint(0, rows, size=SAMPLE).astype(np.int32)


def draw_clip(rng, counts, app_counts):
    """The draws of one clip after its frame choices, in the reference's order: motion rows, key rows, one per appearance
    frame.  counts = (hits, unique, key hits, key unique).  Returns ((2, 2048), (frames, 2048)) int32."""
    hits, nu, khits, knu = (int(c) for c in counts)
    idx = np.stack((draw_rows(rng, hits, nu if hits > SAMPLE else hits),
                    draw_rows(rng, khits, knu if khits > SAMPLE else khits)))
    app = [draw_rows(rng, int(c), int(c)) for c in app_counts]
    return idx, np.stack(app)


def check_frames(name, files, has_pixel, kept):
    """files: the file index of the clip's uploaded frames (first file, then the chosen ones)."""
    for f, any_, cnt in zip(files, has_pixel, kept):
        if not any_:
            raise ValueError("clip %s: frame %d has no non-zero pixel (generate_NTU.py:346-348 fails on it)" % (name, f))
    for f, cnt in list(zip(files, kept))[1:]:
        if cnt == 0:
            raise ValueError("clip %s: frame %d has no pixel left after the crop of generate_NTU.py:347-350" % (name, f))


def check_counts(name, counts):
    if int(counts[0]) == 0:
        raise ValueError("clip %s: no voxel survives the density filter, the motion cloud is empty" % name)
    if int(counts[2]) == 0:
        raise ValueError("clip %s: no key voxel survives the density filter (generate_NTU.py:225 fails in randint(0, 0))"
                         % name)


def grid_of(ext, voxel_size):
    """:165-181 from the per-frame extents (min and max are exact in any order): (min, max, (nx, ny, nz))."""
    mn, mx = ext[:, :3].min(axis=0), ext[:, 3:].max(axis=0)
    d = (mx - mn) / voxel_size
    return mn, mx, tuple(int(v) + 1 for v in d)


# ---- the device path ---------------------------------------------------------------------------------------------------------
def _frames_of(f, name):
    if isinstance(f, torch.Tensor):
        _lib.require_cuda(f)
        if f.dtype not in (torch.uint16, torch.int16):
            raise ValueError("clip %s: depth frames are uint16" % name)
        f = f.view(torch.int16)
    elif not (isinstance(f, np.ndarray) and f.dtype == np.uint16):
        raise ValueError("clip %s: depth frames are a uint16 (frames, H, W) array" % name)
    if f.ndim != 3 or f.shape[0] < 1:
        raise ValueError("clip %s: depth frames are (frames, H, W), got %s" % (name, tuple(f.shape)))
    return f


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).pin_memory().to(device, non_blocking=True)


def generate_clips(frames_list, names, rng=None, py_random=None, mode="numpy", seed=0, resolution=0, device="cuda",
                   voxel_size=30, k=K, intermediates=False):
    """frames_list: per clip every depth frame of its folder, uint16 (n, H, W) NumPy arrays (uploaded through pinned memory)
    or CUDA tensors; names: the clips' names.  Returns a list of (motion (2048, 8), key (2048, 8), app (frames, 2048, 4))
    float64 NumPy arrays, with `intermediates=True` a list of (those three, dict of the stages' results)."""
    if mode not in ("numpy", "philox"):
        raise ValueError("rows are drawn with mode numpy or philox")
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("facl_amd ops run on the GPU only (device %s); there is no CPU path" % dev)
    if len(frames_list) != len(names) or not names:
        raise ValueError("one name per clip")
    if mode == "numpy" and rng is None:
        raise ValueError("mode numpy draws from the RandomState it is given")
    frames_list = [_frames_of(f, n) for f, n in zip(frames_list, names)]
    H, W = frames_list[0].shape[1:]
    if any(tuple(f.shape[1:]) != (H, W) for f in frames_list):
        raise ValueError("the clips of one batch share one image size")
    if H * W > MAX_PIXELS:
        raise ValueError("images of more than %d pixels are not supported" % MAX_PIXELS)
    B = len(names)
    crcs = [name_crc(n) for n in names]
    chosen = []
    for f, n, c in zip(frames_list, names, crcs):
        if mode == "numpy" and f.shape[0] > k and py_random is None:
            raise ValueError("clip %s has more than %d frames: mode numpy samples them from the random.Random it is given" % (n, k))
        chosen.append(choose_frames(f.shape[0], k, py_random, (seed, resolution, c) if mode == "philox" else None))
    with torch.cuda.device(dev):
        return _run(dev, frames_list, names, crcs, chosen, rng, mode, seed, resolution, float(voxel_size), H, W, B,
                    intermediates)


def _run(dev, frames_list, names, crcs, chosen, rng, mode, seed, resolution, voxel, H, W, B, intermediates):
    # frames: per clip its first file, then the chosen ones
    files = [[0] + c for c in chosen]
    first = np.cumsum([0] + [len(f) for f in files])               # frame offset of each clip
    NF = int(first[-1])
    if isinstance(frames_list[0], np.ndarray):
        pin = torch.empty((NF, H, W), dtype=torch.int16).pin_memory()
        host = pin.numpy().view(np.uint16)
        for b, f in enumerate(frames_list):
            host[first[b]:first[b + 1]] = f[files[b]]
        with _lib.timed("gen3dv_upload"):
            frames = pin.to(dev, non_blocking=True)
    else:
        frames = torch.cat([f[torch.as_tensor(files[b], device=f.device)] for b, f in enumerate(frames_list)]).to(dev)
    fbox = _lib.empty((NF, 4), dtype=torch.int32, device=dev)
    fcount = _lib.empty((NF,), dtype=torch.int32, device=dev)
    fext = _lib.empty((NF, 6), dtype=torch.float64, device=dev)
    with _lib.timed("gen3dv_frames"):
        _lib.call("facl_gen3dv_frames", frames, NF, H, W, fbox, fcount, fext)
    h_box, h_cnt, h_ext = fbox.cpu().numpy(), fcount.cpu().numpy(), fext.cpu().numpy()      # first of two small copies back

    fmeta = np.zeros((NF, 4), dtype=np.int32)
    cmin = np.zeros((B, 3), dtype=np.float64)
    cmax = np.zeros((B, 3), dtype=np.float64)
    cgrid = np.zeros((B, 4), dtype=np.int32)
    wtab = np.zeros((B, M, MAX_FRAMES), dtype=np.int32)
    NV = NP = 0
    for b in range(B):
        lo, hi = int(first[b]), int(first[b + 1])
        check_frames(names[b], files[b], h_box[lo:hi, 3], h_cnt[lo:hi])
        cmin[b], cmax[b], dims = grid_of(h_ext[lo + 1:hi], voxel)
        V = dims[0] * dims[1] * dims[2]
        if V > MAX_VOXELS or NV + V > MAX_VOXELS_TOTAL:
            raise ValueError("clip %s: a grid of %s voxels is beyond what the kernels were sized for" % (names[b], dims))
        cgrid[b] = dims + (NV,)
        NV += V
        wtab[b] = weight_table(hi - lo - 1)
        fmeta[lo] = (b, -1, lo, 0)
        for i, g in enumerate(range(lo + 1, hi)):
            fmeta[g] = (b, i, g - 1, NP)                               # the first chosen frame follows the first file
            NP += int(h_cnt[g])
    maxvox = int((cgrid[:, 0] * cgrid[:, 1] * cgrid[:, 2]).max())
    maxF = max(len(c) for c in chosen)
    d_fmeta, d_cmin, d_cgrid, d_wtab = (_dev(a, dev) for a in (fmeta, cmin, cgrid, wtab))
    occ = torch.zeros((2, NV), dtype=torch.int64, device=dev)
    pix = _lib.empty((NP,), dtype=torch.int32, device=dev)
    err = torch.zeros((1,), dtype=torch.int32, device=dev)
    vol = _lib.empty((M, NV), dtype=torch.int32, device=dev)
    key = _lib.empty((NV,), dtype=torch.int32, device=dev)
    vol0f = _lib.empty((NV,), dtype=torch.int32, device=dev)
    keyf = _lib.empty((NV,), dtype=torch.int32, device=dev)
    lists = _lib.empty((12 * NV,), dtype=torch.int32, device=dev)
    counts = _lib.empty((B, 4), dtype=torch.int32, device=dev)
    with _lib.timed("gen3dv_voxelise"):
        _lib.call("facl_gen3dv_voxelise", frames, NF, H, W, fbox, d_fmeta, d_cmin, d_cgrid, B, maxF, maxvox, NV, NP, voxel,
                  occ[0], occ[1], pix, err)
    with _lib.timed("gen3dv_volumes"):
        _lib.call("facl_gen3dv_volumes", occ[0], occ[1], d_wtab, d_cgrid, B, maxvox, NV, vol, key)
    with _lib.timed("gen3dv_filter"):
        _lib.call("facl_gen3dv_filter", vol, key, d_cgrid, B, maxvox, NV, TH_ALL, TH_KEY, vol0f, keyf)
    with _lib.timed("gen3dv_compact"):
        _lib.call("facl_gen3dv_compact", vol, vol0f, keyf, d_cgrid, B, maxvox, NV, lists, counts)
    h_counts = counts.cpu().numpy()                                    # second small copy: the draws' sizes depend on it
    _raise_err(err, "voxelise")
    for b in range(B):
        check_counts(names[b], h_counts[b])

    # frame choices of the appearance clouds and, with mode numpy, the draws: clip by clip in the reference's order
    ameta, idx, aidx, app_choice = [], [], [], []
    for b in range(B):
        lo = int(first[b]) + 1
        ph = (seed, resolution, crcs[b]) if mode == "philox" else None
        ch = choose_app_frames(len(chosen[b]), rng, ph)
        app_choice.append(ch)
        ameta += [(lo + f, b, j) for j, f in enumerate(ch)]
        if mode == "numpy":
            i2, ia = draw_clip(rng, h_counts[b], [h_cnt[lo + f] for f in ch])
            idx.append(i2)
            aidx.append(ia)
    NA = len(ameta)
    d_ameta = _dev(np.array(ameta, dtype=np.int32), dev)
    d_crc = _dev(np.array(crcs, dtype=np.uint32).view(np.int32), dev)
    d_idx = _dev(np.stack(idx), dev) if mode == "numpy" else None
    d_aidx = _dev(np.concatenate(aidx), dev) if mode == "numpy" else None
    out_raw = _lib.empty((B, SAMPLE, 8), dtype=torch.float64, device=dev)
    out_key = _lib.empty((B, SAMPLE, 8), dtype=torch.float64, device=dev)
    out_app = _lib.empty((NA, SAMPLE, 4), dtype=torch.float64, device=dev)
    norm = _lib.empty((B, 14), dtype=torch.float64, device=dev)
    with _lib.timed("gen3dv_sample"):
        _lib.call("facl_gen3dv_sample", vol, vol0f, lists, counts, d_cgrid, B, maxvox, NV, d_idx, int(seed), int(resolution),
                  d_crc, out_raw, out_key, norm, err)
    with _lib.timed("gen3dv_app"):
        _lib.call("facl_gen3dv_app", frames, NF, H, W, d_fmeta, fcount, pix, NP, d_ameta, NA, d_aidx, int(seed),
                  int(resolution), d_crc, d_cmin, d_cgrid, B, maxvox, NV, voxel, vol0f, norm, out_app, err)
    raw, keyc, app = out_raw.cpu().numpy(), out_key.cpu().numpy(), out_app.cpu().numpy()
    _raise_err(err, "sample")
    a0 = np.cumsum([0] + [len(c) for c in app_choice])
    outs = [(raw[b], keyc[b], app[a0[b]:a0[b + 1]]) for b in range(B)]
    if not intermediates:
        return outs
    h_vol, h_key, h_v0, h_kf, h_lists, h_norm = (t.cpu().numpy() for t in (vol, key, vol0f, keyf, lists, norm))
    res = []
    for b in range(B):
        nx, ny, nz, off = (int(v) for v in cgrid[b])
        V = nx * ny * nz
        base = 12 * off
        c = h_counts[b]
        lo = int(first[b]) + 1
        res.append((outs[b], dict(
            chosen=chosen[b], app_choice=app_choice[b], mn=cmin[b], mx=cmax[b], dims=(nx - 1, ny - 1, nz - 1),
            frame_counts=h_cnt[lo:int(first[b + 1])].copy(), counts=c.copy(), norm=h_norm[b].copy(),
            vol=h_vol[:, off:off + V].reshape(M, nx, ny, nz).copy(), key=h_key[off:off + V].reshape(nx, ny, nz).copy(),
            vol0_filtered=h_v0[off:off + V].reshape(nx, ny, nz).copy(),
            key_filtered=h_kf[off:off + V].reshape(nx, ny, nz).copy(),
            hits=h_lists[base:base + c[0]].copy(), unique=h_lists[base + 5 * V:base + 5 * V + c[1]].copy(),
            key_hits=h_lists[base + 6 * V:base + 6 * V + c[2]].copy(),
            key_unique=h_lists[base + 11 * V:base + 11 * V + c[3]].copy())))
    return res


def _raise_err(err, what):
    e = int(err.item())
    if e:
        raise RuntimeError("3DV generation (%s): %s" % (what, ", ".join(m for bit, m in ERR_BITS.items() if e & bit)))
