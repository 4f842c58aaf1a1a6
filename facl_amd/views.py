"""GPU view construction for a batch of clips.

Mirrors the per-sample work of the reference's dataset class (training_code/cn3D_data_set.py: `__getitem__` :99-140,
`get_temporal_augment_data` :654-663, `get_data_train` :285-350 with `jitter_point_cloud` :767-778,
`reverse_transform` :708-713, `rotate_trans` :734-749) plus the loop head of cn3d_train_motion_GL.py:225-228
(`permute(1,0,2,3).reshape(-1,N,D)`, `.type(FloatTensor)`): the 16-worker NumPy pipeline and the float64 H2D copy
collapse into one host pass that only DRAWS the random numbers -- in the reference's order, from the generator it is
given, so a seed reproduces the reference's views -- and one HIP launch (csrc/views.hip) that gathers, jitters,
mirrors, rotates, casts and writes the view-major (G*B, 512, 4) float32 tensor the grouping op consumes.
"""
import numpy as np
import torch

from . import _lib

NUM_POINT = 512        # cn3D_data_set.py:24
NUM_CROP = 10          # get_data_train(..., num_crop=10)


def draw_clip(rng, points, key_points, res_points_1, res_points_2, base):
    """All random draws of one `__getitem__`, in call order.  `base` = row offsets of the four source clouds inside
    the packed batch buffer.  Returns (idx (10,512) int32 absolute rows, noise (7,512,3) float64, cossin (2,2))."""
    def nonzero_rows(t):                                   # get_temporal_augment_data: rows with a non-zero channel t
        nz = np.flatnonzero(points[:, t] != 0)
        return nz[rng.randint(0, nz.shape[0], 512)]
    t2 = nonzero_rows(4)
    t4 = nonzero_rows(7)
    idx = np.empty((NUM_CROP, NUM_POINT), dtype=np.int64)
    noise = np.empty((7, NUM_POINT, 3), dtype=np.float64)
    cs = np.empty((2, 2), dtype=np.float64)
    P, Kp, R1, R2 = points.shape[0], key_points.shape[0], res_points_1.shape[0], res_points_2.shape[0]
    idx[0] = base[0] + rng.randint(0, P, NUM_POINT)                          # raw_p
    idx[1] = base[0] + rng.randint(0, P, NUM_POINT)                          # rev_p
    noise[0] = rng.randn(1, NUM_POINT, 3)[0]
    noise[1] = rng.randn(1, NUM_POINT, 3)[0]                                 # inside reverse_transform
    idx[2] = base[1] + rng.randint(0, Kp, NUM_POINT)                         # ke1_p
    noise[2] = rng.randn(1, NUM_POINT, 3)[0]
    idx[3] = base[1] + rng.randint(0, Kp, NUM_POINT)                         # ke2_p
    noise[3] = rng.randn(1, NUM_POINT, 3)[0]
    noise[4] = rng.randn(1, NUM_POINT, 3)[0]
    for k, (vi, ni) in enumerate(((4, 5), (5, 6))):                          # ro1_p, ro2_p
        idx[vi] = base[0] + rng.randint(0, P, NUM_POINT)
        noise[ni] = rng.randn(1, NUM_POINT, 3)[0]
        angle = (rng.rand() - 0.5) * np.pi * 0.8
        cs[k] = (np.cos(angle), np.sin(angle))
    idx[6] = base[0] + t2                                                    # ti1_p / ti2_p: no new draws
    idx[7] = base[0] + t4
    idx[8] = base[2] + rng.randint(0, R1, NUM_POINT)                         # rs1_p
    idx[9] = base[3] + rng.randint(0, R2, NUM_POINT)                         # rs2_p
    return idx.astype(np.int32), noise, cs


def _device_draws(clips, bases, gen, dev):
    """The random draws of a whole batch ON THE DEVICE (torch generator `gen`): the same distributions as draw_clip -- 512
    uniform row draws with replacement per view, rows of non-zero temporal channel for the two temporal views, standard-normal
    jitter, a uniform rotation angle in +-0.4 pi -- but NOT NumPy's stream (a seed does not reproduce the reference's views;
    the throughput mode: the host draws of draw_clip cost ~0.19 ms per clip, 6 ms per batch of 32)."""
    B = len(clips)
    src_of = (0, 0, 1, 1, 0, 0, 2, 3)                               # source cloud of views 0,1,2,3,4,5,8,9
    sizes = torch.tensor([[c[k].shape[0] for k in src_of] for c in clips], dtype=torch.float64).to(dev)
    base = torch.tensor([[bases[b][k] for k in src_of] for b in range(B)], dtype=torch.int64).to(dev)
    u = torch.rand((B, 8, NUM_POINT), generator=gen, device=dev, dtype=torch.float64)
    idx8 = torch.minimum((u * sizes.unsqueeze(-1)).long(), (sizes.long() - 1).unsqueeze(-1)) + base.unsqueeze(-1)
    pmax = max(c[0].shape[0] for c in clips)
    masks = np.zeros((2, B, pmax), dtype=np.float32)
    for b, c in enumerate(clips):
        masks[0, b, :c[0].shape[0]] = c[0][:, 4] != 0
        masks[1, b, :c[0].shape[0]] = c[0][:, 7] != 0
    m = torch.from_numpy(masks).to(dev)
    base0 = torch.tensor([bases[b][0] for b in range(B)], dtype=torch.int64, device=dev).unsqueeze(-1)
    t2 = torch.multinomial(m[0], NUM_POINT, replacement=True, generator=gen) + base0
    t4 = torch.multinomial(m[1], NUM_POINT, replacement=True, generator=gen) + base0
    idx = torch.stack((idx8[:, 0], idx8[:, 1], idx8[:, 2], idx8[:, 3], idx8[:, 4], idx8[:, 5], t2, t4, idx8[:, 6], idx8[:, 7]), dim=1)
    noise = torch.randn((B, 7, NUM_POINT, 3), generator=gen, device=dev, dtype=torch.float64)
    ang = (torch.rand((B, 2), generator=gen, device=dev, dtype=torch.float64) - 0.5) * (np.pi * 0.8)
    cs = torch.stack((torch.cos(ang), torch.sin(ang)), dim=-1)
    return idx.to(torch.int32).contiguous(), noise, cs.contiguous()


def check_view_size(num_crop, num_point):
    """The domain of the philox kernels (include/facl_hip.h): 1..64 views; 64..4096 points in multiples of 64."""
    if not (1 <= int(num_crop) <= 64) or not (64 <= int(num_point) <= 4096) or int(num_point) % 64:
        raise ValueError("philox views: 1 <= num_crop <= 64 and 64 <= num_point <= 4096 in multiples of 64 (got %r, %r)"
                         % (num_crop, num_point))


def build_views(clips, rng=None, device="cuda", device_rng=None, philox=None, num_crop=NUM_CROP, num_point=NUM_POINT,
                recipe=None):
    """clips: list of (points (P,>=8), key_points, res_points_1, res_points_2) NumPy arrays of one dtype (float32 or
    float64), the arrays `__getitem__` loads for a video.  Returns the (10*B, 512, 4) float32 CUDA tensor = the
    reference's `data1` (view-major rows g*B+b).  `rng`: np.random.RandomState (default: NumPy's global generator,
    like the reference): every draw happens on the host in the reference's order, a seed reproduces its views.
    `device_rng` (a torch.Generator on the device): draw on the device instead -- same distributions, another stream,
    no per-clip host work.  `philox` = (seed, epoch, clip_ids): counter-based draws on the device (csrc/views_philox.hip):
    a clip's views depend on (seed, epoch, its dataset index clip_ids[b]) only.  `num_crop`, `num_point`: with `philox`
    any (G, P) of the kernels' domain -> (G*B, P, 4) (the recipe is in facl_amd/philox.py); the other two streams are the
    reference's and know 10 x 512 only.  `recipe` (facl_amd.philox.Recipe; None = the reference's ten kinds at its strengths):
    the kinds of a round and the strengths, with `philox` only."""
    if philox is None and recipe is not None and not recipe.is_default():
        raise ValueError("the reference's stream defines its ten views only; another view recipe needs the counter-based "
                         "draws (philox)")
    if philox is not None:
        check_view_size(num_crop, num_point)
        src, meta, dt = pack_clips(clips, philox[2])
        dev = torch.device(device)
        return build_views_philox(torch.from_numpy(src).to(dev), torch.from_numpy(meta).to(dev), dt, philox[0], philox[1],
                                  num_crop=num_crop, num_point=num_point, recipe=recipe)
    if (num_crop, num_point) != (NUM_CROP, NUM_POINT):
        raise ValueError("the reference's stream defines %d views of %d points only; other sizes need the counter-based "
                         "draws (philox)" % (NUM_CROP, NUM_POINT))
    rng = np.random if rng is None else rng
    B = len(clips)
    dt = clips[0][0].dtype
    if dt not in (np.float32, np.float64):
        raise TypeError("source clouds must be float32 or float64")
    rows, off = [], 0
    idxs, noises, css, bases = [], [], [], []
    for clip in clips:
        if any(a.dtype != dt or a.ndim != 2 or a.shape[1] < 8 for a in clip):
            raise ValueError("every source cloud must be (rows, >=8) of one dtype")
        base = []
        for a in clip:
            base.append(off)
            rows.append(np.ascontiguousarray(a[:, :8]))
            off += a.shape[0]
        bases.append(base)
        if device_rng is None:
            i, n, c = draw_clip(rng, clip[0], clip[1], clip[2], clip[3], base)
            idxs.append(i); noises.append(n); css.append(c)
    dev = torch.device(device)
    src = torch.from_numpy(np.concatenate(rows, 0)).to(dev)
    if device_rng is None:
        idx = torch.from_numpy(np.stack(idxs)).to(dev)
        noise = torch.from_numpy(np.stack(noises)).to(dev)
        cs = torch.from_numpy(np.stack(css)).to(dev)
    else:
        idx, noise, cs = _device_draws(clips, bases, device_rng, dev)
    out = _lib.empty((NUM_CROP * B, NUM_POINT, 4), dtype=torch.float32, device=dev)
    _lib.require_cuda(out)
    _lib.call("facl_build_views_f32" if dt == np.float32 else "facl_build_views_f64", src, src.shape[0], 8, idx, noise, cs, B, out)
    return out


def check_temporal_rows(clip, name):
    """get_temporal_augment_data (:654-663) draws from the rows whose channel 4 / 7 is non-zero: a clip without any cannot
    give its temporal views (the reference fails inside np.random.randint(0, 0))."""
    for t in (4, 7):
        if not (clip[0][:, t] != 0).any():
            raise ValueError("clip %s: no row of its point cloud has a non-zero channel %d, so its temporal view cannot be "
                             "drawn (cn3D_data_set.py:654-663)" % (name, t))


_F32_MAX = float(np.finfo(np.float32).max)


def check_finite_coordinates(clip, name):
    """Every xyz of the four source clouds must be a finite float32: the views' first 64 rows are the grouping kernel's
    centroids, and its radix select (csrc/group.hip) orders distance bit patterns that it takes for real numbers.  With a
    NaN / inf centroid every key is NaN; padding indices >= N (N no multiple of 64) are then kept as neighbours and read past
    the cloud, and with a sign-bit NaN nothing is selected at all and the emission reads indices out of unwritten LDS.  The
    clips are host arrays here, so the check costs no device synchronisation.  Feature channels are NOT checked: a NaN there
    travels through the step and ends in check_finite_loss's FloatingPointError."""
    for k, a in enumerate(clip):
        xyz = a[:, :3]
        if not (np.abs(xyz) <= _F32_MAX).all():              # False for NaN, inf and what overflows the float32 views
            r, c = np.argwhere(~(np.abs(xyz) <= _F32_MAX))[0]
            raise ValueError("clip %s: non-finite coordinate %r in row %d, column %d of source cloud %d: the grouping needs "
                             "finite xyz (fix or drop the clip)" % (name, float(xyz[r, c]), r, c, k))


def pack_clips(clips, clip_ids, out=None):
    """The batch's source clouds packed row-wise, (rows, 8) in the clips' one dtype, and the (B, 9) int32 meta of
    csrc/views_philox.hip (row offsets and counts of the four clouds, dataset index).  Checks what the kernels assume:
    one float dtype, 2-D (rows >= 1, >= 8 channels) clouds, non-zero temporal rows, finite coordinates.  `out`: a (>= rows, 8) array to pack
    into (a pinned staging buffer); returns (src, meta, dtype) with src a view of it."""
    dt = clips[0][0].dtype
    if dt not in (np.float32, np.float64):
        raise TypeError("source clouds must be float32 or float64")
    B = len(clips)
    meta = np.empty((B, 9), dtype=np.int32)
    off = 0
    for b, clip in enumerate(clips):
        if any(a.dtype != dt or a.ndim != 2 or a.shape[1] < 8 or a.shape[0] < 1 for a in clip):
            raise ValueError("every source cloud must be (rows >= 1, >= 8) of one dtype")
        check_temporal_rows(clip, clip_ids[b])
        check_finite_coordinates(clip, clip_ids[b])
        for k, a in enumerate(clip):
            meta[b, k], meta[b, 4 + k] = off, a.shape[0]
            off += a.shape[0]
        meta[b, 8] = int(clip_ids[b])
    if off >= 1 << 30:
        raise ValueError("batch too large: %d source rows" % off)
    src = np.empty((off, 8), dtype=dt) if out is None else out[:off]
    for b, clip in enumerate(clips):
        for k, a in enumerate(clip):
            src[meta[b, k]:meta[b, k] + a.shape[0]] = a[:, :8]
    return src, meta, dt


def recipe_args(recipe):
    """The three trailing arguments of the C ABI's recipe entries: HOST arrays, read before the launch.  Returns (the two
    arrays -- keep them alive over the call --, (kinds, n_kinds, strengths))."""
    kinds, strengths = np.ascontiguousarray(recipe.codes(), dtype=np.int32), np.ascontiguousarray(recipe.strengths(), dtype=np.float64)
    return (kinds, strengths), (kinds.ctypes.data, int(kinds.shape[0]), strengths.ctypes.data)


def _call_view_entry(stem, f64, recipe, seed, args):
    """What the philox entries' callers share (build_views_philox, resident.build_views_resident): calls
    facl_build_views_<stem>_{gp | recipe}_{f32 | f64} on the current stream.  `args(seed)` gives the entry's arguments up to the
    recipe's, with the seed as the signed 64-bit integer the C ABI takes; the recipe's host arrays follow and stay alive over
    the call."""
    name = "facl_build_views_%s_%s_%s" % (stem, "gp" if recipe is None else "recipe", "f64" if f64 else "f32")
    keep, extra = ((), ()) if recipe is None else recipe_args(recipe)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    _lib.call(name, *args(seed - (1 << 64) if seed >= 1 << 63 else seed), *extra)
    del keep


def build_views_philox(src, meta, dt, seed, epoch, return_idx=False, num_crop=NUM_CROP, num_point=NUM_POINT, recipe=None):
    """Device half of the philox mode: src (rows, 8) and meta (B, 9) int32 on the device (pack_clips' layout, temporal
    rows already checked).  Two launches on the current stream: the temporal-row compaction, then the views.
    Returns the (G*B, P, 4) float32 views of G = num_crop views of P = num_point points (and, with return_idx, the
    (B, G, P) source rows and the error word).  `recipe`: a facl_amd.philox.Recipe, None = the default (the _gp entry)."""
    check_view_size(num_crop, num_point)
    G, P = int(num_crop), int(num_point)
    dev = src.device
    B, rows = meta.shape[0], src.shape[0]
    lists = _lib.empty((2, rows), dtype=torch.int32, device=dev)
    counts = _lib.empty((B, 2), dtype=torch.int32, device=dev)
    err = torch.zeros((1,), dtype=torch.int32, device=dev)
    out = _lib.empty((G * B, P, 4), dtype=torch.float32, device=dev)
    idx = _lib.empty((B, G, P), dtype=torch.int32, device=dev) if return_idx else None
    _lib.require_cuda(out)
    f64 = dt == np.float64
    _lib.call("facl_views_temporal_rows_f64" if f64 else "facl_views_temporal_rows_f32", src, rows, 8, meta, B, lists, counts, err)
    _call_view_entry("philox", f64, recipe, seed, lambda sd: (src, rows, 8, meta, lists, counts, sd, int(epoch), B, G, P, out, idx))
    return (out, idx, err) if return_idx else out


def synthetic_raw_clip(seed, dtype=np.float32, P=900, Kp=300, R1=500, R2=200):
    """The four (rows, 8) source clouds `__getitem__` loads for one video (cn3D_data_set.py:105-116), synthetic: uniform
    coordinates / channels in [-0.5, 0.5) with zeros sprinkled into the two temporal channels (the rows the temporal views
    must skip).  `--synthetic 2` of the training entries feeds these through build_views, so the loop body runs from the
    loader's output on (cn3d_train_motion_GL.py:224-228)."""
    r = np.random.RandomState(seed)
    pts = (r.rand(P, 8) - 0.5).astype(dtype)
    pts[::3, 4] = 0
    pts[1::4, 7] = 0
    return pts, (r.rand(Kp, 8) - 0.5).astype(dtype), (r.rand(R1, 8) - 0.5).astype(dtype), (r.rand(R2, 8) - 0.5).astype(dtype)
