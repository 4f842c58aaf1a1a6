"""NumPy restatement of the reference's 3DV generation (generate_data/generate_NTU.py), for modern NumPy.

A test helper: tests/test_gen3dv_cpu.py holds it to the reference's own results (tests/golden/gen3dv.npz, written by
tools/make_3dv_goldens.py), tests/test_gpu_gen3dv.py holds the HIP path (facl_amd/gen3dv.py) to it.  Every stage is a
function of its own so that both sides can be compared stage by stage; `generate_clip` chains them and draws from the two
host streams in the reference's order.  Also here: the integer-only procedure that makes the fixture's depth clips, and the
digest the fixture stores for arrays too large to commit.
"""
import hashlib
import zlib

import numpy as np

FX = FY = 365.481                       # generate_NTU.py:14-17
CX, CY = 257.346, 210.347
VOXEL = 30                              # :19
M = 5                                   # :20
K = 60                                  # :30
SAMPLE = 2048                           # :27
TOP, BOTTOM, SIDE = 60, 29, 10          # :31
LOW, UP = 50, 300                       # :356-357
TH_KEY, TH_ALL = 6, 5                   # :190-191
APP_MIN = 10                            # :52


# ---- stages -----------------------------------------------------------------------------------------------------------------
def crop(frame):
    """:339-351.  The two `-1:-10` slices select nothing.  The slice starts below go negative for a very low / very left
    last pixel and then wrap as Python slices do; kept, because the reference does it."""
    im = np.array(frame, copy=True)
    im[0:2, :] = 0
    im[:, 0:2] = 0
    r, c = np.nonzero(im)
    if r.size == 0:
        raise ValueError("frame without a non-zero pixel")
    im[:TOP, :] = 0
    im[int(r[-1]) - BOTTOM:, :] = 0
    im[:, :int(c.min()) + SIDE] = 0
    im[:, int(c.max()) - SIDE:] = 0
    return im


def motion_image(prev, cur):
    """:355-366: (pixels of `cur` whose change against `prev` is strictly between the thresholds, the new `prev`), int32."""
    cur = cur.astype(np.int32)
    d = np.abs(cur - prev)
    return np.where((d > LOW) & (d < UP), cur, 0).astype(np.int32), cur


def backproject(depth):
    """:321-335: (3, N) float64, pixels in row-major order; each coordinate is subtract, multiply, divide."""
    rows, cols = np.nonzero(depth > 0)
    d = depth[rows, cols]
    return np.array([(cols - CX) * d / FX, (rows - CY) * d / FY, d])


def choose_frames(n, py_random):
    """:121-132"""
    if n > K:
        return sorted(py_random.sample(list(range(n)), K))
    return list(range(n))


def bounding_box(points_list):
    """:165-181: (min xyz, max xyz, (dx, dy, dz))"""
    allp = np.concatenate(points_list, axis=1)
    mn, mx = allp.min(axis=1), allp.max(axis=1)
    return mn, mx, tuple(int(v) for v in (mx - mn) / VOXEL)


def window_bounds(n):
    return [round(n * a / 5) for a in range(6)]


def weight_table(n):
    """:409-438: (5, n) integer weights of frame i in channel m, zero outside the channel's window."""
    a = window_bounds(n)
    w = np.zeros((M, n), dtype=np.int64)
    for m, (lo, hi) in enumerate([(0, n), (0, a[2]), (a[1], a[3]), (a[2], a[4]), (a[3], n)]):
        i = np.arange(lo, hi)
        w[m, lo:hi] = (i - lo) * 2 - (hi - lo) + 1
    return w


def voxel_index(points, mn):
    return tuple(((points[k] - mn[k]) / VOXEL).astype(np.int32) for k in range(3))


def rank_pool(points_list, motion_list, mn, dims):
    """:369-440: (5, dx+1, dy+1, dz+1) and (1, ...) float64 volumes."""
    shape = tuple(d + 1 for d in dims)
    n = len(points_list)
    w = weight_table(n)
    vol = np.zeros((M,) + shape)
    key = np.zeros((1,) + shape)
    for i in range(n):
        occ = np.zeros(shape, dtype=bool)
        occ[voxel_index(points_list[i], mn)] = True
        vol += w[:, i].reshape(M, 1, 1, 1) * occ
        occ = np.zeros(shape, dtype=bool)
        occ[voxel_index(motion_list[i], mn)] = True
        key[0] += w[0, i] * occ
    return vol, key


def density_filter(v, th):
    """:277-296: keep a non-zero voxel off the grid's shell whose 3x3x3 block holds at least `th` non-zero voxels."""
    occ = (v != 0)
    cnt = np.zeros(v.shape, dtype=np.int64)
    pad = np.pad(occ.astype(np.int64), 1)
    for a in range(3):
        for b in range(3):
            for c in range(3):
                cnt += pad[a:a + v.shape[0], b:b + v.shape[1], c:c + v.shape[2]]
    inner = np.zeros(v.shape, dtype=bool)
    inner[1:-1, 1:-1, 1:-1] = True
    return np.where(occ & inner & (cnt >= th), v, 0.0)


def voxel_rows(vol):
    """:196-201: (rows (R, 8) float64, number of hits).  More than SAMPLE hits: the sorted unique (x, y, z)."""
    _, x, y, z = np.nonzero(vol)
    hits = x.shape[0]
    xyz = np.column_stack((x, y, z))
    if hits > SAMPLE:
        xyz = np.unique(xyz, axis=0)
    feat = vol[:, xyz[:, 0], xyz[:, 1], xyz[:, 2]]
    return np.concatenate((xyz, feat.T), axis=1), hits


def sample_rows(rows, hits, np_random):
    """:203-209: the comparison is on the hit count, the bound on the row count."""
    if hits < SAMPLE:
        idx = np_random.randint(0, rows.shape[0], size=SAMPLE - hits)
        return np.concatenate((rows, rows[idx]), axis=0)
    return rows[np_random.randint(0, rows.shape[0], size=SAMPLE)]


def key_volume(vol, key_filtered):
    """:212-214"""
    return np.where(key_filtered != 0, vol, 0.0)


def norm_constants(cloud):
    """:232-240: centres (3,), y_len, c_min (5,), c_len (5,) of the sampled motion cloud."""
    hi, lo = cloud.max(axis=0), cloud.min(axis=0)
    return (hi[:3] + lo[:3]) / 2, hi[1] - lo[1], lo[3:8], hi[3:8] - lo[3:8]


def normalise(cloud, consts):
    centre, y_len, c_min, c_len = consts
    out = cloud.copy()
    out[:, 0:3] = (cloud[:, 0:3] - centre) / y_len
    out[:, 3:8] = (cloud[:, 3:8] - c_min) / c_len - 0.5
    return out


def app_frame_choice(n, np_random):
    """:51-56"""
    if n < APP_MIN:
        return sorted(np_random.randint(0, n, APP_MIN).tolist())
    return list(range(n))


def app_rows(points, vol0, mn):
    """:61-73: (N, 4) unrounded voxel coordinates and channel 0 of the filtered volume at the point's voxel."""
    out = np.zeros((points.shape[1], 4))
    for k in range(3):
        out[:, k] = (points[k] - mn[k]) / VOXEL
    out[:, 3] = vol0[voxel_index(points, mn)]
    return out


def normalise_app(rows, consts):
    centre, y_len, c_min, c_len = consts
    out = rows.copy()
    out[:, 0:3] = (rows[:, 0:3] - centre) / y_len
    out[:, 3] = (rows[:, 3] - c_min[0]) / c_len[0] - 0.5
    return out


def sample_app(rows, np_random):
    """:252-257"""
    n = rows.shape[0]
    if n < SAMPLE:
        return np.concatenate((rows, rows[np_random.randint(0, n, size=SAMPLE - n)]), axis=0)
    return rows[np_random.randint(0, n, size=SAMPLE)]


# ---- the chain ---------------------------------------------------------------------------------------------------------------
def prepare(frames, chosen):
    """Everything before the first draw that depends on a count: crops, motion images, point lists, box, volumes, filters."""
    prev = crop(frames[0]).astype(np.int32)
    cropped, motion, pts, mpts = [], [], [], []
    for i in chosen:
        cur = crop(frames[i])
        mot, prev = motion_image(prev, cur)
        cropped.append(cur)
        motion.append(mot)
        mpts.append(backproject(mot))
        pts.append(backproject(cur))
    mn, mx, dims = bounding_box(pts)
    vol, key = rank_pool(pts, mpts, mn, dims)
    keyf = density_filter(key[0], TH_KEY)
    vol[0] = density_filter(vol[0].copy(), TH_ALL)
    return dict(cropped=cropped, motion=motion, points=pts, motion_points=mpts, mn=mn, mx=mx, dims=dims, vol=vol,
                key_raw=key, key_filtered=keyf)


def generate_clip(frames, np_random, py_random, intermediates=False):
    """One clip of :121-264: ((2048, 8), (2048, 8), (frames, 2048, 4)) float64.  `np_random` is the `numpy.random` module or
    a RandomState, `py_random` the `random` module or a random.Random: draws are made in the reference's order."""
    chosen = choose_frames(frames.shape[0], py_random)
    st = prepare(frames, chosen)
    app_choice = app_frame_choice(len(chosen), np_random)
    rows, hits = voxel_rows(st["vol"])
    cloud = sample_rows(rows, hits, np_random)
    kvol = key_volume(st["vol"], st["key_filtered"])
    krows, khits = voxel_rows(kvol)
    if krows.shape[0] == 0:
        raise ValueError("no key voxel survives the density filter")
    kcloud = sample_rows(krows, khits, np_random)
    consts = norm_constants(cloud)
    app = np.zeros((len(app_choice), SAMPLE, 4))
    app_lists = []
    for j, f in enumerate(app_choice):
        ar = app_rows(st["points"][f], st["vol"][0], st["mn"])
        app_lists.append(ar)
        app[j] = normalise_app(sample_app(ar, np_random), consts)
    out = (normalise(cloud, consts), normalise(kcloud, consts), app)
    if not intermediates:
        return out
    st.update(chosen=chosen, app_choice=app_choice, rows=rows, hits=hits, key_rows=krows, key_hits=khits, key_vol=kvol,
              consts=consts, app_lists=app_lists)
    return out, st


def lists_of(vol):
    """The two ordered lists the device builds for a 5-channel volume, as flat voxel indices (x * ny + y) * nz + z:
    the (m, x, y, z)-ordered hits and the (x, y, z)-ordered unique voxels."""
    _, x, y, z = np.nonzero(vol)
    flat = (x * vol.shape[2] + y) * vol.shape[3] + z
    return flat.astype(np.int32), np.unique(flat).astype(np.int32)


# ---- fixture helpers -----------------------------------------------------------------------------------------------------------
def digest(a):
    """sha256 over dtype, shape and bytes: what tests/golden/gen3dv.npz stores for arrays too large to commit."""
    a = np.ascontiguousarray(a)
    h = hashlib.sha256()
    h.update(("%s %s " % (a.dtype.str, a.shape)).encode())
    h.update(a.tobytes())
    return h.hexdigest()


def clip_crc(frames):
    return zlib.crc32(np.ascontiguousarray(frames).tobytes())


# Procedural depth clips, integers only.  A scene is a list of ellipses (centre row / column, radii, base depth) whose
# centre and depth move linearly or alternate with the frame number t; later ellipses overwrite earlier ones.
#   (row, col, rrad, crad, depth, drow, dcol, ddepth, alt)  -- per frame: row += drow * t, col += dcol * t,
#   depth += ddepth * t + alt * (t % 2)
H, W = 212, 256
CASES = {
    # fewer than 10 frames, a small swinging limb over a still trunk: both lists below 2048 hits, cancelling weights
    "few": dict(n=6, parts=[(130, 120, 62, 34, 2400, 0, 0, 0, 0), (110, 150, 14, 12, 2100, 1, 4, 25, 0)]),
    # 10..60 frames, the whole body sways: motion list over 2048 hits, key list too
    "mid": dict(n=14, parts=[(126, 126, 62, 50, 2600, 0, 1, 0, 90), (100, 70, 16, 14, 2300, 2, 3, 30, 0)]),
    # 10..60 frames, large still trunk and a small limb: motion list over 2048 hits, key list below
    "still": dict(n=12, parts=[(126, 126, 62, 56, 2600, 0, 0, 0, 0), (96, 110, 16, 14, 2200, 2, 3, 30, 0)]),
    # more than 60 frames: random.sample picks 60
    "long": dict(n=64, parts=[(126, 120, 60, 40, 2500, 0, 0, 2, 80), (100, 150, 14, 12, 2250, 0, 1, 6, 0)]),
}


def make_clip(case):
    """uint16 (n, H, W) depth frames of a fixture case (a name in CASES or a dict of the same form)."""
    spec = CASES[case] if isinstance(case, str) else case
    h, w = spec.get("hw", (H, W))
    r, c = np.mgrid[0:h, 0:w].astype(np.int64)
    out = np.zeros((spec["n"], h, w), dtype=np.uint16)
    for t in range(spec["n"]):
        for (pr, pc, rr, cr, d, dr, dc, dd, alt) in spec["parts"]:
            y, x = r - (pr + dr * t), c - (pc + dc * t)
            q = y * y * cr * cr + x * x * rr * rr
            inside = q < rr * rr * cr * cr
            # a dome: depth grows towards the rim, plus a small integer texture
            depth = d + dd * t + alt * (t % 2) + (q * 160) // (rr * rr * cr * cr) + (r * 7 + c * 3) % 11
            out[t][inside] = depth[inside].astype(np.uint16)
    return out
