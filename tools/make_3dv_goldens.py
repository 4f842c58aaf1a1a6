#!/usr/bin/env python
"""Generate tests/golden/gen3dv.npz by running the REFERENCE's 3DV generator (generate_data/generate_NTU.py) on the
procedural depth clips of tests/ref3dv.py, in the style of tools/make_goldens.py.

Runs only where the reference is available; the tests only read the committed .npz.  Three stand-ins make the reference
run here: `np.float` / `np.int` (removed from NumPy), an `imageio` module whose `imread` hands out the generated frames,
and a `save_npy` that records what `main()` hands it (the reference's own reads three names that `main()` binds as locals).
`main()` reads '../ntu120dataset' and creates '../ntu/...': the tool builds that tree in a temporary folder and chdirs into
a sibling.

Recorded: (a) for every clip and "resolution" the three arrays of `main()` under np.random.seed / random.seed, and the next
value of both streams; (b) the results of the reference's functions called stage by stage.  Arrays too large to commit are
stored as digests (tests/ref3dv.py `digest`) next to their first rows; the clips themselves as a CRC (the tests regenerate
them).  The tool refuses inputs on which the reference warns or fails, or that miss a branch the tests need.

    python tools/make_3dv_goldens.py            # rewrites tests/golden/gen3dv.npz
"""
import argparse
import os
import random
import sys
import tempfile
import types
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference/generate_data"
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ref3dv as T                                          # noqa: E402

np.float, np.int = float, int                               # stand-in 1
FRAMES = {}                                                 # path of a frame file -> uint16 image
_imageio = types.ModuleType("imageio")
_imageio.imread = lambda path: FRAMES[os.path.normpath(path)].copy()
sys.modules["imageio"] = _imageio                           # stand-in 2
import generate_NTU as R                                    # noqa: E402  reference

OUT = os.path.join(ROOT, "tests", "golden", "gen3dv.npz")
NP_SEED, PY_SEED, STAGE_SEED = 20, 21, 22
# NTU-style folder names, sorted as the cases are listed
NAMES = {"few": "S001C001P001R001A001", "long": "S001C001P001R001A002", "mid": "S001C001P001R001A003",
         "still": "S001C001P001R001A004"}
HEAD = 64                                                   # rows of a digested array kept for diagnosis


def put(out, key, a, full=False):
    a = np.ascontiguousarray(a)
    out[key + "/sha"] = np.array(T.digest(a))
    if full:
        out[key] = a
    elif a.ndim >= 2:
        out[key + "/head"] = a.reshape(-1, a.shape[-1])[:HEAD]


def run_main(tmp, clips, out):
    work = os.path.join(tmp, "work")
    os.makedirs(work)
    for case, frames in clips.items():
        d = os.path.join(tmp, "ntu120dataset", "nturgbd_depth_masked_s001", "nturgb+d_depth_masked", NAMES[case])
        os.makedirs(d)
        for i, f in enumerate(frames):
            p = os.path.join(d, "MDepth-%08d.png" % (i + 1))
            open(p, "w").close()
            FRAMES[os.path.normpath(os.path.join("..", os.path.relpath(p, tmp)))] = f
    saved = []
    R.save_npy = lambda data, filename, mode=1: saved.append((filename, mode, np.array(data, copy=True)))   # stand-in 3
    cwd = os.getcwd()
    os.chdir(work)
    try:
        np.random.seed(NP_SEED)
        random.seed(PY_SEED)
        R.main()
        out["main/np_next"] = np.int64(np.random.randint(0, 2 ** 31 - 1))
        out["main/py_next"] = np.float64(random.random())
    finally:
        os.chdir(cwd)
    order = sorted(clips, key=lambda c: NAMES[c])
    assert len(saved) == 3 * 3 * len(order)
    it = iter(saved)
    for res in range(3):
        for case in order:
            for kind, mode, suffix in (("raw", 1, ".npy"), ("key", 2, "_key.npy"), ("app", 3, "_app.npy")):
                name, m, a = next(it)
                assert name == NAMES[case] + suffix and m == mode and a.dtype == np.float64
                assert np.isfinite(a).all(), (case, kind)
                put(out, "main/%d/%s/%s" % (res, case, kind), a)


def run_stages(case, frames, out):
    random.seed(STAGE_SEED)
    n = frames.shape[0]
    chosen = sorted(random.sample(list(range(n)), R.K)) if n > R.K else list(range(n))
    out[case + "/chosen"] = np.array(chosen, dtype=np.int64)
    paths = []
    for i, f in enumerate(frames):
        FRAMES[os.path.normpath("stage/%s/%d" % (case, i))] = f
        paths.append("stage/%s/%d" % (case, i))
    prev = R.load_depth_from_img(paths[0]).astype(np.int32)
    cropped, motion, pts, mpts = [], [], [], []
    for i in chosen:
        cur = R.load_depth_from_img(paths[i])
        mot, prev = R.locate_motion(prev, cur)
        cropped.append(cur)
        motion.append(mot)
        mpts.append(R.depth_to_pointcloud(mot, 1))
        pts.append(R.depth_to_pointcloud(R.load_depth_from_img(paths[i]), 1))
    put(out, case + "/cropped", np.stack(cropped))
    put(out, case + "/motion", np.stack(motion))
    put(out, case + "/points", np.concatenate(pts, axis=1).T)
    put(out, case + "/motion_points", np.concatenate(mpts, axis=1).T)
    out[case + "/counts"] = np.array([p.shape[1] for p in pts], dtype=np.int64)
    out[case + "/motion_counts"] = np.array([p.shape[1] for p in mpts], dtype=np.int64)
    allp = np.concatenate(pts, axis=1)
    mn, mx = allp.min(axis=1), allp.max(axis=1)
    dx, dy, dz = map(int, (mx - mn) / R.voxel_size)
    out[case + "/min"], out[case + "/max"] = mn, mx
    out[case + "/dims"] = np.array([dx, dy, dz], dtype=np.int64)
    vol, key = R.get_modify_rankpooling_point(dx, dy, dz, len(chosen), mn[0], mn[1], mn[2], pts, mpts, M=5)
    assert np.array_equal(vol, np.rint(vol)) and np.array_equal(key, np.rint(key))
    out[case + "/vol_raw"] = vol.copy()
    out[case + "/key_raw"] = key.copy()
    keyf = R.disca_voxel(key[0].copy(), 6)
    vol0 = R.disca_voxel(vol[0].copy(), 5)
    out[case + "/key_filtered"] = keyf
    out[case + "/vol0_filtered"] = vol0
    vol[0] = vol0
    np.random.seed(STAGE_SEED)
    app = R.append_points(pts, vol, mn[0], mn[1], mn[2])
    put(out, case + "/app_rows", np.concatenate(app, axis=0))
    out[case + "/app_counts"] = np.array([a.shape[0] for a in app], dtype=np.int64)
    # the branches this case is in, for the tool's own checks
    hits = int(np.count_nonzero(vol))
    khits = int(np.count_nonzero(np.where(keyf != 0, vol, 0.0)))
    occupied = np.zeros(vol.shape[1:], dtype=bool)
    for p in pts:
        occupied[tuple(((p[k] - mn[k]) / R.voxel_size).astype(np.int32) for k in range(3))] = True
    cancel = int(np.count_nonzero(occupied & (np.abs(vol).sum(axis=0) == 0) & (R.disca_voxel(occupied * 1.0, 5) != 0)))
    out[case + "/hits"] = np.array([hits, khits, int(np.count_nonzero(keyf)), cancel], dtype=np.int64)
    return hits, khits, int(np.count_nonzero(keyf)), cancel


def weight_tables(out):
    """One point per frame, each in a voxel of its own: the volume then holds the weight of frame i in channel m."""
    for n in range(1, R.K + 1):
        pts = [np.array([[15.0 + 30.0 * i], [15.0], [15.0]]) for i in range(n)]
        vol, key = R.get_modify_rankpooling_point(n - 1, 0, 0, n, 0.0, 0.0, 0.0, pts, pts, M=5)
        assert np.array_equal(key[0, :, 0, 0], vol[0, :, 0, 0])
        out["weights/%d" % n] = vol[:, :, 0, 0].astype(np.int32)


def main():
    argparse.ArgumentParser(description=__doc__).parse_args()
    out = {}
    clips = {c: T.make_clip(c) for c in T.CASES}
    out["cases"] = np.array(sorted(clips))
    out["names"] = np.array([NAMES[c] for c in sorted(clips)])
    for c, f in clips.items():
        out[c + "/crc"] = np.int64(T.clip_crc(f))
    with warnings.catch_warnings():
        warnings.simplefilter("error")                      # the reference must finish without a warning
        with tempfile.TemporaryDirectory() as tmp:
            run_main(tmp, clips, out)
        br = {c: run_stages(c, f, out) for c, f in clips.items()}
        weight_tables(out)
    for c, (hits, khits, kvox, cancel) in sorted(br.items()):
        print("%-6s frames %2d  hits %5d  key hits %5d  key voxels %4d  cancelling occupied voxels %d"
              % (c, clips[c].shape[0], hits, khits, kvox, cancel))
    assert any(h[0] < T.SAMPLE for h in br.values()) and any(h[0] > T.SAMPLE for h in br.values()), "motion branch"
    assert any(h[1] < T.SAMPLE for h in br.values()) and any(h[1] > T.SAMPLE for h in br.values()), "key branch"
    assert all(h[2] >= 40 for h in br.values()), "too few surviving key voxels"
    assert any(h[3] > 0 for h in br.values()), "no occupied voxel with cancelling weights"
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
