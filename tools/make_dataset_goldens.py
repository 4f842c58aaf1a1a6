#!/usr/bin/env python
"""Generate tests/golden/dataset.npz by running the REFERENCE's dataset class (training_code/cn3D_data_set.py
`NTU_RGBD_new`) on generated file names and small generated clips, in the style of tools/make_goldens.py.

Runs only where the reference is available; the tests only read the committed .npz.  The reference's paths are the
literals '../ntu/3DV_ntu60/...': the generator builds that tree in a temporary folder and chdirs into a sibling of
`ntu/`, so that they resolve.  Same harness-side stand-ins as tools/make_goldens.py (empty `imageio` module).

    python tools/make_dataset_goldens.py            # rewrites tests/golden/dataset.npz
"""
import argparse
import os
import sys
import tempfile
import types
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference/training_code"
sys.path.insert(0, REF)
sys.modules.setdefault("imageio", types.ModuleType("imageio"))
import cn3D_data_set as R_data                              # noqa: E402  reference

OUT = os.path.join(ROOT, "tests", "golden", "dataset.npz")
SENTINEL = "S017C003P020R002A060.npy"

# split modes: (tag, ctor kwargs)
MODES = [
    ("subject_train", dict(DATA_CROSS_VIEW=False, full_train=True)),
    ("subject_trainval", dict(DATA_CROSS_VIEW=False, full_train=False)),
    ("subject_validation", dict(DATA_CROSS_VIEW=False, validation=True)),
    ("subject_test", dict(DATA_CROSS_VIEW=False, test=True)),
    ("view_train", dict(DATA_CROSS_VIEW=True)),
    ("view_test", dict(DATA_CROSS_VIEW=True, test=True)),
    ("set_train", dict(DATA_CROSS_SET=True)),
    ("set_test", dict(DATA_CROSS_SET=True, test=True)),
]


def gen_names(rng, n):
    """n distinct names spread over setups 1..32, cameras 1..3, performers 1..106, replications 1..2, actions 1..120."""
    out = set()
    while len(out) < n:
        out.add("S%03dC%03dP%03dR%03dA%03d.npy" % (rng.randint(1, 33), rng.randint(1, 4), rng.randint(1, 107),
                                                   rng.randint(1, 3), rng.randint(1, 121)))
    return sorted(out)


def opt_of(dataset, branch="0"):
    return SimpleNamespace(SAMPLE_NUM=2048, INPUT_FEATURE_NUM=4, depth_path="", dataset=dataset, branch_choose=branch)


def make_clip(seed, P, Kp, R1, R2):
    r = np.random.RandomState(seed)
    pts = r.rand(P, 8) - 0.5
    pts[r.rand(P) < 0.4, 4] = 0
    pts[r.rand(P) < 0.6, 7] = 0
    return pts, r.rand(Kp, 8) - 0.5, r.rand(R1, 8) - 0.5, r.rand(R2, 8) - 0.5


def main():
    argparse.ArgumentParser(description=__doc__).parse_args()
    out = {}
    rng = np.random.RandomState(5)
    names = gen_names(rng, 40)
    lists = {"with": sorted(set(names) | {SENTINEL}), "without": [n for n in names if n != SENTINEL]}
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        work = os.path.join(tmp, "work")
        os.makedirs(work)
        os.chdir(work)
        try:
            for tag, lst in lists.items():
                d = os.path.join(tmp, "index_" + tag)
                os.makedirs(d)
                for n in lst:
                    open(os.path.join(d, n), "w").close()
                out[f"names_{tag}"] = np.array(lst)
                for dataset in ("ntu60", "ntu120"):
                    for mode, kw in MODES:
                        key = f"{tag}/{dataset}/{mode}"
                        try:
                            ds = R_data.NTU_RGBD_new(root_path=d, opt=opt_of(dataset), **kw)
                        except ValueError:                       # list.index: the ntu60 sentinel is missing
                            out[key + "/raises"] = np.int32(1)
                            continue
                        out[key + "/vid_ids"] = np.array(ds.vid_ids, dtype=np.int64)
                        out[key + "/labels"] = np.array([ds.id_to_action[v] for v in ds.vid_ids], dtype=np.int64)
                        out[key + "/v_names"] = np.array([ds.id_to_vidName[v][:20] for v in ds.vid_ids])
            # items: three clips in the reference layout, __getitem__ under np.random.seed(s)
            item_names = ["S001C002P001R001A007", "S002C003P002R002A013", "S003C002P004R001A042"]
            shapes = [(300, 200, 150, 100), (257, 129, 64, 33), (400, 96, 200, 80)]
            base = os.path.join(tmp, "ntu", "3DV_ntu60", "reslution")
            for res, sub in (("Resolution60", "raw"), ("Resolution60", "others"), ("Resolution30", "raw"), ("Resolution10", "raw")):
                os.makedirs(os.path.join(base, res, sub), exist_ok=True)
            for i, (n, sh) in enumerate(zip(item_names, shapes)):
                clip = make_clip(100 + i, *sh)
                for k, a in enumerate(clip):
                    out[f"item{i}/cloud{k}"] = a
                np.save(os.path.join(base, "Resolution60", "raw", n + ".npy"), clip[0])
                np.save(os.path.join(base, "Resolution60", "others", n + "_key.npy"), clip[1])
                np.save(os.path.join(base, "Resolution30", "raw", n + ".npy"), clip[2])
                np.save(os.path.join(base, "Resolution10", "raw", n + ".npy"), clip[3])
            out["item_names"] = np.array(item_names)
            ds = R_data.NTU_RGBD_new(root_path="../ntu/3DV_ntu60/reslution/Resolution60/raw/", opt=opt_of("ntu120"),
                                     DATA_CROSS_VIEW=True)
            assert [ds.id_to_vidName[v][:20] for v in ds.vid_ids] == item_names
            for s in (3, 11):
                np.random.seed(s)
                for i in range(3):
                    o, v_name, label = ds[i]
                    assert v_name == item_names[i] and o.shape == (10, 512, 4) and o.dtype == np.float64
                    out[f"seed{s}/item{i}"] = o.astype(np.float32)       # what the loop feeds the model (:227)
                    out[f"item{i}/label"] = np.int64(label)
                out[f"seed{s}/next_rand"] = np.float64(np.random.rand())
        finally:
            os.chdir(cwd)
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
