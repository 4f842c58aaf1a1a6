#!/usr/bin/env python
"""Generate tests/golden/view_kinds.npz by running the REFERENCE's own transforms on CPU (the pattern of tools/make_goldens.py).

The view kinds `jitter`, `scale`, `tilt_neg` and `tilt_pos` of a view recipe (facl_amd/philox.py: Recipe) are transforms the
reference's dataset class defines and never wires into its loader.  This script imports training_code/cn3D_data_set.py (with an
empty stand-in for its unused `import imageio`), calls `jitter_point_cloud`, `scale_trans` and `depth_transform(., -1 / +1)` of
`NTU_RGBD_new` UNBOUND -- they use no instance state -- on a synthetic cloud in float32 and float64 with NumPy's generator
seeded, and records the inputs, the drawn factor / noise (re-drawn from the same seed) and the outputs.  Nothing of the
reference is copied: data only.

    python tools/make_view_kind_goldens.py --reference <the reference's checkout>      # rewrites tests/golden/view_kinds.npz
"""
import argparse
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "tests", "golden", "view_kinds.npz")
ROWS = 64
JITTERS = (("default", 21, {}), ("strong", 22, dict(sigma=0.02, clip=0.03)))
SCALE_SEEDS = (31, 32, 33)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reference", default=os.environ.get("FACL_REFERENCE_DIR", ""), help="the reference's checkout")
    opt = ap.parse_args()
    if not opt.reference:
        ap.error("--reference (or FACL_REFERENCE_DIR) is required")
    sys.path.insert(0, os.path.join(opt.reference, "training_code"))
    sys.modules.setdefault("imageio", types.ModuleType("imageio"))
    import cn3D_data_set as R_data                                  # reference
    from helpers import synth_clip
    cls = R_data.NTU_RGBD_new
    out = {"scale_seeds": np.array(SCALE_SEEDS, dtype=np.int32)}
    for dt in (np.float32, np.float64):
        tag = np.dtype(dt).name
        pts = synth_clip(6, dt)[0][:ROWS, :4].reshape(1, ROWS, 4).copy()
        keep = pts.copy()
        out["%s/in" % tag] = pts
        for name, seed, kw in JITTERS:
            np.random.seed(seed)
            o = cls.jitter_point_cloud(None, pts[:, :, 0:3], **kw)
            np.random.seed(seed)
            out["%s/jitter_%s_noise" % (tag, name)] = np.random.randn(1, ROWS, 3)
            out["%s/jitter_%s_out" % (tag, name)] = o
            out["%s/jitter_%s_strengths" % (tag, name)] = np.array([kw.get("sigma", 0.01), kw.get("clip", 0.05)])
        for seed in SCALE_SEEDS:
            np.random.seed(seed)
            o = cls.scale_trans(None, pts)
            np.random.seed(seed)
            out["%s/scale_%d_factor" % (tag, seed)] = np.float64(np.random.rand() + 0.5)
            assert o.dtype == dt
            out["%s/scale_%d_out" % (tag, seed)] = o
        for name, sign in (("tilt_neg", -1), ("tilt_pos", 1)):
            o = cls.depth_transform(None, pts, sign)
            assert o.dtype == np.float32
            out["%s/%s_out" % (tag, name)] = o
        assert np.array_equal(pts, keep)                            # the inputs are untouched
    np.savez_compressed(OUT, **out)
    print(OUT, {k: np.shape(v) for k, v in out.items()}, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
