#!/usr/bin/env python
"""Generate tests/golden/c1_d8.npz: the first-configuration fixture of tools/make_goldens.py (`run_c1`: the reference's own
group_points_3DV, PointNet_Plus_fine, both losses and three Adam steps) at INPUT_FEATURE_NUM = 8, xyz plus five feature
channels.  Like make_goldens.py it runs only where the reference is importable; the tests only read the .npz.

run_c1 fixes its own sizes, and at D = 8 its file (2.2 MB) is over the 1 MiB limit of a committed file.  The 8-channel
points themselves are incompressible, so what the D = 8 tests (tests/test_feature_dims_cpu.py, tests/test_gpu_feature_dims.py)
do not read is dropped and the file is saved again: the stage taps (pooled features, x_pre) and the normalised features that
the D = 3 / 4 fixtures already pin, the full gradients of the tensors over 4096 elements (their norms stay), one of the five
post-Adam tensors, and all but the first two groups of xt_first8 (xt_sum still covers every group).

    python tools/make_golden_d8.py           # rewrites tests/golden/c1_d8.npz
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_goldens import OUT, run_c1                        # noqa: E402

DROP = ("train_pooled", "train_x_pre", "eval_x_nor", "train_x_nor", "param3/net3DV_1.6.weight")


def main():
    import torch
    torch.set_num_threads(8)
    run_c1(8, False, "d8")
    path = os.path.join(OUT, "c1_d8.npz")
    with np.load(path) as z:
        kept = {k: z[k] for k in z.files if k not in DROP and not (k.startswith("grad/") and z[k].size > 4096)}
        kept["xt_first8"] = kept["xt_first8"][:2]
    np.savez_compressed(path, **kept)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
