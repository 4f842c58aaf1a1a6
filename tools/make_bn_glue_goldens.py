#!/usr/bin/env python
"""Record tests/golden/bn_glue_parent.npz: every output of the cases in tests/bn_glue_cases.py (the small fp64 kernels between
the heavy BatchNorm passes), as computed on the GPU by the library that is loaded.  Run it on the build whose bits are the
contract -- the commit BEFORE a change to csrc/finalize.hip, csrc/fchead.hip or the constants helpers they share (FACL_LIB
selects another build of the same ABI) -- and commit the file with the change; tests/test_gpu_bn_glue.py then holds the new
build to those bits.

An output that is bit-identical to one already stored (dW3 and dW2 do not depend on D) is stored once: `aliases` maps its key
to the stored one.

    python tools/make_bn_glue_goldens.py            # rewrites tests/golden/bn_glue_parent.npz
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import bn_glue_cases                                        # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "bn_glue_parent.npz")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    out, aliases, seen = {}, {}, {}
    for group in bn_glue_cases.GROUPS:
        for key, a in bn_glue_cases.run_group(group).items():
            sig = (a.dtype.str, a.shape, a.tobytes())
            if sig in seen:
                aliases[key] = seen[sig]
            else:
                seen[sig] = key
                out[key] = a
    out["aliases"] = np.array(json.dumps(aliases))
    np.savez_compressed(args.out, **out)
    print(args.out, os.path.getsize(args.out), "bytes,", len(out) - 1, "arrays,", len(aliases), "aliases")


if __name__ == "__main__":
    main()
