"""The small fp64 kernels between the heavy BatchNorm passes (csrc/finalize.hip, the finalize / constants kernels of
csrc/fchead.hip, the helpers of csrc/bn_consts.h) against tests/golden/bn_glue_parent.npz: the outputs of the same calls as
recorded on the MI355X from the build before these kernels were folded onto shared helpers
(tools/make_bn_glue_goldens.py).  The rule: NaN at the same positions, every other element equal as raw bits."""
import json

import numpy as np
import pytest

from helpers import load_golden

pytestmark = pytest.mark.gpu

GROUP_NAMES = ["finalize", "eval_consts", "bn1", "bwd_consts", "sa_consts", "sa_final", "fc_head", "amax"]
_FLOAT_OF = {4: np.float32, 8: np.float64}


@pytest.fixture(scope="module")
def golden():
    g = load_golden("bn_glue_parent.npz")
    aliases = json.loads(str(g.pop("aliases")))
    keys = list(g) + list(aliases)
    return {k: g[aliases.get(k, k)] for k in keys}


def same_bits(got, want):
    """NaN positions equal, every other element equal as raw bits (amax words are float bits: judged as floats)"""
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    f, w = got.view(_FLOAT_OF[got.dtype.itemsize]), want.view(_FLOAT_OF[want.dtype.itemsize])
    nf, nw = np.isnan(f), np.isnan(w)
    bits = np.uint32 if got.dtype.itemsize == 4 else np.uint64
    return bool(np.array_equal(nf, nw) and np.array_equal(f.view(bits)[~nf], w.view(bits)[~nw]))


def test_cases_cover_the_groups():
    import bn_glue_cases
    assert list(bn_glue_cases.GROUPS) == GROUP_NAMES


@pytest.mark.parametrize("group", GROUP_NAMES)
def test_outputs_equal_the_parent_build_bitwise(group, golden):
    import bn_glue_cases
    got = bn_glue_cases.run_group(group)
    want = {k for k in golden if k.startswith(group + "/")}
    assert got and set(got) == want
    bad = [k for k in sorted(got) if not same_bits(got[k], golden[k])]
    assert not bad, bad
