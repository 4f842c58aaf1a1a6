"""The support modules of the suite, on the CPU: synth_tree.write_tree writes the trees the test modules' own builders wrote
before they were folded into it, step_factory.step_opt is the namespace they spelled out, and ranks.run_ranks ends its
children whatever they do.

tests/golden/support_digests.json was recorded by running the builders it names (`call`), as they stood in the commit before
the shared writer existed, into empty directories and taking `tree_digest` of each; nothing in it comes from write_tree."""
import functools
import hashlib
import json
import multiprocessing
import os
import sys
import time

import numpy as np
import pytest

from helpers import GOLDEN
from ranks import run_ranks
from synth_tree import tree_clip, write_tree


def tree_digest(root):
    """SHA-256 over the sorted relative paths under `root` (directories, empty ones included, and files) and the file bytes."""
    root = str(root)
    entries = []
    for d, dirs, files in os.walk(root):
        rel = os.path.relpath(d, root)
        if rel != ".":
            entries.append((rel.replace(os.sep, "/") + "/", None))
        entries += [(os.path.relpath(os.path.join(d, f), root).replace(os.sep, "/"), os.path.join(d, f)) for f in files]
    h = hashlib.sha256()
    for rel, path in sorted(entries):
        h.update(rel.encode() + b"\0")
        if path is not None:
            with open(path, "rb") as f:
                data = f.read()
            h.update(b"%d\0" % len(data) + data)
    return h.hexdigest()


# ---- 1: the tree is the old tree ----------------------------------------------------------------------------------------------
_resident = functools.partial(write_tree, scale=1, listed=("res10",))          # as test_gpu_resident.py binds it
_clip = functools.partial(tree_clip, R1=500, R2=200)                           # its default cloud sizes (P by keyword or position)
TREES = {
    "finetune": lambda r: write_tree(r),
    "knn_entries": lambda r: write_tree(r),
    "dataset_24": lambda r: write_tree(r, n=24, listed=("raw", "res10")),
    "dataset_27": lambda r: write_tree(r, n=27, listed=("raw", "res10")),
    "resident_f64": lambda r: _resident(r, dt=np.float64),
    "resident_f32": lambda r: _resident(r, dt=np.float32),
    "resident_scale4": lambda r: _resident(r, scale=4),
    "resident_clips": lambda r: _resident(r, n=6, clips={0: _clip(3, 1), 1: _clip(3, 5000), 3: tree_clip(4, 2, 1, 1, 1)}),
}


@pytest.mark.parametrize("case", sorted(TREES))
def test_shared_writer_writes_the_old_tree(tmp_path, case):
    with open(os.path.join(GOLDEN, "support_digests.json")) as f:
        recorded = json.load(f)
    assert sorted(recorded) == sorted(TREES)
    names = TREES[case](str(tmp_path))
    assert len(names) == len(set(names)) > 0
    assert tree_digest(tmp_path) == recorded[case]["sha256"], recorded[case]["call"]


# ---- 2: the namespace is the old namespace -------------------------------------------------------------------------------------
def test_step_opt_is_the_old_namespace():
    from step_factory import step_opt
    old = {"temperal_num": 3, "knn_K": 64, "ball_radius": 0.16, "ball_radius2": 0.25, "sample_num_level1": 64,
           "sample_num_level2": 64, "INPUT_FEATURE_NUM": 4, "Num_Class": 512, "batchSize": 3, "pooling": "concatenation",
           "SAMPLE_NUM": 512}
    assert vars(step_opt(4, 3, 512)) == old
    assert list(vars(step_opt(4, 3, 512))) == list(old)
    assert vars(step_opt(4, 3, 512, loss_mask="exclude")) == dict(old, loss_mask="exclude")


# ---- 3: the launcher ends trouble ----------------------------------------------------------------------------------------------
def _posts(rank, world, port, q, tag):
    q.put((tag, rank, world, port))


def _one_dies(rank, world, port, q):
    if rank == 1:
        sys.exit(3)
    time.sleep(60)


def _sleeps(rank, world, port, q):
    time.sleep(60)


def test_run_ranks_returns_results_in_rank_order():
    assert run_ranks(_posts, 2, 4711, args=("x",), timeout=60, check_exit=True) == [("x", 0, 2, 4711), ("x", 1, 2, 4711)]
    assert multiprocessing.active_children() == []


def test_run_ranks_ends_the_others_when_a_rank_dies_before_posting():
    t0 = time.monotonic()
    with pytest.raises(pytest.fail.Exception, match=r"rank 1 exited before posting.*\[None, 3\]"):
        run_ranks(_one_dies, 2, 4711, timeout=20)
    assert time.monotonic() - t0 < 10
    assert multiprocessing.active_children() == []


def test_run_ranks_ends_everything_at_the_timeout():
    t0 = time.monotonic()
    with pytest.raises(pytest.fail.Exception, match=r"no result from rank 0, 1 after 2 s.*\[None, None\]"):
        run_ranks(_sleeps, 2, 4711, timeout=2)
    assert 2 <= time.monotonic() - t0 < 10
    assert multiprocessing.active_children() == []
