"""Starting the ranks of a multi-process test and ending them, whatever happens.

A worker is a top-level function of its test module (spawn pickles it by module name) with the signature
`worker(rank, world, port, q, *args)`.  It calls `rank_env` first, posts exactly one result with `q.put(result)` and then
leaves its process group."""
import multiprocessing
import os
import queue
import sys
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rank_env(rank, world, port, **extra):
    """The worker preamble: the repository on sys.path and the rendezvous of torch.distributed in the environment."""
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), **extra)


class _RankQueue:
    """What a worker gets as `q`: its result travels with its rank, so the parent knows who has posted."""

    def __init__(self, q, rank):
        self.q, self.rank = q, rank

    def put(self, item):
        self.q.put((self.rank, item))


def _stop(procs):
    """Terminate, then kill, whatever is still alive; join everything."""
    for p in procs:
        if p.is_alive():
            p.terminate()
    for p in procs:
        p.join(timeout=5)
    for p in procs:
        if p.is_alive():
            p.kill()
    for p in procs:
        p.join()


def run_ranks(target, world, port, args=(), timeout=300, check_exit=False):
    """Start `world` ranks of `target` once and return their results in rank order.

    A rank that exits with a non-zero status before it has posted, or `timeout` seconds without all results, ends the
    run: every rank still alive is terminated, then killed, all are joined, and the test fails with the exit codes.
    Nothing is started a second time.  `check_exit`: the ranks must also have exited with status 0 after posting."""
    ctx = multiprocessing.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=target, args=(r, world, port, _RankQueue(q, r)) + tuple(args)) for r in range(world)]
    for p in procs:
        p.start()
    results, why = {}, None
    deadline = time.monotonic() + timeout

    def drain(wait):
        try:
            while True:
                rank, item = q.get(timeout=wait)
                results[rank] = item
                wait = 0.05
        except queue.Empty:
            pass

    while len(results) < world:
        drain(0.2)
        dead = [r for r, p in enumerate(procs) if r not in results and p.exitcode not in (None, 0)]
        if dead:
            drain(0.5)                                         # a result posted just before the exit may still be in flight
            dead = [r for r in dead if r not in results]
        if dead:
            why = "rank %s exited before posting a result" % ", ".join(str(r) for r in dead)
        elif time.monotonic() > deadline and len(results) < world:
            why = "no result from rank %s after %g s" % (", ".join(str(r) for r in range(world) if r not in results), timeout)
        if why:
            codes = [p.exitcode for p in procs]                # before the clean-up: None = was still running
            _stop(procs)
            pytest.fail("%s; exit codes by rank %s (None: still running, stopped here)" % (why, codes), pytrace=False)
    for p in procs:
        p.join(timeout=60)
    _stop(procs)
    if check_exit:
        assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    return [results[r] for r in range(world)]
