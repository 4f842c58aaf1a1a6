"""GraphedStep over a step class that is not ContrastiveStep: facl_amd.dense.DenseStep (bench.py --config dense) has no
``queue`` attribute, and its iteration must still be captured and replayed as one HIP graph instead of dropping to eager
launches behind a line on stderr."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def test_dense_bench_step_is_captured_and_restores_its_state(capfd):
    """The benchmark's hook at a small size (2 clips x 4 views x 1024 points, the model's own level sizes): the launch mode is
    "hipgraph" and nothing was reported on stderr; a replay gives a finite loss.  Then GraphedStep(restore=True) over the same
    DenseStep: parameters and running statistics are bit for bit what they were before the three warm-up steps, and the first
    replayed step equals the eager step from that state."""
    from facl_amd import dense
    from facl_amd.train_common import GraphedStep
    a = SimpleNamespace(B=2, T=4, N=1024, D=3, graph=1)
    torch.manual_seed(3)
    run_step, step, batches, mode, _, _, _ = dense.make_bench_step(a, torch.device(DEV), 0, 1)
    assert not hasattr(step, "queue")
    assert mode == "hipgraph" and isinstance(run_step, GraphedStep), capfd.readouterr().err
    assert "graph capture failed" not in capfd.readouterr().err
    order = np.array([2, 0, 3, 1])
    assert torch.isfinite(run_step(batches[1], order=order)[0])
    del run_step
    before = {k: v.detach().clone() for k, v in step.netR.state_dict().items()}
    g = GraphedStep(step, batches[0], a.T, restore=True)
    for k, v in step.netR.state_dict().items():
        assert torch.equal(v, before[k]), k
    snap = g._snapshot()
    assert snap[3] is None
    loss_g = g(batches[1], order=order)[0].detach().clone()
    g._restore(snap)
    loss_e = step(batches[1], order=order)[0].detach()
    print("dense step: graph-replayed loss %.9g, eager loss %.9g" % (float(loss_g), float(loss_e)))
    assert torch.isfinite(loss_g) and torch.equal(loss_g, loss_e)
