"""CPU tests of the seams of the shared training loop (facl_amd/train_common.py): the batch source, capture-or-eager, the
non-finite-loss stop and the launcher's world size.  Fakes only: no device, no file."""
from types import SimpleNamespace

import numpy as np
import pytest

TOO_FEW = "my wording: %(clips)d clips, batches of %(batch)d, %(world)d ranks"


class _Index:
    def __init__(self, n):
        self.n = n

    def select(self, mode, full_train=True):
        assert (mode, full_train) == ("view", True)
        return [100 + 3 * i for i in range(self.n)]              # dataset indices are not positions


class _Disk:
    made = []

    def __init__(self, index, root, branch, vids, mode, device, **kw):
        self.vids, self.kw, self.hold_first = vids, kw, False
        _Disk.made.append(self)

    def __iter__(self):
        return iter(self.vids)


def _source(monkeypatch, clips, B, world, rank, cap, **kw):
    from facl_amd import dataset as fds
    from facl_amd.train_common import TrainBatches
    monkeypatch.setattr(fds.ClipIndex, "from_dir", classmethod(lambda cls, path, dataset: _Index(clips)))
    monkeypatch.setattr(fds, "DiskBatches", _Disk)
    opt = SimpleNamespace(data_root="root", branch_choose="0", dataset="ntu60", split="view", full_train=1, batchSize=B,
                          max_steps_per_epoch=cap, resident=0, manualSeed=1, view_rng="philox", prefetch=0, num_crop=10,
                          SAMPLE_NUM=512)
    return TrainBatches(opt, None, rank, world, TOO_FEW, **kw)


@pytest.mark.parametrize("clips,B,world,cap", [(16, 4, 1, 0), (16, 4, 2, 0), (17, 4, 1, 3)])
def test_batch_source_steps_and_positions(monkeypatch, clips, B, world, cap):
    from facl_amd.dataset import train_batches
    steps = clips // (B * world)
    steps = min(steps, cap) if cap else steps
    for rank in range(world):
        src = _source(monkeypatch, clips, B, world, rank, cap)
        assert src.steps == steps
        for epoch in (0, 1, 5):
            for hold in (False, True):
                _Disk.made.clear()
                got = list(src.epoch(epoch, hold_first=hold))
                disk, = _Disk.made
                want = train_batches(clips, B, world, rank, 1, epoch)[:steps]
                assert len(got) == steps
                np.testing.assert_array_equal(np.stack(got), 100 + 3 * want)
                assert disk.hold_first is hold
                assert (disk.kw["seed"], disk.kw["epoch"], disk.kw["num_crop"], disk.kw["num_point"]) == (2000, epoch, 10, 512)
                assert disk.kw["rng"] is src.view_rng


@pytest.mark.parametrize("clips,B,world", [(3, 4, 1), (7, 4, 2)])
def test_batch_source_refuses_less_than_one_batch(monkeypatch, clips, B, world):
    with pytest.raises(RuntimeError) as e:
        _source(monkeypatch, clips, B, world, 0, 0)
    assert str(e.value) == "my wording: %d clips, batches of %d, %d ranks" % (clips, B, world)


def test_batch_source_subset_narrows_the_split(monkeypatch):
    src = _source(monkeypatch, 16, 4, 1, 0, 0, subset=lambda index, split: split[::2])
    assert src.steps == 2 and list(src.split) == [100 + 6 * i for i in range(8)]
    with pytest.raises(RuntimeError, match="my wording: 2 clips"):
        _source(monkeypatch, 16, 4, 1, 0, 0, subset=lambda index, split: split[:2])


def _graph_opt(graph=1, swa_if=0, cld_if=0):
    return SimpleNamespace(graph=graph, swa_if=swa_if, cld_if=cld_if)


@pytest.mark.parametrize("flags", [dict(graph=0), dict(swa_if=1), dict(cld_if=1)])
def test_capture_or_eager_stays_eager_without_constructing_a_graph(monkeypatch, flags):
    import facl_amd.train_common as tc

    def never(*a, **k):
        raise AssertionError("a graph was constructed")
    monkeypatch.setattr(tc, "GraphedStep", never)
    step, opt = SimpleNamespace(G=3), _graph_opt(**flags)
    assert tc.capture_or_eager(step, "points", opt) is step
    assert opt.graph == flags.get("graph", 1)


def test_capture_or_eager_captures_falls_back_and_propagates(monkeypatch, capsys):
    import facl_amd.train_common as tc
    step, opt, calls = SimpleNamespace(G=3), _graph_opt(), []

    def graphed(*a, **k):
        calls.append((a, k))
        return "graphed"
    monkeypatch.setattr(tc, "GraphedStep", graphed)
    assert tc.capture_or_eager(step, "points", opt) == "graphed"
    assert calls == [((step, "points", 3), dict(restore=True))] and opt.graph == 1

    def failing(*a, **k):
        raise tc.GraphCaptureFailed("no luck")
    monkeypatch.setattr(tc, "GraphedStep", failing)
    capsys.readouterr()
    assert tc.capture_or_eager(step, "points", opt) is step
    assert capsys.readouterr().out == "graph capture failed (no luck); running eager\n"
    assert opt.graph == 0

    def broken(*a, **k):
        raise ValueError("something else")
    monkeypatch.setattr(tc, "GraphedStep", broken)
    opt = _graph_opt()
    with pytest.raises(ValueError, match="something else"):
        tc.capture_or_eager(step, "points", opt)
    assert opt.graph == 1


@pytest.mark.parametrize("lv,shown", [(float("nan"), "nan"), (float("inf"), "inf"), (float("-inf"), "-inf")])
def test_non_finite_loss_stops(lv, shown):
    from facl_amd.train_common import check_finite_loss
    with pytest.raises(FloatingPointError) as e:
        check_finite_loss(lv, 3, 7)
    assert str(e.value) == "non-finite loss %s at epoch 3, iteration 7" % shown
    assert check_finite_loss(1.25, 0, 0) is None and check_finite_loss(-3e38, 0, 0) is None


@pytest.mark.parametrize("value,world", [(None, 1), ("1", 1), ("2", 2)])
def test_world_size_reader(monkeypatch, value, world):
    from facl_amd import dist as fdist
    from facl_amd.finetune import check_finetune_flags, finetune_parser
    from facl_amd.train_common import build_parser, check_knn_flags
    if value is None:
        monkeypatch.delenv("WORLD_SIZE", raising=False)
    else:
        monkeypatch.setenv("WORLD_SIZE", value)
    assert fdist.env_world_size() == world
    knn, ft = build_parser('0').parse_args(["--synthetic", "0", "--knn_every", "1"]), finetune_parser().parse_args([])
    if world == 1:                                               # the two flag checks read the same value
        check_knn_flags(knn)
        check_finetune_flags(ft)
    else:
        with pytest.raises(RuntimeError, match="one rank only \\(got 2 ranks\\)"):
            check_knn_flags(knn)
        with pytest.raises(RuntimeError, match="one rank only \\(got 2 ranks\\)"):
            check_finetune_flags(ft)
