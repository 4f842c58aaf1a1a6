"""Prediction with a saved classifier (facl_amd/predict.py, csrc/predict.hip): the two kernels against numpy fp64 (every
64-lane stride boundary of the class loop, ragged row counts, padded rows), their tie / NaN / infinity rules, the `first` flag,
and the entry end to end on a tiny dataset -- against facl_amd.finetune's own test top-1, over several draws of the views,
with a ragged last batch, and on extracted features with a probe head.  The whole module runs on NaN-poisoned scratch."""
import os

import numpy as np
import pytest
import torch

from poison import poisoned_scratch  # noqa: F401
from synth_tree import clip_names, write_tree

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ULP = 2                 # top_p against fp64: the kernels work in fp64 and round once (tests/test_gpu_cls.py's convention)
GAP = 1e-6              # least relative distance of consecutive ranks in the fp64 reference of the random cases


# ---- numpy fp64 reference ----------------------------------------------------------------------------------------------------
def _softmax64(x):
    x = np.asarray(x, dtype=np.float64)
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def _order(acc_row):
    """classes under (value descending, class ascending)."""
    return np.lexsort((np.arange(len(acc_row)), -acc_row))


def _reference(acc, labels):
    """(order (R, ncls), rank (R,)) of an fp64 acc; rank -2 for a label outside the range."""
    order = np.stack([_order(r) for r in acc])
    rank = np.array([int(np.flatnonzero(order[i] == l)[0]) if 0 <= l < acc.shape[1] else -2 for i, l in enumerate(labels)])
    return order, rank


def _ulps(got, want64):
    want32 = np.asarray(want64, dtype=np.float64).astype(np.float32)
    return np.abs(got.astype(np.float64) - want64) / np.spacing(np.abs(want32)).astype(np.float64)


def _min_gap(acc):
    """per row, the least relative distance between consecutive ranks."""
    s = -np.sort(-acc, axis=1)
    return ((s[:, :-1] - s[:, 1:]) / s[:, :-1]).min(axis=1)


def _random_case(R, ncls, ndraws, seed):
    """`ndraws` (R, ncls) float32 logit matrices, random normal times 10 with the leading class of every row raised by 2, and
    the fp64 sum of their softmaxes.  A row in which two consecutive ranks of that sum lie closer than GAP (relative: the
    small probabilities of a 1000-class row are themselves far below any absolute figure) is drawn again, so the reference
    alone fixes the order; that is checked here, on the host."""
    logits = np.zeros((ndraws, R, ncls), dtype=np.float32)
    todo = np.arange(R)
    for attempt in range(64):
        r = np.random.RandomState([seed, attempt])
        x = (10.0 * r.randn(ndraws, len(todo), ncls)).astype(np.float32)
        lead = x.argmax(axis=2)
        for d in range(ndraws):
            x[d, np.arange(len(todo)), lead[d]] += 2.0
        logits[:, todo] = x
        acc = sum(_softmax64(logits[d]) for d in range(ndraws))
        todo = np.flatnonzero(~(_min_gap(acc) > GAP))
        if not len(todo):
            break
    assert (_min_gap(acc) > GAP).all()
    return logits, acc


def _run(logits, k, labels=None, ld_pad=0):
    """probs_acc over the draws, then topk; rows `ld_pad` floats wider than ncls hold NaN in the padding."""
    from facl_amd import cls_head
    acc = None
    for x in logits:
        t = torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
        if ld_pad:
            wide = torch.full((t.shape[0], t.shape[1] + ld_pad), float("nan"), device=DEV)
            wide[:, :t.shape[1]] = t
            t = wide[:, :t.shape[1]]
            assert t.stride(0) == x.shape[1] + ld_pad
        acc = cls_head.probs_acc(t, acc)
    y = None if labels is None else torch.from_numpy(np.asarray(labels, dtype=np.int32)).to(DEV)
    top_p, top_c, rank = cls_head.topk(acc, len(logits), k, y)
    torch.cuda.synchronize()
    return acc.cpu().numpy(), top_p.cpu().numpy(), top_c.cpu().numpy(), None if rank is None else rank.cpu().numpy()


# ---- 1. probabilities and top-k against numpy fp64 ------------------------------------------------------------------------------
@pytest.mark.parametrize("ncls", [2, 3, 60, 64, 65, 120, 1000, 1024])
def test_probs_and_topk_vs_fp64(ncls):
    worst = 0.0
    for R in (1, 5, 67):
        for ndraws in (1, 3):
            logits, acc64 = _random_case(R, ncls, ndraws, seed=1000 * ncls + 10 * R + ndraws)
            labels = np.random.RandomState(R + ncls).randint(0, ncls, R)
            order, rank64 = _reference(acc64, labels)
            for ld_pad in (0, 4):
                for k in sorted({1, min(5, ncls), min(ncls, 64)}):
                    acc, top_p, top_c, rank = _run(logits, k, labels, ld_pad)
                    tag = (R, ncls, ndraws, ld_pad, k)
                    assert np.array_equal(top_c, order[:, :k]), tag
                    assert np.array_equal(rank, rank64), tag
                    want = np.take_along_axis(acc64, order[:, :k], axis=1) / ndraws
                    u = float(_ulps(top_p, want).max())
                    worst = max(worst, u)
                    assert u <= ULP, (tag, u)
                    assert np.abs(acc - acc64).max() <= 1e-14 * ndraws, tag            # fp64 throughout: a few units of 2^-53
    print("[ncls %d] top_p worst %.2f fp32 ulp" % (ncls, worst))


# ---- 2. ties and extremes -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ncls,k", [(2, 2), (60, 5), (64, 64), (65, 7), (1000, 64)])
def test_all_equal_logits(ncls, k):
    R = 6
    labels = np.array([0, 1, ncls - 1, ncls // 2, 1, 0])
    for value in (0.0, -3.5, 1e4):
        _, top_p, top_c, rank = _run([np.full((R, ncls), value, dtype=np.float32)], k, labels)
        assert np.array_equal(top_c, np.tile(np.arange(k), (R, 1)))
        assert _ulps(top_p, np.full((R, k), 1.0 / ncls)).max() <= 1
        assert np.array_equal(rank, labels)


@pytest.mark.parametrize("ndraws", [1, 2])
def test_exact_duplicates_follow_the_total_order(ndraws):
    """Rows of small integers: equal logits give bit-equal probabilities (one draw, or the same draw twice), so the list is
    (logit descending, class ascending) exactly, over a stride boundary of the class loop."""
    R, ncls, k = 9, 70, 64
    x = np.random.RandomState(7).randint(0, 4, (R, ncls)).astype(np.float32)
    x[0, :] = 1.0
    x[1, 5], x[1, 69] = 3.0, 3.0
    labels = np.array([69, 69, 5, 0, 64, 63, 1, 2, 3])
    order = np.stack([np.lexsort((np.arange(ncls), -r)) for r in x])
    rank64 = np.array([int(np.flatnonzero(order[i] == l)[0]) for i, l in enumerate(labels)])
    _, top_p, top_c, rank = _run([x] * ndraws, k, labels)
    assert np.array_equal(top_c, order[:, :k]) and np.array_equal(rank, rank64)
    want = np.take_along_axis(_softmax64(x), order[:, :k], axis=1)
    assert _ulps(top_p, want).max() <= ULP
    assert (np.diff(top_p, axis=1) <= 0).all()


def test_extremes_nan_inf_and_bad_labels():
    ncls, k = 66, 6
    inf, nan = float("inf"), float("nan")
    x = np.random.RandomState(11).randn(8, ncls).astype(np.float32)
    x[1, :] = 0.0
    x[1, 0], x[1, 1] = 1e4, -1e4                              # +-1e4: exp(-2e4) is 0, nothing overflows
    x[2, :] = -inf
    x[2, [1, 3, 65]] = 2.0, 1.0, 0.0                          # -inf entries: p = 0, last, by class
    x[3, 64] = nan
    x[5, 2] = inf
    x[6, :] = -inf                                            # nothing but -inf: the maximum is not finite
    labels = np.array([3, 1, 0, 3, -1, 3, 3, ncls])
    acc, top_p, top_c, rank = _run([x], k, labels)
    clean = [0, 1, 2, 4, 7]
    acc64 = _softmax64(np.where(np.isfinite(x[clean]) | np.isneginf(x[clean]), x[clean], 0.0))
    order, rank64 = _reference(acc64, labels[clean])
    assert np.isfinite(acc[clean]).all() and np.abs(acc[clean] - acc64).max() <= 1e-14
    assert np.array_equal(top_c[clean], order[:, :k]) and np.array_equal(rank[clean], rank64)
    assert _ulps(top_p[clean], np.take_along_axis(acc64, order[:, :k], axis=1)).max() <= ULP
    assert top_c[1, 0] == 0 and top_p[1, 0] == 1.0 and np.array_equal(top_c[1, 1:], np.arange(1, k)) and (top_p[1, 1:] == 0).all()
    assert np.array_equal(top_c[2], [1, 3, 65, 0, 2, 4]) and (top_p[2, 3:] == 0).all() and (acc[2, [0, 2, 4]] == 0).all()
    assert rank[2] == 3 and rank[4] == -2 and rank[7] == -2
    for i in (3, 5, 6):                                       # a NaN, a +inf, only -inf: the whole row is NaN
        assert np.isnan(acc[i]).all() and np.isnan(top_p[i]).all() and (top_c[i] == -1).all() and rank[i] == -1, i
    # a NaN row stays NaN through a later draw, the rows beside it do not catch it; without labels there is no rank
    y = x.copy()
    y[[3, 5, 6]] = 0.0
    acc2, top_p2, top_c2, rank2 = _run([x, y], k)
    assert rank2 is None and np.isnan(acc2[[3, 5, 6]]).all() and np.isfinite(acc2[clean]).all()
    assert (top_c2[[3, 5, 6]] == -1).all() and np.array_equal(top_c2[clean], top_c[clean])
    # the same bits every run
    again = _run([x], k, labels)
    for a, b in zip((acc, top_p, top_c, rank), again):
        assert a.tobytes() == b.tobytes()


# ---- 3. the `first` flag ----------------------------------------------------------------------------------------------------------
def test_first_flag_overwrites_then_adds():
    from facl_amd import cls_head
    R, ncls = 7, 130
    r = np.random.RandomState(3)
    a, b = (3.0 * r.randn(R, ncls)).astype(np.float32), (3.0 * r.randn(R, ncls)).astype(np.float32)
    acc = torch.full((R, ncls), float("nan"), dtype=torch.float64, device=DEV)
    out = cls_head.probs_acc(torch.from_numpy(a).to(DEV), acc, first=True)
    assert out is acc
    single = cls_head.probs_acc(torch.from_numpy(a).to(DEV))
    assert torch.equal(acc, single) and np.abs(acc.cpu().numpy() - _softmax64(a)).max() <= 1e-14
    cls_head.probs_acc(torch.from_numpy(b).to(DEV), acc)
    assert np.abs(acc.cpu().numpy() - (_softmax64(a) + _softmax64(b))).max() <= 2e-14
    # into a slice of a larger tensor (what Classifier.predict does): the rows beside it keep their contents
    big = torch.full((R + 4, ncls), 5.0, dtype=torch.float64, device=DEV)
    cls_head.probs_acc(torch.from_numpy(a).to(DEV), big[2:2 + R], first=True)
    assert torch.equal(big[2:2 + R], single) and (big[:2] == 5.0).all() and (big[2 + R:] == 5.0).all()


# ---- the entry on a tiny dataset ---------------------------------------------------------------------------------------------
VIEW_ARGS = ["--num_crop", "10", "--SAMPLE_NUM", "512", "--INPUT_FEATURE_NUM", "4"]


@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    """The tree, and finetune.main's two epochs on it: (data root, checkpoint folder, finetune's returned test top-1)."""
    from facl_amd import finetune
    root = tmp_path_factory.mktemp("predict")
    d, ck = str(root / "d"), str(root / "ck")
    write_tree(d)
    top1 = finetune.main(["--synthetic", "0", "--data_root", d, "--dataset", "ntu120", "--batchSize", "4", "--nepoch", "2",
                          "--save_root_dir", ck, "--eval_every", "1", "--label_fraction", "0.5", "--num_class", "4"] + VIEW_ARGS)
    return d, ck, top1


def _predict_args(d, ck, *more):
    return ["--data_root", d, "--dataset", "ntu120", "--batchSize", "4", "--encoder", os.path.join(ck, "finetune_enc_1.pth"),
            "--head", os.path.join(ck, "finetune_fc_1.pth")] + VIEW_ARGS + list(more)


def _test_names():
    return sorted(nm for i, nm in enumerate(clip_names(24)) if i % 3 == 2)


def test_entry_equals_finetune_top1(trained, tmp_path, capsys):
    from facl_amd import predict
    d, ck, ft_top1 = trained
    capsys.readouterr()
    outs = [str(tmp_path / "a"), str(tmp_path / "b")]
    res = predict.main(_predict_args(d, ck, "--draws", "1", "--topk", "3", "--out", outs[0]))
    text = capsys.readouterr().out
    assert isinstance(ft_top1, float) and res["top1"] == ft_top1, (res, ft_top1)
    assert "top1: %s\n" % ft_top1 in text and "top3: %s\n" % res["topk"] in text
    assert "mean class accuracy: %s\n" % res["mean_class_accuracy"] in text
    assert res["clips"] == 8 and res["k"] == 3 and res["topk"] >= res["top1"]
    z = np.load(os.path.join(outs[0], "predictions.npz"))
    assert sorted(z.files) == ["labels", "names", "rank", "top_c", "top_p"]
    names = _test_names()
    assert z["names"].tolist() == names and z["labels"].tolist() == [int(n[-3:]) - 1 for n in names]
    assert z["top_c"].shape == (8, 3) and z["top_c"].dtype == np.int32 and z["top_p"].dtype == np.float32
    assert np.array_equal(z["rank"] == 0, z["top_c"][:, 0] == z["labels"])
    assert (np.diff(z["top_p"], axis=1) <= 0).all() and (z["top_p"] > 0).all()
    hits = int((z["rank"] == 0).sum())
    assert res["top1"] == 100.0 * hits / 8
    conf = np.load(os.path.join(outs[0], "confusion.npy"))
    assert conf.shape == (4, 4) and conf.dtype == np.int64 and conf.sum() == 8 and np.trace(conf) == hits
    assert np.array_equal(conf.sum(axis=1), np.bincount(z["labels"], minlength=4))
    # a second run writes identical files
    assert predict.main(_predict_args(d, ck, "--draws", "1", "--topk", "3", "--out", outs[1])) == res
    for f in ("predictions.npz", "confusion.npy"):
        assert open(os.path.join(outs[0], f), "rb").read() == open(os.path.join(outs[1], f), "rb").read(), f
    # every class listed: the probabilities of a clip sum to 1, and the leading three are the ones above
    out4 = str(tmp_path / "k4")
    capsys.readouterr()
    res4 = predict.main(_predict_args(d, ck, "--topk", "4", "--out", out4, "--no_labels"))
    assert res4 == {"clips": 8} and not os.path.exists(os.path.join(out4, "confusion.npy"))
    text = capsys.readouterr().out
    assert "top1:" not in text and "mean class accuracy" not in text
    z4 = np.load(os.path.join(out4, "predictions.npz"))
    assert sorted(z4.files) == ["names", "top_c", "top_p"] and z4["names"].tolist() == names
    assert np.abs(z4["top_p"].astype(np.float64).sum(axis=1) - 1.0).max() <= 1e-6
    assert np.array_equal(z4["top_c"][:, :3], z["top_c"]) and np.array_equal(z4["top_p"][:, :3], z["top_p"])
    assert np.array_equal(np.sort(z4["top_c"], axis=1), np.tile(np.arange(4), (8, 1)))


def test_draws(trained, tmp_path):
    from facl_amd import dataset as fds
    from facl_amd import predict
    d, ck, _ = trained
    philox = ["--view_rng", "philox", "--topk", "4"]
    o1, o3 = str(tmp_path / "d1"), str(tmp_path / "d3")
    predict.main(_predict_args(d, ck, "--draws", "1", "--out", o1, *philox))
    predict.main(_predict_args(d, ck, "--draws", "3", "--out", o3, *philox))
    z1, z3 = np.load(os.path.join(o1, "predictions.npz")), np.load(os.path.join(o3, "predictions.npz"))
    assert z1["names"].tolist() == z3["names"].tolist() and z3["top_p"].shape == (8, 4)
    assert not np.array_equal(z1["top_p"], z3["top_p"])
    assert np.abs(z3["top_p"].astype(np.float64).sum(axis=1) - 1.0).max() <= 1e-6
    # two draws through the class: the mean of the fp64 softmaxes of the two passes' logits
    opt = predict.predict_parser().parse_args(_predict_args(d, ck, *philox))
    predict.check_predict_flags(opt)
    load = lambda p: torch.load(p, map_location="cpu", weights_only=True)
    clf = predict.Classifier(load(opt.head), opt, load(opt.encoder)).to(DEV)
    assert (clf.num_class, clf.views) == (4, 10) and not clf.encoder.training
    index = fds.ClipIndex.from_dir(os.path.join(d, fds.EXTRACT_LIST_DIR), "ntu120")
    split = index.select("view", test=True)
    source = predict.ViewSource(opt, torch.device(DEV), index, split)
    res = clf.predict(source, draws=2, k=4)
    passes = []
    for r in range(2):
        lg = torch.cat([clf.logits_of_views(v, B) for v, B in predict.ViewSource(opt, torch.device(DEV), index, split).batches(r)])
        assert lg.shape == (8, 4)
        passes.append(_softmax64(lg.cpu().numpy()))
    assert not np.array_equal(passes[0], passes[1])
    mean = (passes[0] + passes[1]) / 2
    assert _ulps(res["top_p"], np.take_along_axis(mean, res["top_c"].astype(np.int64), axis=1)).max() <= ULP
    order, rank64 = _reference(mean, source.labels)
    assert np.array_equal(res["rank"], rank64) and np.array_equal(res["top_c"], order)
    # one draw through the class is the entry's --draws 1
    one = clf.predict(predict.ViewSource(opt, torch.device(DEV), index, split), draws=1, k=4)
    assert np.array_equal(one["top_p"], z1["top_p"]) and np.array_equal(one["top_c"], z1["top_c"])


def test_ragged_last_batch(trained, tmp_path):
    """8 test clips in batches of 3 (3 + 3 + 2) and of 4: the same probabilities within 1e-5 (the bound tests/test_gpu_cls.py
    holds the head's logits to against fp64; a probability is at most 1), and the same leading class on every clip whose
    top-1 / top-2 margin exceeds 4e-5 -- which must be all eight.  Measured on the MI355X with this tree: the closest clip
    had a margin of 1.630e-3 (the eight lie in 1.630e-3 .. 1.638e-3), and the two batch sizes gave the same bits."""
    from facl_amd import predict
    d, ck, _ = trained
    z = {}
    for B in ("3", "4"):
        args = _predict_args(d, ck, "--topk", "4", "--out", str(tmp_path / B))
        args[args.index("--batchSize") + 1] = B
        predict.main(args)
        z[B] = np.load(os.path.join(str(tmp_path / B), "predictions.npz"))
    assert z["3"]["names"].tolist() == z["4"]["names"].tolist()
    p = {}
    for B in z:                                               # probabilities by class, not by list position
        p[B] = np.zeros((8, 4))
        np.put_along_axis(p[B], z[B]["top_c"].astype(np.int64), z[B]["top_p"].astype(np.float64), axis=1)
    diff = np.abs(p["3"] - p["4"]).max()
    margin = np.minimum(*(z[B]["top_p"][:, 0].astype(np.float64) - z[B]["top_p"][:, 1] for B in z))
    print("ragged: max |p3 - p4| %.3e, top-1 / top-2 margins %s" % (diff, " ".join("%.3e" % v for v in margin)))
    assert diff <= 1e-5
    assert (margin > 4e-5).all(), margin
    assert np.array_equal(z["3"]["top_c"][:, 0], z["4"]["top_c"][:, 0])
    assert np.array_equal(z["3"]["rank"] == 0, z["4"]["rank"] == 0)


# ---- the probe path --------------------------------------------------------------------------------------------------------------
def test_probe_path(trained, tmp_path, capsys):
    from facl_amd import linear_classify, predict
    d = trained[0]
    width = 11 * 512
    r = np.random.RandomState(21)
    folders = {}
    for stream in ("motion", "app"):
        folders[stream] = str(tmp_path / stream)
        os.makedirs(folders[stream])
        means = r.randn(4, width)
        for n in sorted(os.listdir(os.path.join(d, "raw"))):
            n = n[:20]
            np.save(os.path.join(folders[stream], n + ".npy"), (means[int(n[-3:]) - 1] + 0.1 * r.randn(width)).astype(np.float32))
    fc = str(tmp_path / "probe_fc.pth")
    common = ["--data_root", d, "--dataset", "ntu120", "--batchSize", "8", "--motion_feature_dir", folders["motion"],
              "--appearance_feature_dir", folders["app"]]
    capsys.readouterr()
    probe_top1 = linear_classify.main(common + ["--nepoch", "18", "--num_class", "4", "--save_fc", fc])
    text = capsys.readouterr().out
    assert "epoch: 17 test top1: %s\n" % probe_top1 in text
    sd = torch.load(fc, map_location="cpu", weights_only=True)
    linear_classify.Final_FC(input_dim=512, gost=22, num_class=4).load_state_dict(sd, strict=True)
    out = str(tmp_path / "out")
    res = predict.main(common + ["--head", fc, "--topk", "2", "--out", out])
    assert res["top1"] == probe_top1 and res["clips"] == 8 and res["topk"] >= res["top1"]
    assert "top1: %s\n" % probe_top1 in capsys.readouterr().out
    z = np.load(os.path.join(out, "predictions.npz"))
    assert z["names"].tolist() == _test_names() and z["top_c"].shape == (8, 2)
    assert np.array_equal(z["rank"] == 0, z["top_c"][:, 0] == z["labels"])
    conf = np.load(os.path.join(out, "confusion.npy"))
    assert conf.sum() == 8 and 100.0 * np.trace(conf) / 8 == probe_top1
    with pytest.raises(RuntimeError, match="--draws 2 needs --encoder"):
        predict.main(common + ["--head", fc, "--draws", "2"])
    # one stream alone does not fit the two-stream head
    with pytest.raises(RuntimeError, match="the head reads vectors of 11264 floats, the feature folders give 5632"):
        predict.main(common[:-2] + ["--head", fc, "--topk", "2"])
