"""What the torch fp64 reference does with a NaN or an inf at every site of tests/nonfinite_sites.py (no GPU).

tests/test_gpu_nonfinite.py holds the HIP path to these reference results; this file evaluates them on the CPU and pins, per
site, what they are -- so that a change of a site or of the oracle that empties an expectation (a reference that stays finite
where the GPU test means to see a NaN) fails here, without a GPU.

Per site, the reference (nn.Conv2d / train-mode BatchNorm2d / nn.ReLU / MaxPool2d, the FC head, the contrastive losses):
  SA block, training mode (a)
    any element of x (coordinate, feature, first row, last row; NaN, +inf, -inf; K = 16, 64, 128; D = 4, 8): the row's y1 is
      non-finite in every channel, so every batch statistic of layer 1 is, every activation after it, all of `pooled` and all
      six running buffers.
    W1[c,i], b1[c] (NaN): channel c of y1 is NaN in every row, a1[:, c] is, and W2 spreads it: `pooled`, rm2, rv2, rm3, rv3 are
      all NaN; rm1 / rv1 are NaN in channel c only.
    g2[c] (NaN): the statistics of y2 stay finite (gamma comes after them): rm1..rv2 finite; a2[:, c] is NaN, so `pooled`, rm3, rv3
      are all NaN.
    W2[c,j] (NaN): y2[:, c] is NaN: rm2 / rv2 NaN in channel c only, rm1 / rv1 finite, `pooled`, rm3, rv3 all NaN.
    W3[c,j], b3[c] (NaN): only channel c of y3: `pooled`[:, c] and rm3[c], rv3[c] NaN, everything else finite.
    be3[c] (NaN): `pooled`[:, c] NaN, every running buffer finite.
  SA block, eval mode (b): a NaN coordinate makes its row NaN in every channel of every layer and MaxPool2d hands it to the
    group: all 256 features of that group NaN, every other group finite.  A +inf coordinate gives +-inf in y1; the ReLU turns
    -inf into 0 and keeps +inf, and the next convolution adds +inf and -inf products: NaN in some channel of y2, which the
    third convolution spreads -- at this site again all 256 features of the group, every other group finite.
  SA backward (c): one NaN / +inf element of dpooled where the forward's ReLU is open: the BatchNorm backward of layer 3 spreads it
    over channel c of dy3 (inf - inf = NaN for the inf), W3 carries it to every channel below: all twelve gradients hold a
    non-finite element.
  whole model + losses (d): every site -- centre coordinate, neighbour feature (NaN, +inf, -inf), net3DV_3.3.weight, netR_FC.1.weight,
    netR_FC.3.bias (NaN), the cosine / temperature mode, a NaN in a valid row of the negative queue -- gives a non-finite loss.
  grouping (f): a NaN / +inf coordinate of a non-centroid point makes its distance sort behind every real one: the point is never
    grouped, idx / xt / yt are finite and equal those of the cloud without the point's value mattering.  A NaN / +inf feature of a
    point near centroid 0 is gathered: xt holds it at exactly the positions idx names, the coordinates stay finite.
  Adam (h): without clipping only the element with the non-finite gradient becomes non-finite (parameter and both moments; a -inf
    or +inf gradient gives exp_avg = +-inf, exp_avg_sq = +inf and the parameter NaN = inf / inf); with clip_grad_norm_ a NaN
    gradient makes the norm, the coefficient and so every parameter NaN, an infinite one makes the norm inf, the coefficient 0
    and only that element NaN (0 * inf)."""
import numpy as np
import pytest
import torch

import nonfinite_sites as NS


def _all_bad(t):
    return bool((~torch.isfinite(t)).all())


def _all_fine(t):
    return bool(torch.isfinite(t).all())


def _only(t, c):
    """non-finite exactly in channel c (last axis)"""
    bad = ~torch.isfinite(t)
    want = torch.zeros_like(bad)
    want[..., c] = True
    return bool((bad == want).all())


@pytest.mark.parametrize("case", NS.SA_TRAIN_CASES, ids=NS.ids(NS.SA_TRAIN_CASES))
def test_sa_training_reference(case):
    ref = NS.sa_reference(case, True)
    pooled, buf = ref["pooled"], ref["buffers"]
    assert pooled.shape == (case["groups"], 256)
    site = case["site"]
    if site.startswith("x_"):
        assert _all_bad(pooled) and all(_all_bad(b) for b in buf.values())
        return
    el = NS.SA_PARAM_ELEMENT[site]
    c = {"W1": el // case["D"], "W2": el // 64, "W3": el // 64}.get(site, el)
    if site in ("W1", "b1"):
        assert _all_bad(pooled) and _only(buf["rm1"], c) and _only(buf["rv1"], c)
        assert all(_all_bad(buf[k]) for k in ("rm2", "rv2", "rm3", "rv3"))
    elif site == "g2":
        assert _all_bad(pooled) and all(_all_fine(buf[k]) for k in ("rm1", "rv1", "rm2", "rv2"))
        assert _all_bad(buf["rm3"]) and _all_bad(buf["rv3"])
    elif site == "W2":
        assert _all_bad(pooled) and _all_fine(buf["rm1"]) and _all_fine(buf["rv1"])
        assert _only(buf["rm2"], c) and _only(buf["rv2"], c) and _all_bad(buf["rm3"]) and _all_bad(buf["rv3"])
    elif site in ("W3", "b3"):
        assert _only(pooled, c) and _only(buf["rm3"], c) and _only(buf["rv3"], c)
        assert all(_all_fine(buf[k]) for k in ("rm1", "rv1", "rm2", "rv2"))
    else:
        assert site == "be3" and _only(pooled, c) and all(_all_fine(b) for b in buf.values())


@pytest.mark.parametrize("case", NS.SA_EVAL_CASES, ids=NS.ids(NS.SA_EVAL_CASES))
def test_sa_eval_reference(case):
    pooled = NS.sa_reference(case, False)["pooled"]
    bad = ~torch.isfinite(pooled)
    g = (case["groups"] * case["K"] // 2 + 3) // case["K"]              # the group of site x_coord
    rows = torch.zeros(case["groups"], dtype=torch.bool)
    rows[g] = True
    assert bool((bad.any(dim=1) == rows).all()) and bool(bad[g].all())


@pytest.mark.parametrize("case", NS.SA_BWD_CASES, ids=NS.ids(NS.SA_BWD_CASES))
def test_sa_backward_reference(case):
    g, c = NS.sa_bwd_element(case)
    assert float(NS.sa_reference(dict(case, site=None), True)["pooled"][g, c]) > 0
    grads = NS.sa_bwd_reference(case)
    assert set(grads) == set(NS.SA_KEYS)
    for k, v in grads.items():
        assert not _all_fine(v), k


@pytest.mark.parametrize("case", NS.MODEL_CASES, ids=NS.ids(NS.MODEL_CASES))
def test_model_and_loss_reference(case):
    ref = NS.model_reference(case)
    c = NS.MODEL_SHAPES[case["tail"]]
    assert ref["x"].shape == (c["M"], 512) and ref["xg"].shape == (c["M"] // c["G"], 512)
    assert not np.isfinite(ref["loss"])


def test_queue_reference_equals_the_plain_loss_without_a_queue():
    """loss64's closed form with an EMPTY queue is oracle.loss on the same embeddings: the closed form is the reference's loss."""
    from oracle import loss as OL
    gen = torch.Generator().manual_seed(0)
    G, B = 4, 3
    x, xg = torch.randn(G * B, 16, generator=gen, dtype=torch.float64), torch.randn(B, 16, generator=gen, dtype=torch.float64)
    order = np.array([2, 0, 3, 1])
    lc, lo = NS.loss64({"loss": "queue"}, x, xg, G, B, order, torch.zeros(0, 16))
    assert abs(float(lc) - float(OL.global_contrast(G, xg, x, B))) < 1e-12
    assert abs(float(lo) - float(OL.circle_contrast(G, x, B, order))) < 1e-12


def test_step_reference():
    """(e): the first batch is finite, the second holds its NaN in a feature of a centroid point -- every coordinate is finite,
    so the grouping of both batches is, and the NaN is in its own group: the first loss is finite, the second is not."""
    clips, _, order = NS.step_inputs()
    b, g, pt, ch = NS.STEP_ELEMENT
    assert torch.isfinite(clips[0]).all() and int((~torch.isfinite(clips[1])).sum()) == 1
    assert ch == 3 and pt < 64 and torch.isnan(clips[1][b, g, pt, ch])
    assert sorted(order.tolist()) == list(range(NS.STEP_SHAPE["G"]))
    assert np.isfinite(NS.step_reference(0)) and not np.isfinite(NS.step_reference(1))


def test_entry_reference(tmp_path):
    """(g): the dataset on disk with one NaN feature value.  The clip is the first one of iteration 1 of epoch 0; the
    reference's views of that batch (oracle.views, the entry's NumPy stream) hold the NaN in channel 3 only -- every
    coordinate, so every centroid, is finite -- and the reference's loss on the batch is non-finite."""
    bad, batches = NS.entry_tree(tmp_path)
    assert len(batches) == NS.ENTRY["iteration"] + 1 and all(len(b) == NS.ENTRY["B"] for b in batches)
    assert bad == batches[-1][0] and all(bad not in b for b in batches[:-1])
    loss, views = NS.entry_reference(tmp_path, batches)
    assert views.shape == (10 * NS.ENTRY["B"], 512, 4)
    assert np.isfinite(views[..., :3]).all() and np.isnan(views[..., 3]).any()
    assert not np.isfinite(loss)


@pytest.mark.parametrize("value", [float("nan"), float("inf"), float("-inf"), -float.fromhex("0x1p128")])
@pytest.mark.parametrize("cloud,column", [(0, 0), (1, 2), (2, 1), (3, 0)])
def test_loaders_refuse_a_non_finite_coordinate(tmp_path, cloud, column, value):
    """The host-side guard in front of the grouping kernel (facl_amd.views.check_finite_coordinates): a NaN (either sign), an inf
    or a float64 beyond the float32 range in ANY xyz of ANY of a clip's four clouds is refused with the clip's name by
    dataset.load_clip (what DiskBatches reads through) and by views.pack_clips (what every view builder packs through), while a
    NaN in a feature channel passes both: that one has to reach the step and end in a non-finite loss."""
    from facl_amd import dataset as fds, views as V
    name = "S001C002P001R001A001"
    clip = [a.copy() for a in NS._entry_clip(3, 200, 80, 90, 70)]
    clip[cloud][3, 3] = clip[cloud][3, 5] = np.nan                     # feature channels only: accepted
    for p, a in zip(fds.clip_paths(str(tmp_path), name, "0"), clip):
        import os
        os.makedirs(os.path.dirname(p), exist_ok=True)
        np.save(p, a)
    got = fds.load_clip(str(tmp_path), name, "0")
    assert np.isnan(got[cloud][3, 3])
    V.pack_clips([got], [7])
    for v in (value, -value):
        clip[cloud][5, column] = v
        np.save(fds.clip_paths(str(tmp_path), name, "0")[cloud], clip[cloud])
        with pytest.raises(ValueError, match=r"%s: non-finite coordinate .* row 5, column %d of source cloud %d" % (name, column, cloud)):
            fds.load_clip(str(tmp_path), name, "0")
        with pytest.raises(ValueError, match="non-finite coordinate"):
            V.pack_clips([clip], [name])


@pytest.mark.parametrize("case", NS.GROUP_CASES, ids=NS.ids(NS.GROUP_CASES))
def test_grouping_reference(case):
    from oracle import grouping as OG
    idx, xt, yt = NS.group_reference(case)
    S, K, N, D = case["S"], case["K"], case["N"], case["D"]
    assert K <= N - 2 and idx.shape == (NS.GROUP_M, S, K)
    bad_pt = S + 5
    assert np.isfinite(yt).all() and np.isfinite(xt[..., :3]).all()
    if case["site"] == "coord":
        assert not (idx[1] == bad_pt).any() and np.isfinite(xt).all()
        clean = NS.group_inputs(case)
        clean[1, bad_pt, 2] = 1e3                      # any far-away finite value: the same groups
        i2, x2, _ = OG.group_points(clean, S, K, NS.GROUP_R2)
        assert np.array_equal(idx, i2) and np.array_equal(xt, x2)
    else:
        hit = idx == bad_pt
        hit[[0, 2, 3]] = False
        assert hit[1, 0].any()                         # a close neighbour of centroid 0
        assert np.array_equal(~np.isfinite(xt[..., D - 1]), hit) and np.isfinite(xt[..., :D - 1]).all()


@pytest.mark.parametrize("case", NS.ADAM_CASES, ids=NS.ids(NS.ADAM_CASES))
def test_adam_reference(case):
    out, norm = NS.adam_reference(case)
    t, e = NS.ADAM_ELEMENT
    everything = case["max_grad_norm"] and case["value"] == "nan"
    if case["max_grad_norm"]:
        assert np.isnan(norm) if case["value"] == "nan" else np.isinf(norm)
    for i, (p, m, v) in enumerate(out):
        for a in (p, m, v):
            bad = ~torch.isfinite(a)
            want = torch.zeros_like(bad)
            if everything:
                want[:] = True
            elif i == t:
                want[e] = True
            assert bool((bad == want).all()), i
