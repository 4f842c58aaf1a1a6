"""Grouping ops -- drop-in for the reference's ``training_code/utils_my.py`` grouping functions.

Same names, arguments, return shapes/strides and ``opt`` side effects as the reference
(utils_my.py:7-42, :217-253, :255-291, :293-328); the body is one fused HIP kernel
(facl_group) instead of the expand/sub/mul/sum/topk/masked-assign/gather chain.
"""
import numpy as np
import torch

from . import _lib


def knn_radius_group(points, sample_num_level1, knn_K, ball_radius, want_idx=False):
    """points (M,N,D) float32 CUDA -> (inputs_level1 (M,D,S,K) view, center (M,3,S,1) view[, idx]).

    The returned tensors are transposed VIEWS of contiguous (M,S,K,D) / (M,S,3) buffers, exactly
    like the reference's (utils_my.py:283-284).  ``points`` is not modified.
    A 4-D ``points`` (B,G,N,D) is the loader's clip-major batch: the outputs are those of
    ``points.permute(1,0,2,3).reshape(G*B,N,D)`` (cn3d_train_motion_GL.py:226) without materialising that copy.

    The xyz of the centroids (rows 0..S-1 of every cloud) must be finite: the kernel's selection is undefined for a NaN / inf
    centroid.  The tensor is on the device, so it is not checked here; the loaders check the clips on the host
    (facl_amd.views.check_finite_coordinates).  A non-finite value elsewhere -- another point's xyz, any feature channel --
    is handled like the reference does (the point sorts last; the feature is gathered)."""
    _lib.require_cuda(points)
    if points.dtype != torch.float32:
        raise TypeError("points must be float32 (the reference casts with .type(torch.FloatTensor))")
    pts = points.contiguous()
    if pts.dim() == 4:
        return _knn_radius_group_clips(pts, sample_num_level1, knn_K, ball_radius, want_idx)
    M, N, D = pts.shape
    S, K = int(sample_num_level1), int(knn_K)
    xt = _lib.empty((M, S, K, D), dtype=torch.float32, device=pts.device)
    yt = _lib.empty((M, S, 3), dtype=torch.float32, device=pts.device)
    idx = _lib.empty((M, S, K), dtype=torch.int32, device=pts.device) if want_idx else None
    with _lib.timed("facl_group"):
        _lib.call("facl_group", pts, M, N, D, S, K, float(ball_radius), idx, xt, yt)
    inputs_level1 = xt.permute(0, 3, 1, 2)                       # (M,D,S,K), utils_my.py:283
    inputs_level1_center = yt.view(M, 1, S, 3).transpose(1, 3)   # (M,3,S,1), utils_my.py:284
    if want_idx:
        return inputs_level1, inputs_level1_center, idx
    return inputs_level1, inputs_level1_center


def _knn_radius_group_clips(clips, sample_num_level1, knn_K, ball_radius, want_idx):
    B, G, N, D = clips.shape
    M, S, K = B * G, int(sample_num_level1), int(knn_K)
    xt = _lib.empty((M, S, K, D), dtype=torch.float32, device=clips.device)
    yt = _lib.empty((M, S, 3), dtype=torch.float32, device=clips.device)
    idx = _lib.empty((M, S, K), dtype=torch.int32, device=clips.device) if want_idx else None
    with _lib.timed("facl_group"):
        _lib.call("facl_group_clips", clips, B, G, N, D, S, K, float(ball_radius), idx, xt, yt)
    out = (xt.permute(0, 3, 1, 2), yt.view(M, 1, S, 3).transpose(1, 3))
    return out + (idx,) if want_idx else out


def group_points_3DV(points, opt):
    """utils_my.py:255-291.  Like the reference it overwrites ``opt.INPUT_FEATURE_NUM`` (from
    the data), ``opt.knn_K = 64`` and ``opt.ball_radius = 0.06`` (:259-261)."""
    cur_train_size = points.shape[0]
    opt.INPUT_FEATURE_NUM = points.shape[-1]
    opt.knn_K = 64
    opt.ball_radius = 0.06
    points = points.view(cur_train_size, opt.SAMPLE_NUM, -1)
    return knn_radius_group(points, opt.sample_num_level1, opt.knn_K, opt.ball_radius)


def group_points_3DV_2048(points, knn_K, sample_num_level1, SAMPLE_NUM=2048):
    """utils_my.py:7-42: N-parametrised twin, r^2 = 0.16 (:13)."""
    cur_train_size = points.shape[0]
    points = points.view(cur_train_size, -1, points.shape[-1])
    if points.shape[1] != SAMPLE_NUM:
        raise RuntimeError("points has %d rows per cloud, SAMPLE_NUM=%d" % (points.shape[1], SAMPLE_NUM))
    return knn_radius_group(points, sample_num_level1, knn_K, 0.16)


def group_points_3DV_nums(points, opt, sample_num_level1, knn_K):
    """utils_my.py:293-328: explicit S and K, r^2 = 0.06 (:299)."""
    cur_train_size = points.shape[0]
    opt.INPUT_FEATURE_NUM = points.shape[-1]
    opt.ball_radius = 0.06
    points = points.view(cur_train_size, opt.SAMPLE_NUM, -1)
    return knn_radius_group(points, sample_num_level1, knn_K, opt.ball_radius)


def group_points(points, opt):
    """utils_my.py:217-253: K = 64, r^2 = 0.14 (:220-221)."""
    opt.knn_K = 64
    opt.ball_radius = 0.14
    cur_train_size = points.shape[0]
    opt.INPUT_FEATURE_NUM = points.shape[-1]
    points = points.view(cur_train_size, opt.SAMPLE_NUM, -1)
    return knn_radius_group(points, opt.sample_num_level1, opt.knn_K, opt.ball_radius)


# ---- contrastive losses (utils_my.py:53-116 = cn3d_train_motion_GL.py:265-316) -------------------
# Loss modes (no counterpart in the reference; the defaults are the reference's loss):
#   normalize    every embedding row r -> r / max(||r||_2, 1e-12) (F.normalize), x_global rows included: cosine similarity
#   temperature  similarities are divided by tau; folded into the rows as the factor s = fp32(1 / sqrt(tau))
#   mask         'zero': same-clip key columns are multiplied by 0 and stay in the softmax as exp(0) (the reference);
#                'exclude': they are no members of the log-sum-exp at all (negatives only)
#                'class': 'exclude', and the keys of clips KNOWN to share the anchor's class leave the log-sum-exp too (false-
#                negative removal with labels).  Every key clip carries an int32 class id, >= 0 a class, < 0 unknown; key column
#                j of anchor clip c is masked iff clip(j) == c or (id[c] >= 0 and id[clip(j)] == id[c]); a queue row with the id
#                q of the clip that pushed it iff id[c] >= 0 and q == id[c].  Positives stay the clip's own views.  A clip may
#                be left without a negative: its log-sum-exp is -inf, its terms and gradients are exactly 0
#   class_positives  (mask 'class' only) lambda > 0: the cells that mask 'class' removes for a reason other than "own clip" -- key
#                columns of OTHER clips with the anchor's known class, queue rows with it: the clip's class cells C -- are
#                positive slots against the same log-sum-exp as well, through their mean term:
#                loss_n = sum_s term(pos_s) + (lambda nS / |C|) sum_{c in C} term(sim_c), term(p) = logaddexp(p, lse) - p, nS the
#                clip's own slots (G resp. G-1); nothing is added when |C| = 0, and |C| is a count (not differentiated).  0 = off
MASK_MODES = {"zero": 0, "exclude": 1, "class": 2}


def check_class_positives(class_positives, mask):
    """The weight of the class cells as a float: finite and >= 0, and > 0 only with mask 'class'; ValueError otherwise."""
    w = float(class_positives)
    if not (w >= 0.0 and w < float("inf")):
        raise ValueError("class_positives must be finite and >= 0 (got %r)" % (class_positives,))
    if w > 0.0 and mask != "class":
        raise ValueError("class_positives adds the keys that mask 'class' removes as positives: it needs mask 'class' "
                         "(got mask %r)" % (mask,))
    return w


def loss_scale(temperature):
    """s = fp32(1 / sqrt(tau)), the factor on every embedding row; ValueError unless tau is finite and positive."""
    t = float(temperature)
    if not (t > 0.0 and t < float("inf")):
        raise ValueError("the loss temperature must be finite and positive (got %r)" % (temperature,))
    s = float(np.float32(1.0 / np.sqrt(t)))
    if not (s > 0.0 and s < float("inf")):
        raise ValueError("the loss temperature %r is outside the fp32 range of 1 / sqrt(tau)" % (temperature,))
    return s


def check_loss_mode(temperature, mask, key_clips=None):
    """The host refusals of the loss modes, before any launch: (s, mask_mode) or ValueError."""
    s = loss_scale(temperature)
    if mask not in MASK_MODES:
        raise ValueError("unknown loss mask %r (one of %s)" % (mask, ", ".join(sorted(MASK_MODES))))
    if mask in ("exclude", "class") and key_clips is not None and key_clips < 2:
        raise ValueError("mask %r with one key clip leaves no negative: it needs batch x world >= 2" % mask)
    return s, MASK_MODES[mask]


def is_default_loss_mode(normalize, temperature, mask):
    """True for the reference's loss (no row pass, mask mode zero)."""
    return not normalize and float(temperature) == 1.0 and mask == "zero"


def _loss_rows_torch(x, normalize, temperature):
    """n = x * s / max(||x||, 1e-12) resp. x * s in x's dtype (the truth of the HIP row pass); x itself at the defaults."""
    if not normalize and float(temperature) == 1.0:
        return x
    s = loss_scale(temperature)
    return (torch.nn.functional.normalize(x, p=2, dim=1, eps=1e-12) if normalize else x) * s


def _check_classes(mask, key_classes, Bk, queue=None, queue_classes=None):
    """mask 'class' needs one id per key clip (and per queue row); any other mask takes none.  The ids as int64 on their device."""
    if mask != "class":
        if key_classes is not None or queue_classes is not None:
            raise ValueError("class ids belong to mask 'class' (got mask %r)" % (mask,))
        return None, None
    if key_classes is None:
        raise ValueError("mask 'class' needs the class ids of the key clips")
    if key_classes.dim() != 1 or key_classes.shape[0] != Bk:
        raise ValueError("mask 'class' takes one class id per key clip, (%d,); got %s" % (Bk, tuple(key_classes.shape)))
    Q = 0 if queue is None else queue.shape[0]
    if Q and (queue_classes is None or queue_classes.dim() != 1 or queue_classes.shape[0] != Q):
        raise ValueError("mask 'class' with a queue takes one class id per queue row, (%d,)" % Q)
    return key_classes.long(), (queue_classes.long() if Q else None)


def _masked_sim(anchors, keys, anchor_clip, key_clip, mask="zero", key_classes=None):
    """l_neg = (anchors @ keys^T) * mask, mask = 0 where the key belongs to the anchor's own clip
    (utils_my.py:55-56,71-72).  Same-clip columns are multiplied by 0 -- NOT removed -- so each of them
    still contributes exp(0) = 1 to the softmax denominator, exactly like the reference.  mask 'exclude': they become
    -inf, i.e. they leave the log-sum-exp.  mask 'class': so do the columns of clips known to share the anchor's class
    (``key_classes`` (Bk,): the class id of every key clip, < 0 = unknown, which matches nothing)."""
    sim = anchors @ keys.t()
    same = anchor_clip[:, None] == key_clip[None, :]
    if mask == "class":
        kc = key_classes.to(sim.device)
        a_cls, k_cls = kc[anchor_clip], kc[key_clip]
        same = same | ((a_cls[:, None] >= 0) & (a_cls[:, None] == k_cls[None, :]))
    fill = 0.0 if mask == "zero" else float("-inf")
    return torch.where(same, torch.full((), fill, dtype=sim.dtype, device=sim.device), sim)


def _queue_sim(anchors, queue, anchor_classes=None, queue_classes=None):
    """anchors @ queue^T for the valid rows of a negative queue (stored as they are: never mapped again); None without rows.
    mask 'class' (``anchor_classes`` given): -inf where the anchor's class is known and is the queue row's."""
    if queue is None or queue.shape[0] == 0:
        return None
    sim = anchors @ queue.to(device=anchors.device, dtype=anchors.dtype).t()
    if anchor_classes is None:
        return sim
    a_cls, q_cls = anchor_classes.to(sim.device), queue_classes.to(sim.device)
    same = (a_cls[:, None] >= 0) & (a_cls[:, None] == q_cls[None, :])
    return torch.where(same, torch.full((), float("-inf"), dtype=sim.dtype, device=sim.device), sim)


def _lse_rows(neg, mask):
    """logsumexp over dim 1.  mask 'class' may leave a row without a member (all -inf): its value is -inf, and -- treated
    explicitly, autograd of logsumexp over an all -inf row yields NaN -- it sends no gradient anywhere."""
    if mask != "class":
        return torch.logsumexp(neg, dim=1)
    empty = (neg == float("-inf")).all(dim=1)
    lse = torch.logsumexp(torch.where(empty[:, None], torch.zeros((), dtype=neg.dtype, device=neg.device), neg), dim=1)
    return torch.where(empty, torch.full((), float("-inf"), dtype=neg.dtype, device=neg.device), lse)


def _pair_terms(pos, lse):
    """sum over slots of mean over clips of logaddexp(pos, lse) - pos; a clip with lse = -inf (no negative) contributes exactly
    0 and no gradient (logaddexp(pos, -inf) - pos is 0 with derivative 0, which autograd would form as 1 - 1)."""
    empty = (lse == float("-inf")).unsqueeze(0)
    if not bool(empty.any()):
        return (torch.logaddexp(pos, lse.unsqueeze(0)) - pos).mean(dim=1).sum()
    zero = torch.zeros((), dtype=pos.dtype, device=pos.device)
    t = torch.logaddexp(torch.where(empty, zero, pos), torch.where(empty, zero, lse.unsqueeze(0))) - torch.where(empty, zero, pos)
    return torch.where(empty, zero, t).mean(dim=1).sum()


def _class_cell_terms(anchors, keys, anchor_clip, key_clip, kc, queue, qc, nA, lse, nS, weight):
    """The class cells' share of a loss: sum over the B clips of (weight nS / |C_n|) sum_{c in C_n} term(v_c, lse_n), divided by
    B.  ``anchors``: nA * B rows, row i * B + n an anchor row of local clip n.  A clip with lse = -inf contributes exactly 0 and
    no gradient (treated explicitly, as in _pair_terms); so does a clip without a class cell.  None when no clip has one."""
    B = anchors.shape[0] // nA
    kc = kc.to(anchors.device)
    a_cls = kc[anchor_clip]
    vals = anchors @ keys.t()
    cell = (a_cls[:, None] >= 0) & (a_cls[:, None] == kc[key_clip][None, :]) & (anchor_clip[:, None] != key_clip[None, :])
    if queue is not None and queue.shape[0]:
        vals = torch.cat((vals, anchors @ queue.to(device=anchors.device, dtype=anchors.dtype).t()), dim=1)
        cell = torch.cat((cell, (a_cls[:, None] >= 0) & (a_cls[:, None] == qc.to(anchors.device)[None, :])), dim=1)
    vals = vals.view(nA, B, -1).permute(1, 0, 2).reshape(B, -1)
    cell = cell.view(nA, B, -1).permute(1, 0, 2).reshape(B, -1)
    count = cell.sum(dim=1)
    if not bool(count.any()):
        return None
    use = cell & (lse != float("-inf"))[:, None]
    zero = torch.zeros((), dtype=vals.dtype, device=vals.device)
    v, l = torch.where(use, vals, zero), torch.where(use, lse[:, None].expand_as(vals), zero)
    terms = torch.where(use, torch.logaddexp(v, l) - v, zero).sum(dim=1)
    w = weight * nS / count.clamp_min(1).to(vals.dtype)
    return (torch.where(count > 0, w * terms, zero)).sum() / B


def _clip_ids(G, B, device, offset=0):
    return (torch.arange(B, device=device) + offset).repeat(G)     # row g*B+b -> clip id b


def global_contrast(num_crop, x_global, x, opt, criterion=None, x_keys=None, clip_offset=0, normalize=False, temperature=1.0,
                    mask='zero', queue=None, key_classes=None, queue_classes=None, class_positives=0.0):
    """utils_my.py:53-83.  loss_c = sum_g CE([<xg_n, x_{gB+n}> | (xg @ x^T)*mask], 0), CE = mean over B.
    The (G,B,1+GB) logits tensor and its ``repeat`` are never built: every g shares the negatives, so
    CE_g[n] = logaddexp(pos[g,n], LSE_n) - pos[g,n].

    Data-parallel form: ``x_keys`` = the all-gathered view-major embeddings (G*B_global rows) and
    ``clip_offset`` = rank*B_local; anchors stay local (mean over local B, gradients averaged by DDP).

    ``normalize`` / ``temperature`` / ``mask``: the loss modes above.  The rows of x_global, x and x_keys (the gathered RAW
    embeddings: normalising a row commutes with gathering it) are mapped first; the rest is unchanged.

    ``queue``: the valid rows (Q, C) of a negative queue (facl_amd/neg_queue.py), extra negative columns <xg_n, q_k> of every
    clip.  They carry no clip identity (masks 'zero' and 'exclude' do not touch them) and are used as stored.

    ``key_classes`` (Bk,) / ``queue_classes`` (Q,): the class ids of mask 'class' (see the loss modes above), integer tensors;
    required with that mask (the queue's whenever the queue has rows), refused with any other.

    ``class_positives``: the weight of the class cells as extra positives (the loss modes above); mask 'class' only."""
    B, G = x_global.shape[0], num_crop
    cp = check_class_positives(class_positives, mask)
    check_loss_mode(temperature, mask, (x if x_keys is None else x_keys).shape[0] // G)
    x_global, x = _loss_rows_torch(x_global, normalize, temperature), _loss_rows_torch(x, normalize, temperature)
    keys = x if x_keys is None else _loss_rows_torch(x_keys, normalize, temperature)
    Bk = keys.shape[0] // G
    kc, qc = _check_classes(mask, key_classes, Bk, queue, queue_classes)
    a_clip = torch.arange(B, device=x.device) + clip_offset
    neg = _masked_sim(x_global, keys, a_clip, _clip_ids(G, Bk, x.device), mask, kc)  # (B, G*Bk)
    neg_q = _queue_sim(x_global, queue, *(() if qc is None else (kc.to(x.device)[a_clip], qc)))
    if neg_q is not None:
        neg = torch.cat((neg, neg_q), dim=1)
    lse = _lse_rows(neg, mask)
    pos = (x_global.unsqueeze(0) * x.view(G, B, -1)).sum(-1)                   # (G,B)
    if mask == "class":
        extra = None if not cp else _class_cell_terms(x_global, keys, a_clip, _clip_ids(G, Bk, x.device), kc, queue, qc, 1, lse, G, cp)
        return _pair_terms(pos, lse) if extra is None else _pair_terms(pos, lse) + extra
    return (torch.logaddexp(pos, lse.unsqueeze(0)) - pos).mean(dim=1).sum()


def circle_contrast(num_crop, x, batchSize, criterion=None, order=None, x_keys=None, clip_offset=0, normalize=False,
                    temperature=1.0, mask='zero', queue=None, key_classes=None, queue_classes=None, class_positives=0.0):
    """utils_my.py:85-116.  ``order`` replaces the reference's np.random.shuffle(arange(num_crop)) (:96-97);
    when omitted it is drawn from NumPy's global RNG like the reference.  Loss modes, ``queue`` and the class ids: as in
    global_contrast (the shared negative set of a clip becomes the (G-1) x (J + Q) block); ``class_positives``: the class cells
    of that block, against nS = G-1 own slots."""
    G, B = num_crop, batchSize
    cp = check_class_positives(class_positives, mask)
    check_loss_mode(temperature, mask, (x if x_keys is None else x_keys).shape[0] // G)
    if order is None:
        order = np.arange(0, G, 1)
        np.random.shuffle(order)
    order = torch.as_tensor(np.asarray(order), device=x.device, dtype=torch.long)
    x = _loss_rows_torch(x, normalize, temperature)
    keys = x if x_keys is None else _loss_rows_torch(x_keys, normalize, temperature)
    Bk = keys.shape[0] // G
    xv = x.view(G, B, -1)
    anchors = xv[order[:-1]]                                                   # (G-1,B,C)
    pos = (anchors * xv[order[1:]]).sum(-1)                                    # (G-1,B)   :100
    kc, qc = _check_classes(mask, key_classes, Bk, queue, queue_classes)
    a_clip = (torch.arange(B, device=x.device) + clip_offset).repeat(G - 1)
    neg = _masked_sim(anchors.reshape((G - 1) * B, -1), keys, a_clip, _clip_ids(G, Bk, x.device), mask, kc)
    neg = neg.view(G - 1, B, G * Bk).permute(1, 0, 2).reshape(B, -1)           # all anchors' negatives, shared (:105-109)
    neg_q = _queue_sim(anchors.reshape((G - 1) * B, -1), queue, *(() if qc is None else (kc.to(x.device)[a_clip], qc)))
    if neg_q is not None:
        neg = torch.cat((neg, neg_q.view(G - 1, B, -1).permute(1, 0, 2).reshape(B, -1)), dim=1)
    lse = _lse_rows(neg, mask)
    if mask == "class":
        extra = None if not cp else _class_cell_terms(anchors.reshape((G - 1) * B, -1), keys, a_clip, _clip_ids(G, Bk, x.device), kc,
                                                      queue, qc, G - 1, lse, G - 1, cp)
        return _pair_terms(pos, lse) if extra is None else _pair_terms(pos, lse) + extra
    return (torch.logaddexp(pos, lse.unsqueeze(0)) - pos).mean(dim=1).sum()


# ---- fused HIP path for both losses (csrc/loss.hip): one similarity GEMM + one loss launch ------------
class _ContrastivePair(torch.autograd.Function):
    """(loss_c, loss_circle) from the stacked embeddings [x ; x_global] ((G+1)*B rows): ONE similarity GEMM
    sim = stacked @ keys^T on the hand-written MFMA GEMM, ONE loss launch (facl_contrast_pair_sum_mask: both values and
    d/dsim, the circle anchors addressed through ``order`` instead of gathered), and in the backward one dgrad
    (d stacked = dsim @ keys) plus one wgrad (d keys = dsim^T @ stacked).  The reference's anchors gather and its two
    similarity products (utils_my.py:63-71,100-103) have no counterpart here.

    ``queue`` (a facl_amd.neg_queue.NegativeQueue): a second similarity GEMM sim_q = stacked @ queue^T, the loss launch is
    facl_contrast_pair_queue (the valid queue rows are extra negatives, read on the device), and the backward adds
    dsim_q @ queue to d stacked.  The queue itself gets no gradient and is not written here.

    ``classes`` (mask mode 2, `class`): the int32 class ids of the Bk key clips on the device; the launches are
    facl_contrast_pair_sum_cls resp. facl_contrast_pair_queue_cls with the queue's own ``ids``; with ``class_positives`` > 0
    facl_contrast_pair_sum_sup resp. facl_contrast_pair_queue_sup."""

    @staticmethod
    def forward(ctx, stacked, keys, order, G, clip_offset, mask_mode=0, queue=None, classes=None, class_positives=0.0):
        from . import tail as _tail
        from .sa_mlp import _Workspace
        _lib.require_cuda(stacked, keys)
        dev = stacked.device
        ws = _Workspace.get(dev)
        stacked = stacked.contiguous()
        R, C = stacked.shape
        B = R // (G + 1)
        ctx.own_keys = keys is None                # single process: the keys ARE the view rows of `stacked`
        keys = stacked[:G * B] if keys is None else keys.contiguous()
        J = keys.shape[0]
        Bk = J // G
        ctx.mfma = (J % 4 == 0 and C % 4 == 0)     # the MFMA GEMMs contract over multiples of 4; odd toy shapes: library GEMM
        ctx.prec = _tail.current_precision()       # the backward GEMMs run in the forward's arithmetic
        sim = _tail.gemm_fwd(stacked, keys, None, prec=ctx.prec)[0] if ctx.mfma else stacked @ keys.t()     # ((G+1)B, J)  :71 and :103
        dsim = _lib.empty_like(sim)
        out = _lib.empty(2, dtype=torch.float64, device=dev)
        # [loss_c, loss_circle, loss_circle + loss_c] in fp32 from the loss launch's own finishing kernel (no cast / add launches)
        out32 = _lib.empty(3, dtype=torch.float32, device=dev)
        ctx.queue = queue is not None
        if (mask_mode == MASK_MODES["class"]) != (classes is not None):
            raise ValueError("mask 'class' and the class ids of the key clips come together")
        if classes is not None:
            _lib.require_cuda(classes)
            if classes.dtype != torch.int32 or tuple(classes.shape) != (Bk,) or classes.device != dev or not classes.is_contiguous():
                raise ValueError("classes must be a contiguous int32 (%d,) tensor on %s: one id per key clip; got %s %s on %s"
                                 % (Bk, dev, classes.dtype, tuple(classes.shape), classes.device))
            if queue is not None and getattr(queue, "ids", None) is None:
                raise ValueError("mask 'class' needs a queue that keeps the class ids of its rows: NegativeQueue(..., with_ids=True)")
        if class_positives and classes is None:
            raise ValueError("class_positives needs mask 'class' and the class ids of the key clips")
        if queue is None and class_positives:
            _lib.call("facl_contrast_pair_sum_sup", sim, G, B, Bk, J, order, clip_offset, classes, float(class_positives), dsim,
                      out, out32, ws)
            ctx.save_for_backward(stacked, keys, dsim)
        elif queue is None and classes is not None:
            _lib.call("facl_contrast_pair_sum_cls", sim, G, B, Bk, J, order, clip_offset, classes, dsim, out, out32, ws)
            ctx.save_for_backward(stacked, keys, dsim)
        elif queue is None:
            _lib.call("facl_contrast_pair_sum_mask", sim, G, B, Bk, J, order, clip_offset, mask_mode, dsim, out, out32, ws)
            ctx.save_for_backward(stacked, keys, dsim)
        else:
            if queue.C != C or queue.buf.device != dev:
                raise ValueError("the negative queue holds rows of %d floats on %s; the embeddings have %d on %s"
                                 % (queue.C, queue.buf.device, C, dev))
            L = queue.L
            ctx.mfma_q = (L % 4 == 0 and C % 4 == 0)
            sim_q = _tail.gemm_fwd(stacked, queue.buf, None, prec=ctx.prec)[0] if ctx.mfma_q else stacked @ queue.buf.t()
            dsim_q = _lib.empty_like(sim_q)
            if class_positives:
                _lib.call("facl_contrast_pair_queue_sup", sim, sim_q, G, B, Bk, J, L, order, clip_offset, classes, queue.ids,
                          queue.state, float(class_positives), dsim, dsim_q, out, out32, ws)
            elif classes is not None:
                _lib.call("facl_contrast_pair_queue_cls", sim, sim_q, G, B, Bk, J, L, order, clip_offset, classes, queue.ids,
                          queue.state, dsim, dsim_q, out, out32, ws)
            else:
                _lib.call("facl_contrast_pair_queue", sim, sim_q, G, B, Bk, J, L, order, clip_offset, mask_mode, queue.state,
                          dsim, dsim_q, out, out32, ws)
            ctx.save_for_backward(stacked, keys, dsim, dsim_q, queue.buf)
        ctx.GB = G * B
        ctx.set_materialize_grads(False)           # an unused loss output arrives as None, not as a freshly filled zero tensor
        return out32[0], out32[1], out32[2]

    @staticmethod
    def backward(ctx, g_c, g_o, g_s):
        from . import tail as _tail
        bp = _tail.backward_precision(ctx.prec)
        stacked, keys, dsim = ctx.saved_tensors[:3]
        # upstream gradients of (loss_c, loss_circle, their sum): the training step only uses the sum (no launch here); any
        # other combination is tensor algebra on device scalars
        def tot(g):
            if g is None:
                return g_s
            g = g.contiguous().float()
            return g if g_s is None else g + g_s.float()
        g_c, g_o = tot(g_c), tot(g_o)
        if g_c is None and g_o is None:
            return None, None, None, None, None, None, None, None, None
        zero = None
        if g_c is None or g_o is None:
            zero = torch.zeros((), dtype=torch.float32, device=dsim.device)
        g_c = zero if g_c is None else g_c.contiguous().float()
        g_o = zero if g_o is None else g_o.contiguous().float()
        # rows [0, G*B) carry the circle loss, rows [G*B, (G+1)*B) the global loss: one scaling launch for both
        ds = _lib.empty_like(dsim)
        R, J = dsim.shape
        _lib.call("facl_scale_rows2", dsim, ds, ctx.GB, R, J, g_o, g_c)
        d_stacked = _tail.gemm_dgrad(ds, keys, prec=bp) if ctx.mfma else ds @ keys
        if ctx.queue:                              # the queue's columns: d stacked += dsim_q @ queue (the queue gets no gradient)
            dsim_q, qbuf = ctx.saved_tensors[3:]
            dq = _lib.empty_like(dsim_q)
            _lib.call("facl_scale_rows2", dsim_q, dq, ctx.GB, R, dsim_q.shape[1], g_o, g_c)
            d_stacked += _tail.gemm_dgrad(dq, qbuf, prec=bp) if ctx.mfma_q else dq @ qbuf
        if ctx.own_keys and ctx.mfma:
            # d keys = dsim^T @ stacked accumulated straight into the view rows of d stacked (the keys ARE those rows)
            M_, N_, K_ = ds.shape[0], ds.shape[1], stacked.shape[1]
            pc = {"f32": 0, "x3b": 0, "f16": 1, "x3": 2}[bp]
            with _lib.timed("facl_gemm_wgrad %dx%dx%d%s" % (M_, N_, K_, _tail._LABEL[bp])):
                rc = _lib.call("facl_gemm_wgrad_acc", ds, stacked, M_, N_, K_, stacked.stride(0), d_stacked, pc, accept=(_lib.E_CONFIG,))
            if rc != _lib.E_CONFIG:
                return d_stacked, None, None, None, None, None, None, None, None
        d_keys = _tail.gemm_wgrad(ds, stacked, prec=bp) if ctx.mfma else ds.t() @ stacked
        if ctx.own_keys:
            d_stacked[:ctx.GB] += d_keys
            d_keys = None
        return d_stacked, d_keys, None, None, None, None, None, None, None


class _LossRows(torch.autograd.Function):
    """n = rows * s / max(||row||, 1e-12) (normalize) or rows * s, s = fp32(1 / sqrt(tau)): the row pass in front of
    _ContrastivePair (csrc/loss.hip: k_loss_rows_fwd / _bwd), one launch each way."""

    @staticmethod
    def forward(ctx, x, normalize, s):
        _lib.require_cuda(x)
        if x.dtype != torch.float32 or x.dim() != 2:
            raise TypeError("the loss row pass takes a 2-D float32 matrix")
        x = x.contiguous()
        R, C = x.shape
        n = _lib.empty_like(x)
        inv = _lib.empty(R, dtype=torch.float32, device=x.device)
        _lib.call("facl_loss_rows_fwd", x, R, C, int(normalize), s, n, inv, detail="R=%d, C=%d" % (R, C))
        ctx.save_for_backward(n, inv)
        ctx.mode = (int(normalize), s)
        return n

    @staticmethod
    def backward(ctx, dn):
        n, inv = ctx.saved_tensors
        normalize, s = ctx.mode
        dn = dn.contiguous().float()
        dx = _lib.empty_like(n)
        R, C = n.shape
        _lib.call("facl_loss_rows_bwd", dn, n, inv, R, C, normalize, s, dx, detail="R=%d, C=%d" % (R, C))
        return dx, None, None


def loss_rows(x, normalize=False, temperature=1.0):
    """The loss modes' row map of a (R, C) float32 matrix on the GPU (C % 4 == 0): x * s / max(||x||, 1e-12) or x * s."""
    return _LossRows.apply(x, bool(normalize), loss_scale(temperature))


def _check_order(order, G):
    """A host-side `order` (list / ndarray / CPU tensor) must be a permutation of range(G) (np.random.shuffle of
    arange(G), cn3d_train_motion_GL.py:297-298).  A device tensor is not read back (no sync on the step); the kernel
    clamps its entries so that a corrupt one cannot address outside the similarity matrix."""
    o = np.asarray(order.cpu() if torch.is_tensor(order) else order).reshape(-1)
    if o.shape[0] != G or not np.array_equal(np.sort(o), np.arange(G)):
        raise ValueError("order must be a permutation of range(%d), got %r" % (G, o.tolist()))


def contrastive_losses_stacked(num_crop, stacked, order, x_keys=None, clip_offset=0, with_sum=False, normalize=False,
                               temperature=1.0, mask='zero', queue=None, queue_rows=None, classes=None, class_positives=0.0):
    """(loss_c, loss_circle) from the model's stacked output [x ; x_global] (facl_amd.cn3d_model_conbag: ``_stacked``);
    with_sum: also `loss_circle + loss_c` (fp32, cn3d_train_motion_GL.py:329) as a third output of the same launch.

    ``normalize`` / ``temperature`` / ``mask``: the loss modes (see global_contrast).  At the defaults nothing but today's
    launches runs.  Otherwise one row pass n = loss_rows(stacked) runs in front and the loss sees n.  ``x_keys`` is the
    gathered RAW view-major embeddings (they take the row pass too), or -- what the data-parallel step uses, a row pass over
    the local rows only -- a callable that maps this rank's view rows n[:G*B] to the gathered keys.

    ``queue``: a facl_amd.neg_queue.NegativeQueue whose valid rows are extra negatives of every clip (see _ContrastivePair).
    The step's own key rows for it, n[G*B:] (x_global after the row map, detached), are staged on the queue; the caller
    pushes them (``queue.push()``) after the backward.  None: today's launches, nothing else.

    ``queue_rows``: raw (B, C) rows to stage instead -- the x_global rows of a key encoder (facl_amd/key_encoder.py).  They take
    the same row map, in a launch of their own; the loss does not read them.  None: the step's own rows, as above.

    ``classes``: mask 'class' only, and required there -- the int32 device tensor of the Bk key clips' class ids (< 0: unknown).
    With a queue (created ``with_ids``) the ids of this rank's clips, classes[clip_offset : clip_offset + B], are staged beside
    the rows.  The tensor is read by the launches, not copied: a captured step sees what it holds at replay.

    ``class_positives``: lambda > 0 (mask 'class' only) makes the class cells extra positives of weight lambda (the loss modes,
    see global_contrast): the launch is facl_contrast_pair_sum_sup / _queue_sup.  0: today's launches."""
    cp = check_class_positives(class_positives, mask)
    if (mask == "class") != (classes is not None):
        raise ValueError("mask 'class' needs classes=, the class ids of the key clips, and no other mask takes them "
                         "(got mask %r %s classes)" % (mask, "without" if classes is None else "with"))
    G = num_crop
    GB = G * (stacked.shape[0] // (G + 1))
    if queue_rows is not None:
        if queue is None:
            raise ValueError("queue_rows are rows for a negative queue: pass queue= as well")
        if queue_rows.dim() != 2 or queue_rows.shape != (stacked.shape[0] - GB, stacked.shape[1]):
            raise ValueError("queue_rows must be one raw row per clip, (%d, %d); got %s"
                             % (stacked.shape[0] - GB, stacked.shape[1], tuple(queue_rows.shape)))
        queue_rows = queue_rows.detach()
    if is_default_loss_mode(normalize, temperature, mask):
        mask_mode = 0
        if callable(x_keys):
            x_keys = x_keys(stacked[:GB])
    else:
        key_rows = GB if x_keys is None or callable(x_keys) else x_keys.shape[0]
        s, mask_mode = check_loss_mode(temperature, mask, None if callable(x_keys) else key_rows // G)
        if normalize or s != 1.0:
            stacked = _LossRows.apply(stacked, bool(normalize), s)
            if queue_rows is not None:
                queue_rows = _LossRows.apply(queue_rows, bool(normalize), s)
            if x_keys is not None and not callable(x_keys):
                x_keys = _LossRows.apply(x_keys, bool(normalize), s)
        if callable(x_keys):
            x_keys = x_keys(stacked[:GB])
            check_loss_mode(temperature, mask, x_keys.shape[0] // G)
    if not (torch.is_tensor(order) and order.device == stacked.device and order.dtype == torch.long):
        _check_order(order, G)
        order = torch.as_tensor(order, device=stacked.device, dtype=torch.long)
    if queue is None:
        out = _ContrastivePair.apply(stacked, x_keys, order.contiguous(), G, clip_offset, mask_mode, None, classes, cp)
    else:
        rows = stacked.detach()[GB:] if queue_rows is None else queue_rows
        if classes is None:
            queue.stage(rows)
        else:
            queue.stage(rows, ids=classes[clip_offset:clip_offset + rows.shape[0]])
        out = _ContrastivePair.apply(stacked, x_keys, order.contiguous(), G, clip_offset, mask_mode, queue, classes, cp)
    return out if with_sum else out[:2]
