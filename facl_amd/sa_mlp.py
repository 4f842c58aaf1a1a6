"""Set-abstraction point-MLP (net3DV_1) as HIP passes: host-side orchestration.

Replaces nn.Sequential(Conv2d,BN2d,ReLU x3, MaxPool2d((1,K))) of cn3d_model_conbag.py:43-58.
The train-mode BatchNorm statistics are global over all positions, so the forward is a short
pipeline of kernels with (C,2) fp64 sum buffers between them; under DDP those buffers are the
SyncBN all-reduce points (``reduce_fn``).
"""
import torch

from . import _lib

_FWD_H3 = _lib.env_on("FACL_FWD_H3")
# eval mode through the ONE-kernel path (csrc/sa_eval.hip); FACL_EVAL_FUSED=0: the training passes with folded constants (A/B)
_EVAL_FUSED = _lib.env_on("FACL_EVAL_FUSED")
BN_EPS = 1e-5
BN_MOMENTUM = 0.1
UNIT = 64


class _Workspace:
    """Scratch for the partial-sum rows of the reducing kernels: one buffer per (device, stream).  A buffer is only ever
    touched by launches on the stream it belongs to, so calls on different streams (or threads, each with its own current
    stream) never share scratch; within one stream the launches are ordered."""
    _ws = {}

    @classmethod
    def get(cls, device):
        key = (device.type, device.index, torch.cuda.current_stream(device).cuda_stream)
        if key not in cls._ws:
            n = _lib.call_size("facl_ws_bytes")
            cls._ws[key] = torch.empty(n, dtype=torch.uint8, device=device)
        if _lib.POISON:
            cls._ws[key].fill_(0xFF)                     # NaN bytes: every partial row a reduction reads must be rewritten
        return cls._ws[key]


def _bn_finalize(sums, C, count, gamma, beta, running_mean, running_var, momentum=BN_MOMENTUM, aamax=None, zamax=None, after=None):
    """`aamax` (one row of _lib.amax_buffers): receives the bound of the layer's activation, the fp16x3 scale of the GEMM that
    consumes it (|gamma| sqrt(count - 1) sigma invstd + |beta|: csrc/finalize.hip).
    `after`: the (5, C') constants of the layer in front.  The heavy passes apply that layer's ReLU as max(v, 0), which drops a
    NaN; a non-finite scale or shift there makes every statistic of this layer NaN instead (facl_bn_finalize_after), as the
    reference's are -- the same launch, nothing changes while the constants are finite."""
    bnc = _lib.empty((5, C), dtype=torch.float32, device=sums.device)
    prev, nprev = (None, 0) if after is None else (after[2], 2 * after.shape[1])       # rows 2..3: scale | shift, contiguous
    _lib.call("facl_bn_finalize_after", sums, C, float(count), gamma, beta, BN_EPS, momentum, running_mean, running_var, bnc,
              aamax, zamax, prev, nprev)
    return bnc


def act_amax_eval(y_rows, bnc, aamax):
    """Eval mode: running statistics say nothing about the data, so the activation maximum max relu(scale y + shift) is
    MEASURED (one streaming pass over the layer's raw output) into `aamax`."""
    R, C = y_rows.shape
    _lib.call("facl_rows_act_amax", y_rows, R, C, bnc[2], bnc[3], aamax)


_FRAG_ORDER = {}


def _frag_channel_order(dev):
    """Channel of every float of ONE position-pair... of a unit tile in the fragment layout (csrc/common.h), as a (4096,) index
    tensor: element ((ct*2 + rt)*4 + r4)*256 + lane*4 + e holds channel 32 rt + 8 r4 + 4 (lane >> 5) + e."""
    key = (dev.type, dev.index)
    if key not in _FRAG_ORDER:
        i = torch.arange(4096, device=dev)
        e, lane, r4, rt = i & 3, (i >> 2) & 63, (i >> 8) & 3, (i >> 10) & 1
        _FRAG_ORDER[key] = 32 * rt + 8 * r4 + 4 * (lane >> 5) + e
    return _FRAG_ORDER[key]


def _bn_eval(C, gamma, beta, running_mean, running_var, after=None):
    """`after`: a float32 / int32 tensor the layer's input depends on; a non-finite word in it makes every constant NaN
    (facl_bn_eval_consts_after)."""
    bnc = _lib.empty((5, C), dtype=torch.float32, device=gamma.device)
    _lib.call("facl_bn_eval_consts_after", C, gamma, beta, running_mean, running_var, BN_EPS, bnc, after,
              0 if after is None else after.numel())
    return bnc


def _running_update(bnc, rm, rv, n_true):
    """Running-statistics update with an explicit element count (used when positions are replicated: the batch
    mean / biased variance are unaffected by uniform replication, the unbiased factor n/(n-1) is not)."""
    mean = bnc[0]
    var = 1.0 / (bnc[1].double() ** 2) - BN_EPS
    unb = (var * (n_true / max(n_true - 1.0, 1.0))).float()
    rm.mul_(1 - BN_MOMENTUM).add_(mean, alpha=BN_MOMENTUM)
    rv.mul_(1 - BN_MOMENTUM).add_(unb, alpha=BN_MOMENTUM)


def sa_mlp_forward(x_rows, p, training, reduce_fn=None, update_running=True, K=64, precision="f32", eval_backward=False):
    """x_rows (P,D) contiguous fp32, P = groups*K rows.  ``p``: dict with W1,b1,g1,be1,rm1,rv1, ...3.
    Returns (pooled (groups,256), ctx) where ctx carries what the backward needs.
    ``reduce_fn(t)`` (optional) all-reduces an fp64 tensor in place (SyncBN).
    ``eval_backward`` (eval mode only): a backward may follow (frozen BatchNorm), so the forward takes the storing passes, which
    keep y2 / ymax / arg, instead of the one-kernel eval path, which keeps nothing.

    The kernels work on units of 64 positions.  K = 64 (the reference's live value, utils_my.py:260) maps one
    group to one unit.  Other K are served around the same kernels (cold path, tensor glue):
      * K = 64*R: a group spans R units; their per-unit maxima are merged before the pooling step and the
        sparse backward values are routed to the winning unit;
      * K | 64: every group is replicated 64/K times inside its unit.  Uniform replication leaves the batch mean,
        the biased variance, the max and (with P' = replicated count used consistently) every gradient unchanged;
        only the unbiased running-variance factor needs the true count."""
    _lib.require_cuda(x_rows)
    rep, R = 1, 1
    if K != UNIT:
        if K > UNIT and K % UNIT == 0:
            R = K // UNIT
        elif 0 < K < UNIT and UNIT % K == 0:
            rep = UNIT // K
            G_, D_ = x_rows.shape[0] // K, x_rows.shape[1]
            x_rows = x_rows.view(G_, K, D_).repeat(1, rep, 1).reshape(G_ * UNIT, D_).contiguous()
        else:
            raise NotImplementedError("knn_K must divide 64 or be a multiple of 64 (got %d)" % K)
    P, D = x_rows.shape
    if P % UNIT:
        raise ValueError("P must be a multiple of 64 (knn_K = 64)")
    if not _lib.SA_D_MIN <= D <= _lib.SA_D_MAX:
        raise NotImplementedError("INPUT_FEATURE_NUM must be in %d..%d (got %d)" % (_lib.SA_D_MIN, _lib.SA_D_MAX, D))
    nunits = P // UNIT
    dev = x_rows.device
    ws = _Workspace.get(dev)
    f64 = dict(dtype=torch.float64, device=dev)
    count = float(P)
    W1 = p["W1"].reshape(64, D)
    W2 = p["W2"].reshape(64, 64)
    W3 = p["W3"].reshape(256, 64)
    L1C = _lib.sa_l1_cols(D)                       # folded layer-1 table row: weights | bias in column L1C - 4 (include/facl_hip.h)
    ctx = {}
    # fp16x3 operand maxima (csrc/common.h): [0] max|x| (eval), [1] bound of a1, [2] bound of a2, [3] max(pooled)
    # training: [1], [2] are stored by facl_bn_finalize and [3] is zeroed by BN3's finalize call right before facl_sa_pool
    # raises it -- no fill launch; eval measures with atomics and starts from zeros
    amax = _lib.amax_buffers(4, dev, zero=not training)
    if training:
        mom = _lib.empty(D + D * D, **f64)
        _lib.call("facl_sa_x_moments", x_rows, P, D, mom, ws)
        ctx["mom_local"] = mom
        if reduce_fn is not None:
            mom = reduce_fn(mom.clone())
            count = float(P) * reduce_fn.world_size          # every rank holds the same number of positions
        sums1 = _lib.empty((64, 2), **f64)
        direct = update_running and rep == 1
        n_true = count / rep
        rm, rv = (p["rm1"], p["rv1"]) if direct else (None, None)
        # sums of y1 from the moments -> BatchNorm-1 constants (+ running statistics, + the bound of a1) -> folded layer-1 table:
        # one single-wave launch (facl_sa_bn1_chain; bit-identical to facl_bn1_sums_from_moments + facl_bn_finalize + facl_sa_l1tab)
        bnc1 = _lib.empty((5, 64), dtype=torch.float32, device=dev)
        l1tab = _lib.empty((64, L1C), dtype=torch.float32, device=dev)
        _lib.call("facl_sa_bn1_chain", mom, count, D, W1, p["b1"], p["g1"], p["be1"], BN_EPS, BN_MOMENTUM, rm, rv, sums1, bnc1,
                  amax[1], l1tab)
        if update_running and not direct:
            _running_update(bnc1, p["rm1"], p["rv1"], n_true)
        ctx["mom"] = mom
    else:
        bnc1 = _bn_eval(64, p["g1"], p["be1"], p["rm1"], p["rv1"])
        xa = amax[0]                                       # eval: the bound of a1 follows from max|x| (facl_sa_l1tab)
        _lib.call("facl_absmax", x_rows, x_rows.numel(), xa)
        l1tab = _lib.empty((64, L1C), dtype=torch.float32, device=dev)
        _lib.call("facl_sa_l1tab", W1, p["b1"], D, bnc1[2], bnc1[3], l1tab, xa, amax[1])
    if not training and not eval_backward and _EVAL_FUSED and precision in ("f32", "x3b") and _FWD_H3:
        # eval mode = the extraction path (extract_motion_feature.py:143-221): every BatchNorm is a constant affine, so the whole
        # block is ONE kernel per unit, x -> pooled, with nothing stored in between (csrc/sa_eval.hip)
        bnc2 = _bn_eval(64, p["g2"], p["be2"], p["rm2"], p["rv2"])
        bnc3 = _bn_eval(256, p["g3"], p["be3"], p["rm3"], p["rv3"])
        pooled_u = _lib.empty((nunits, 256), dtype=torch.float32, device=dev)
        with _lib.timed("facl_sa_eval"):
            _lib.call("facl_sa_eval", x_rows, nunits, D, l1tab, W2, p["b2"], bnc2[2], bnc2[3], W3, p["b3"], bnc3[2], bnc3[3],
                      pooled_u, amax[1])
        if R > 1:      # a group spans R units: BN + ReLU are monotone per channel, so the group's feature is the maximum of its units'
            pooled_u = pooled_u.view(nunits // R, R, 256).max(dim=1).values.contiguous()
        return pooled_u, {"amax": None, "nunits": nunits, "D": D, "R": R, "x_rows": x_rows}
    y2f = _lib.empty(nunits * UNIT * 64, dtype=torch.float32, device=dev)
    sums2 = _lib.empty((64, 2), **f64) if training else None
    with _lib.timed("facl_sa_fwd2"):
        _lib.call("facl_sa_fwd2", x_rows, nunits, D, l1tab, W2, p["b2"], y2f, sums2, ws, amax[1])
    if training:
        if reduce_fn is not None:
            reduce_fn(sums2)
        rm, rv = (p["rm2"], p["rv2"]) if direct else (None, None)
        bnc2 = _bn_finalize(sums2, 64, count, p["g2"], p["be2"], rm, rv, aamax=amax[2], after=bnc1)
        if update_running and not direct:
            _running_update(bnc2, p["rm2"], p["rv2"], n_true)
    else:
        bnc2 = _bn_eval(64, p["g2"], p["be2"], p["rm2"], p["rv2"])
        # eval: measured maximum of a2.  The fragment layout keeps 4 consecutive channels per float4 and the 64 channels of a
        # position in 16 float4s whose channel base is a function of the float4's index alone -- the row kernel only needs the
        # per-float4 constants in that order
        lay = _frag_channel_order(dev)
        sc_l, sh_l = bnc2[2][lay].contiguous(), bnc2[3][lay].contiguous()
        _lib.call("facl_rows_act_amax", y2f, nunits, 4096, sc_l, sh_l, amax[2])
    sgn3 = p["g3"]                                                    # the kernels take sign(gamma3) themselves (sign(0) = +1)
    ymax = _lib.empty((nunits, 256), dtype=torch.float32, device=dev)
    arg = _lib.empty((nunits, 256), dtype=torch.uint8, device=dev)
    sums3 = _lib.empty((256, 2), **f64) if training else None
    with _lib.timed("facl_sa_fwd3"):
        # dense configuration: fp16-input 64->256 layer; "x3": the opt-in three-product variant (tail.precision)
        # "f32" / "x3b": the fp32-grade forward -- fp16x3 (csrc/common.h; FACL_FWD_H3=0 selects bf16x6 for A/B)
        f32_fwd3 = "facl_sa_fwd3_h3" if _FWD_H3 else "facl_sa_fwd3"
        fwd3 = {"f32": f32_fwd3, "f16": "facl_sa_fwd3_f16", "x3": "facl_sa_fwd3_x3", "x3b": f32_fwd3}[precision]
        extra = (amax[2],) if fwd3 == "facl_sa_fwd3_h3" else ()
        _lib.call(fwd3, y2f, nunits, bnc2[2], bnc2[3], W3, p["b3"], sgn3, ymax, arg, sums3, ws, *extra)
    _lib.tap("sa_arg", arg)
    if training:
        if reduce_fn is not None:
            reduce_fn(sums3)
        rm, rv = (p["rm3"], p["rv3"]) if direct else (None, None)
        bnc3 = _bn_finalize(sums3, 256, count, p["g3"], p["be3"], rm, rv, zamax=amax[3], after=bnc2)
        if update_running and not direct:
            _running_update(bnc3, p["rm3"], p["rv3"], n_true)
    else:
        # these passes drop a NaN / inf of x in their ReLUs and eval mode has no statistics to carry it: facl_absmax flagged it in
        # amax[0], and the last layer's constants -- so every feature -- become NaN (a superset of the groups the reference loses)
        bnc3 = _bn_eval(256, p["g3"], p["be3"], p["rm3"], p["rv3"], after=amax[0])
    ngroups, ymax_g, rsel = nunits, ymax, None
    if R > 1:                                    # a group spans R units: merge their maxima (first unit wins ties)
        ngroups = nunits // R
        ymax_g, rsel = ymax.view(ngroups, R, 256).max(dim=1)
        ymax_g = ymax_g.contiguous()
    pooled = _lib.empty((ngroups, 256), dtype=torch.float32, device=dev)
    _lib.call("facl_sa_pool", ymax_g, ngroups, 256, bnc3[2], bnc3[3], pooled, amax[3])
    if _lib.TAPS is not None and K == UNIT:          # tests only: the ReLU decisions of the three layers (tie-proof parity)
        xd, tb = x_rows.double(), l1tab.double()
        v = (tb[:, 0] * xd[:, :1] + tb[:, L1C - 4]).float().double()          # the kernels' sequential fp32 FMA chain
        for i in range(1, D):
            v = (tb[:, i] * xd[:, i:i + 1] + v).float().double()
        _lib.TAPS["relu_sa1"] = v > 0
        y2n = y2f.view(nunits, 2, 2, 4, 2, 32, 4).permute(0, 1, 5, 2, 3, 4, 6).reshape(nunits * UNIT, 64)   # fragment layout -> (P, 64)
        _lib.tap_relu("relu_sa2", y2n, bnc2[2], bnc2[3])
        _lib.tap_relu("relu_sa3", a=pooled)
    ctx["amax"] = amax                               # [1], [2]: the backward's operand scales; [3]: max(pooled) for the next GEMM
    ctx.update(y2f=y2f, ymax=ymax_g, arg=arg, bnc1=bnc1, bnc2=bnc2, bnc3=bnc3, sgn3=sgn3, l1tab=l1tab, count=count,
               nunits=nunits, D=D, R=R, rsel=rsel, ngroups=ngroups, x_rows=x_rows, training=training)
    return pooled, ctx


def sa_mlp_backward(ctx, dpooled, x_rows, p, reduce_fn=None):
    x_rows = ctx["x_rows"]                       # the (possibly replicated) rows the forward actually ran on
    return _sa_mlp_backward(ctx, dpooled, x_rows, p, reduce_fn)


def _sa_mlp_backward(ctx, dpooled, x_rows, p, reduce_fn=None):
    """Gradients of the 12 parameters of net3DV_1 given dL/dpooled (P/64,256).

    Four heavy passes (csrc/sa_bwd.hip) with three fp64 closed-form assembly kernels between them
    (csrc/finalize.hip).  ``reduce_fn`` all-reduces the BN-backward sums (SyncBN); parameter gradients stay
    LOCAL sums (the data-parallel wrapper averages them).

    A forward in eval mode (``ctx["training"]`` False: BatchNorm frozen at its running statistics) runs the SAME heavy passes:
    every batch-statistic term reaches them through the tables G3 / h3 / bw2 only, which the frozen closed forms hand over
    without those terms; nothing is all-reduced, and b1, b2, b3 get real gradients."""
    dev = x_rows.device
    ws = _Workspace.get(dev)
    f64 = dict(dtype=torch.float64, device=dev)
    f32 = dict(dtype=torch.float32, device=dev)
    nunits, D, P = ctx["nunits"], ctx["D"], float(ctx["count"])
    bnc1, bnc2, bnc3 = ctx["bnc1"], ctx["bnc2"], ctx["bnc3"]
    W1 = p["W1"].reshape(64, D)
    W2 = p["W2"].reshape(64, 64)
    W3 = p["W3"].reshape(256, 64)
    dpooled = dpooled.contiguous()

    # ---- pass 0: sparse values + (dbeta3, dgamma3)
    ngroups, R = ctx["ngroups"], ctx["R"]
    coef = _lib.empty((ngroups, 256), **f32)
    sums0 = _lib.empty((256, 2), **f64)
    _lib.call("facl_sa_bwd0", dpooled, ctx["ymax"], ngroups, bnc3, coef, sums0, ws)
    if R > 1:                                    # route each group's sparse value to the unit that won the max
        cu = torch.zeros((ngroups, R, 256), **f32)
        cu.scatter_(1, ctx["rsel"].unsqueeze(1), coef.unsqueeze(1))
        coef = cu.view(nunits, 256)
    frozen = not ctx.get("training", True)
    if frozen:
        reduce_fn = None                         # a constant affine: no sum of this backward is global
    sums0_l = sums0
    if reduce_fn is not None:
        sums0 = reduce_fn(sums0.clone())
    G3, h3 = _lib.empty((64, 64), **f32), _lib.empty(64, **f32)
    if frozen:
        _lib.call("facl_sa_bwd_consts3_frozen", G3, h3)
    else:
        _lib.call("facl_sa_bwd_consts3", sums0, bnc3, W3, p["b3"], P, G3, h3)

    # ---- pass 1: dz2 + (dbeta2, dgamma2)
    dz2f = _lib.empty_like(ctx["y2f"])
    sums1 = _lib.empty((64, 2), **f64)
    with _lib.timed("facl_sa_bwd1"):
        _lib.call("facl_sa_bwd1", ctx["y2f"], nunits, bnc2, G3, h3, W3, coef, ctx["arg"], dz2f, sums1, ws, ctx["amax"][2])
    sums1_l = sums1
    if reduce_fn is not None:
        sums1 = reduce_fn(sums1.clone())

    # ---- pass 2: dy2, da1, dz1, dW2, R1 -- launched right behind pass 1 and walking the units backwards: the ends of dz2 / y2
    # that pass 1 touched last are still in the memory-side cache (FACL_BWD2_REV=0: front to back)
    bw2 = _lib.empty((4, 64), **f32)
    if frozen:
        _lib.call("facl_sa_bwd_consts2_frozen", bnc2, bw2)
    else:
        _lib.call("facl_sa_bwd_consts2", sums1, bnc2, P, bw2)
    out2 = _lib.empty(_lib.sa_bwd2_out(D), **f64)
    with _lib.timed("facl_sa_bwd2"):
        _lib.call("facl_sa_bwd2", dz2f, ctx["y2f"], x_rows, nunits, D, bw2, W2, ctx["l1tab"], out2, ws, ctx["amax"][1])
    # ---- layer-3 weight gradient ingredients: sparse gather, Gram, sum a2
    out3 = _lib.empty(256 * 64 + 64 * 64 + 64, **f64)
    with _lib.timed("facl_sa_bwd_w3"):
        _lib.call("facl_sa_bwd_w3", ctx["y2f"], nunits, bnc2, coef, ctx["arg"], out3, ws, ctx["amax"][2])

    g = {"W3": _lib.empty_like(p["W3"]), "g3": _lib.empty(256, **f32), "be3": _lib.empty(256, **f32),
         "W2": _lib.empty_like(p["W2"]), "g2": _lib.empty(64, **f32), "be2": _lib.empty(64, **f32),
         "W1": _lib.empty_like(p["W1"]), "g1": _lib.empty(64, **f32), "be1": _lib.empty(64, **f32),
         # d(bias) of a conv that feeds a train-mode BN is identically zero: None (the parameter is left untouched)
         "b1": None, "b2": None, "b3": None}
    if frozen:                                   # ... and a real gradient behind a frozen one: sum dy = scale * dbeta
        g.update(b1=_lib.empty(64, **f32), b2=_lib.empty(64, **f32), b3=_lib.empty(256, **f32))
        _lib.call("facl_sa_bwd_final_frozen", out3, sums0, bnc3, out2, sums1, bnc2, bnc1, W1, p["b1"], D, g["W3"], g["g3"],
                  g["be3"], g["b3"], g["W2"], g["g2"], g["be2"], g["b2"], g["W1"], g["g1"], g["be1"], g["b1"])
        return g
    R1_g = out2[4096:]                           # (sa_l1_cols(D), 64): rows x_0..x_{D-1}, sum dz1, zeros
    if reduce_fn is not None:
        R1_g = reduce_fn(R1_g.clone())
    _lib.call("facl_sa_bwd_final", out3, sums0, sums0_l, bnc3, W3, p["b3"], out2, sums1_l, R1_g, ctx["mom_local"], bnc1, W1,
              p["b1"], D, P, g["W3"], g["g3"], g["be3"], g["W2"], g["g2"], g["be2"], g["W1"], g["g1"], g["be1"])
    return g


_PARAM_ORDER = ("W1", "b1", "g1", "be1", "W2", "b2", "g2", "be2", "W3", "b3", "g3", "be3")


class SAMLPFunction(torch.autograd.Function):
    """pooled = net3DV_1(x) with HIP forward and backward.  ``state`` carries the BN buffers
    (updated in place in training mode), the mode flag and the optional SyncBN reduce_fn."""

    @staticmethod
    def forward(ctx, x_rows, state, *params):
        p = dict(zip(_PARAM_ORDER, [t.detach().contiguous() for t in params]))
        p.update(state["buffers"])
        # eval mode: the one-kernel path keeps nothing for a backward; the storing passes run only when one can follow
        pooled, c = sa_mlp_forward(x_rows, p, state["training"], state.get("reduce_fn"), K=state.get("K", UNIT),
                                   precision=state.get("precision", "f32"),
                                   eval_backward=not state["training"] and any(ctx.needs_input_grad))
        # max(pooled): the fp16x3 scale of the GEMM that consumes the features (the fused eval kernel keeps none: measured there)
        state["pooled_amax"] = None if c.get("amax") is None else c["amax"][3]
        ctx.c, ctx.p, ctx.x_rows, ctx.reduce_fn = c, p, x_rows, state.get("reduce_fn")
        ctx.training = state["training"]
        return pooled

    @staticmethod
    def backward(ctx, dpooled):
        g = sa_mlp_backward(ctx.c, dpooled, ctx.x_rows, ctx.p, ctx.reduce_fn)    # ctx.c["training"] selects the frozen closed forms
        return (None, None) + tuple(g[k] for k in _PARAM_ORDER)
