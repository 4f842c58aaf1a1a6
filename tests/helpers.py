import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_golden(name):
    return dict(np.load(os.path.join(GOLDEN, name), allow_pickle=False))


def canon_groups_np(xt_MSKD):
    """Sort the K axis of (M,S,K,D) lexicographically (order inside a group is unspecified)."""
    a = np.asarray(xt_MSKD)
    M, S, K, D = a.shape
    flat = a.reshape(M * S, K, D)
    out = np.empty_like(flat)
    for i in range(flat.shape[0]):
        keys = tuple(flat[i, :, d] for d in reversed(range(D)))
        out[i] = flat[i][np.lexsort(keys)]
    return out.reshape(M, S, K, D)


def rel_err(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def bn_consts(K, g):
    """Random (5, K) BatchNorm constants on the generator's device: mean | invstd | scale | shift | (unused)."""
    import torch
    dev = g.device
    return torch.stack((torch.randn(K, device=dev, generator=g) * 0.1, torch.rand(K, device=dev, generator=g) + 0.5,
                        torch.randn(K, device=dev, generator=g), torch.randn(K, device=dev, generator=g) * 0.3,
                        torch.zeros(K, device=dev))).contiguous()


def clear_of_the_relu_edge(y, bnc):
    """Entries whose scale*y + shift is within rounding of 0 would open or close the ReLU depending on fma vs mul+add; the
    reference expression of the caller is not the kernel's instruction sequence, so move them well inside the open side."""
    import torch
    t = bnc[2].double() * y.double() + bnc[3].double()
    return torch.where(t.abs() < 1e-4, ((1.0 - bnc[3]) / bnc[2]).expand_as(y), y).contiguous()


def max_rel_rows(a, b):
    """max over rows of ||a_i-b_i|| / ||b_i|| (features: atol scaled by row norm, SURVEY hard part 4)."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    num = np.linalg.norm(a - b, axis=-1)
    den = np.maximum(np.linalg.norm(b, axis=-1), 1e-30)
    return float((num / den).max())


def sa_params(sd, dev, dtype=None):
    """The 18 tensors of net3DV_1 under the names facl_amd/sa_mlp.py uses (W1 .. rv3), on `dev`, fp32 unless `dtype`."""
    import torch
    m = {"W1": "net3DV_1.0.weight", "b1": "net3DV_1.0.bias", "g1": "net3DV_1.1.weight", "be1": "net3DV_1.1.bias",
         "rm1": "net3DV_1.1.running_mean", "rv1": "net3DV_1.1.running_var",
         "W2": "net3DV_1.3.weight", "b2": "net3DV_1.3.bias", "g2": "net3DV_1.4.weight", "be2": "net3DV_1.4.bias",
         "rm2": "net3DV_1.4.running_mean", "rv2": "net3DV_1.4.running_var",
         "W3": "net3DV_1.6.weight", "b3": "net3DV_1.6.bias", "g3": "net3DV_1.7.weight", "be3": "net3DV_1.7.bias",
         "rm3": "net3DV_1.7.running_mean", "rv3": "net3DV_1.7.running_var"}
    return {k: torch.as_tensor(sd[v]).to(dev).to(dtype or torch.float32).contiguous() for k, v in m.items()}


def oracle_pooled(sd, xt_MDSK, training, dtype):
    """net3DV_1 of the oracle (oracle/encoder.py), in `dtype`, on CPU."""
    import torch
    import torch.nn.functional as F
    from oracle import encoder as E
    sd = {k: (torch.as_tensor(v).to(dtype) if np.asarray(v).dtype.kind == "f" else torch.as_tensor(v).clone())
          for k, v in sd.items()}
    h = xt_MDSK.to(dtype)
    with torch.no_grad():
        for li in (0, 3, 6):
            h = E._conv_bn_relu(sd, "net3DV_1", li, h, training)
        pooled = F.max_pool2d(h, (1, h.shape[-1]), stride=1)
    return pooled.squeeze(-1).permute(0, 2, 1).reshape(-1, 256), sd


def synth_clip(seed, dt, P=900, Kp=300, R1=500, R2=200):
    """The four (rows, 8) clouds `__getitem__` loads for one video (cn3D_data_set.py:105-116), synthetic; the same
    formula as tools/make_goldens.py: synth_clip, whose arguments tests/golden/views.npz records in `cases`."""
    r = np.random.RandomState(seed)
    pts = (r.rand(P, 8) - 0.5).astype(dt)
    pts[::3, 4] = 0
    pts[1::4, 7] = 0
    return pts, (r.rand(Kp, 8) - 0.5).astype(dt), (r.rand(R1, 8) - 0.5).astype(dt), (r.rand(R2, 8) - 0.5).astype(dt)


def golden_view_clips(g):
    """The clips of views.npz, rebuilt from the recorded generator arguments, in stream order, with their tags."""
    out = []
    for tag, (cseed, is64, P, Kp, R1, R2) in zip("abcd", g["cases"].tolist()):
        out.append((tag, synth_clip(cseed, np.float64 if is64 else np.float32, P, Kp, R1, R2)))
    return out


# ---- plain torch-fp64 evaluation of the encoder on grouped rows, optionally with the KERNEL's max-pool routing -----------
def forward64(x_rows, centers, sd, G, S, K, dev, routing=None, grad=False, dtype=None):
    """cn3d_model_conbag.py:213-234 in fp64 (matmuls, train-mode BN with batch statistics, ReLU, the three max-pools) on
    (P,D) grouped rows / (M*S,3) centres.  Returns (x, x_global, stats, q, ties).

    `routing` = {"sa_arg" (M*S,256), "seg_arg" (M,1024), "view_arg" (B,1024)}: the argmax indices the HIP forward chose.
    Each max-pool then GATHERS at those indices instead of taking its own maximum, so the autograd graph routes the gradient
    exactly as the kernels do and a comparison of gradients no longer depends on which side of a numerical near-tie each
    arithmetic lands on.  `ties[name]` = the largest distance of a gathered value from the true fp64 maximum, relative to
    max(|max|, mean |activation|): the test that every differing decision WAS a tie.
    `grad`: parameters require grad (q[k].grad after a backward).  `dtype` (default float64): torch.float32 gives the
    "plain torch fp32 with the same routing" twin -- the conditioning yardstick of a gradient comparison."""
    import torch
    dtype = torch.float64 if dtype is None else dtype
    q = {k: torch.as_tensor(v).to(dev).to(dtype) for k, v in sd.items() if np.asarray(v).dtype.kind == "f"}
    if grad:
        for k in q:
            if "running" not in k:
                q[k].requires_grad_(True)
    stats, ties = {}, {}

    def bn_train(y, gamma, beta, key):
        P = y.shape[0]
        mean, var = y.mean(0), y.var(0, unbiased=False)
        stats[key] = (mean.detach(), (var * (P / (P - 1.0))).detach())
        return (y - mean) / torch.sqrt(var + 1e-5) * gamma + beta

    def pool(h3, idx, name):                                                   # (R, L, C) -> (R, C) over L
        mx = h3.max(dim=1).values
        if idx is None:
            return mx
        got = torch.gather(h3, 1, idx.long().view(h3.shape[0], 1, h3.shape[2])).squeeze(1)
        with torch.no_grad():
            scale = torch.maximum(mx.abs(), h3.abs().mean())
            ties[name] = float(((mx - got).abs() / scale).max())
            ties[name + "_flips"] = int((idx.long().view(h3.shape[0], h3.shape[2]) != h3.argmax(dim=1)).sum())
        return got

    r = routing or {}

    def relu(z, name):
        """ReLU, or -- with the kernel's own decisions in `routing` -- z * mask.  Every decision that differs from z > 0 must
        be a numerical tie: |z| there <= 1e-5 of the layer's mean |z| (recorded in ties["relu_*"])."""
        mask = r.get(name)
        if mask is None:
            return torch.relu(z)
        with torch.no_grad():
            diff = mask.view(z.shape) != (z > 0)
            ties[name + "_flips"] = int(diff.sum())
            ties[name] = float((z.abs() * diff).max() / z.abs().mean())
        return z * mask.view(z.shape)

    h = x_rows.to(dtype)
    for i, li in enumerate((0, 3, 6)):                                         # net3DV_1 (:43-58)
        W = q[f"net3DV_1.{li}.weight"].reshape(q[f"net3DV_1.{li}.weight"].shape[0], -1)
        y = h @ W.t() + q[f"net3DV_1.{li}.bias"]
        z = bn_train(y, q[f"net3DV_1.{li + 1}.weight"], q[f"net3DV_1.{li + 1}.bias"], f"net3DV_1.{li + 1}")
        del y
        # the third layer's ReLU sits behind the max-pool in the kernels (monotone per channel): its decision is pinned there
        h = relu(z, f"relu_sa{i + 1}") if i < 2 else z
        del z
    MS = h.shape[0] // K
    pooled = pool(h.view(MS, K, 256), r.get("sa_arg"), "sa")
    del h
    pooled = relu(pooled, "relu_sa3")
    h = torch.cat((centers.to(dtype), pooled), dim=1)                           # :219
    for i, li in enumerate((0, 3, 6)):                                         # net3DV_3 (:61-77)
        W = q[f"net3DV_3.{li}.weight"].reshape(q[f"net3DV_3.{li}.weight"].shape[0], -1)
        y = h @ W.t() + q[f"net3DV_3.{li}.bias"]
        z = bn_train(y, q[f"net3DV_3.{li + 1}.weight"], q[f"net3DV_3.{li + 1}.bias"], f"net3DV_3.{li + 1}")
        h = relu(z, f"relu_t{i + 1}") if i < 2 else z
    M = MS // S
    B = M // G
    x_pre = relu(pool(h.view(M, S, 1024), r.get("seg_arg"), "seg"), "relu_t3")   # :222 (max of relu = relu of max)
    # :225-226 (rows are view-major g*B+b): max over all G*S local features of a clip = max over the views of the view maxima
    xg_pre = pool(x_pre.view(G, B, 1024).transpose(0, 1), r.get("view_arg"), "view")

    fcm = r.get("relu_fc")                                                     # (M + B, 1024): view rows, then clip rows

    def head(t, key, mask):                                                    # netR_FC (:201-207), two BN calls (:228-229)
        y = t @ q["netR_FC.0.weight"].t() + q["netR_FC.0.bias"]
        z = bn_train(y, q["netR_FC.1.weight"], q["netR_FC.1.bias"], key)
        if mask is not None:
            r["relu_" + key] = mask
        a = relu(z, "relu_" + key)
        return a @ q["netR_FC.3.weight"].t() + q["netR_FC.3.bias"]
    r = dict(r)
    x = head(x_pre, "fc_a", None if fcm is None else fcm[:M])
    xg = head(xg_pre, "fc_b", None if fcm is None else fcm[M:])
    return x, xg, stats, q, ties


class routing_taps:
    """with routing_taps() as r: <HIP forward> -> r = {"sa_arg", "seg_arg", "view_arg"}: the argmax tensors of the three
    max-pools of that forward (facl_amd/_lib.py: tap)."""

    def __enter__(self):
        from facl_amd import _lib
        self.prev, _lib.TAPS = _lib.TAPS, {}
        return _lib.TAPS

    def __exit__(self, *exc):
        from facl_amd import _lib
        _lib.TAPS = self.prev
        return False


# ---- one training step from ANY state (not only the fresh one), in torch fp64 --------------------------------------------
SA_T_BN = ("net3DV_1.1", "net3DV_1.4", "net3DV_1.7", "net3DV_3.1", "net3DV_3.4", "net3DV_3.7")
PRE_BN_BIAS = frozenset({"net3DV_1.0.bias", "net3DV_1.3.bias", "net3DV_1.6.bias", "net3DV_3.0.bias", "net3DV_3.3.bias",
                         "net3DV_3.6.bias", "netR_FC.0.bias"})        # in front of a train-mode BatchNorm: no gradient


def snapshot(net, optimizer):
    """Host-side deep copy of everything a training step reads: parameters, BatchNorm running buffers and
    num_batches_tracked (net.state_dict() writes the host-side counters into the buffers first), the optimizer's exp_avg /
    exp_avg_sq / step / lr.  FusedAdam.state_dict() SHARES its moment tensors: they are copied here.
    s["net"], s["optim"] load into a twin (net.load_state_dict / optimizer.load_state_dict); s["adam"] = {name: state},
    s["step"], s["lr"]."""
    import copy
    import torch
    net_sd = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    osd = optimizer.state_dict()
    state = {i: {k: (v.detach().cpu().clone() if torch.is_tensor(v) else v) for k, v in st.items()}
             for i, st in osd["state"].items()}
    optim_sd = {"state": state, "param_groups": copy.deepcopy(osd["param_groups"])}
    names = {id(p): n for n, p in net.named_parameters()}
    pnames = [names[id(p)] for p in optimizer.param_groups[0]["params"]]
    steps = {int(st["step"]) for st in state.values() if "step" in st}
    assert len(steps) <= 1, steps
    return {"net": net_sd, "optim": optim_sd, "adam": {pnames[i]: st for i, st in state.items()},
            "step": steps.pop() if steps else 0, "lr": float(optim_sd["param_groups"][0]["lr"])}


# facl_amd.optim.FusedAdam passes its betas to the kernels as fp32: its moment updates and bias corrections are torch's with
# beta2 = fp32(0.999) = 0.99900001287 (1 - beta2 = 0.99998712e-3), so its exp_avg_sq sits 1.3e-5 below torch.optim.Adam's with
# beta2 = 0.999; the parameter updates agree with torch's to rounding (v and its bias correction carry the same factor).
FUSED_ADAM_BETAS = (0.5, float(np.float32(0.999)))


def adam64(snap, grads, betas=(0.5, 0.999), eps=1e-6):
    """torch.optim.Adam (cn3d_train_motion_GL.py:180) in fp64, started from the snapshot's parameters, moments, step count
    and lr, applied to `grads` {name: tensor} (parameters without an entry are skipped, like a None .grad).
    Returns {name: (param, exp_avg, exp_avg_sq)} after the update, fp64 on the gradients' device."""
    import torch
    f64 = torch.float64
    ps, out = [], {}
    for n, g in grads.items():
        dev = g.device
        p = snap["net"][n].to(dev, f64).clone().requires_grad_(True)
        p.grad = g.detach().to(f64).reshape(p.shape).clone()
        ps.append((n, p))
    opt = torch.optim.Adam([p for _, p in ps], lr=snap["lr"], betas=betas, eps=eps, foreach=False)
    for n, p in ps:
        st = snap["adam"].get(n)
        if st is not None and snap["step"] > 0:
            opt.state[p] = {"step": torch.tensor(float(snap["step"])), "exp_avg": st["exp_avg"].to(p.device, f64).clone(),
                            "exp_avg_sq": st["exp_avg_sq"].to(p.device, f64).clone()}
    opt.step()
    for n, p in ps:
        out[n] = (p.detach(), opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"])
    return out


def reference_step64(snap, x_rows, centers, G, B, S, K, order, routing, backward=True, momentum=0.1, betas=(0.5, 0.999)):
    """The reference's training step (cn3d_train_motion_GL.py:224-335, without the SwAV / CLD terms) from the state in
    `snap` (snapshot()), evaluated in torch fp64 on the grouped rows (x_rows (P,D), centers (M*S,3)):
      x, xg, loss_c, loss_circle   -- forward with the fp64 max-pools / ReLUs, losses through oracle.loss;
      running                      -- {key: (running_mean, running_var)} after the step (momentum 0.1, netR_FC.1 twice);
    and with `backward` (routing = the kernel's max-pool and ReLU decisions, routing_taps()):
      g64, ties                    -- every parameter gradient, routed through those decisions; ties as in forward64;
      adam64                       -- adam64(snap, g64, betas): parameters and moments after Adam on the fp64 gradients;
      g32, x32, xg32, loss_c32, loss_circle32 -- the same routed computation in plain torch fp32 (conditioning yardstick)."""
    import torch
    from oracle import loss as OL
    dev = x_rows.device
    sd = snap["net"]
    out = {}
    with torch.no_grad():
        x, xg, stats, q, _ = forward64(x_rows, centers, sd, G, S, K, dev)
        out.update(x=x, xg=xg, loss_c=float(OL.global_contrast(G, xg, x, B)), loss_circle=float(OL.circle_contrast(G, x, B, order)))
        run = {}
        for key in SA_T_BN:
            mean, uvar = stats[key]
            run[key] = ((1 - momentum) * q[f"{key}.running_mean"] + momentum * mean,
                        (1 - momentum) * q[f"{key}.running_var"] + momentum * uvar)
        rm, rv = q["netR_FC.1.running_mean"], q["netR_FC.1.running_var"]
        for key in ("fc_a", "fc_b"):                                           # view rows first, then the clip rows
            rm = (1 - momentum) * rm + momentum * stats[key][0]
            rv = (1 - momentum) * rv + momentum * stats[key][1]
        run["netR_FC.1"] = (rm, rv)
        out["running"] = run
    del stats, q
    if not backward:
        return out

    def routed(dtype):
        x_, xg_, _, q_, ties_ = forward64(x_rows, centers, sd, G, S, K, dev, routing=routing, grad=True, dtype=dtype)
        lc, lo = OL.global_contrast(G, xg_, x_, B), OL.circle_contrast(G, x_, B, order)
        (lc + lo).backward()
        g = {k: q_[k].grad.detach() for k in q_ if q_[k].grad is not None}
        return g, ties_, x_.detach(), xg_.detach(), float(lc.detach()), float(lo.detach())
    out["g64"], out["ties"], _, _, _, _ = routed(torch.float64)
    g32, _, out["x32"], out["xg32"], out["loss_c32"], out["loss_circle32"] = routed(torch.float32)
    out["g32"] = {k: v.double() for k, v in g32.items()}
    out["adam64"] = adam64(snap, out["g64"], betas)
    return out
