"""Plain torch evaluation of the encoder with EVAL-mode BatchNorm (cn3d_model_conbag.py:213-234 after ``.eval()``): every
BatchNorm is the constant affine of its running statistics, so autograd gives the frozen-BatchNorm gradients -- the pre-BN biases
included.  Same interface as helpers.forward64 (the kernel's max-pool indices and ReLU masks from helpers.routing_taps, the same
`ties` bookkeeping); helper module, not collected."""
import numpy as np

BN_EPS = 1e-5
BN_KEYS = ("net3DV_1.1", "net3DV_1.4", "net3DV_1.7", "net3DV_3.1", "net3DV_3.4", "net3DV_3.7", "netR_FC.1")


def bn_eval(y, gamma, beta, running_mean, running_var, eps=BN_EPS):
    """BatchNorm in eval mode over (rows, C): z = (y - running_mean) / sqrt(running_var + eps) * gamma + beta."""
    import torch
    return (y - running_mean) / torch.sqrt(running_var + eps) * gamma + beta


def routed_relu(z, mask, ties, name):
    """relu(z), or z * mask with the kernel's decisions; a decision that differs from z > 0 must be a numerical tie
    (ties[name] = the largest |z| at a differing decision over the layer's mean |z|, as helpers.forward64 records it)."""
    import torch
    if mask is None:
        return torch.relu(z)
    with torch.no_grad():
        diff = mask.view(z.shape) != (z > 0)
        ties[name + "_flips"] = int(diff.sum())
        ties[name] = float((z.abs() * diff).max() / z.abs().mean())
    return z * mask.view(z.shape)


def routed_pool(h3, idx, ties, name):
    """max over dim 1 of (R, L, C), or the gather at the kernel's argmax `idx` (R, C); ties[name] = the largest distance of a
    gathered value from the true maximum relative to max(|max|, mean |activation|)."""
    import torch
    mx = h3.max(dim=1).values
    if idx is None:
        return mx
    got = torch.gather(h3, 1, idx.long().view(h3.shape[0], 1, h3.shape[2])).squeeze(1)
    with torch.no_grad():
        scale = torch.maximum(mx.abs(), h3.abs().mean())
        ties[name] = float(((mx - got).abs() / scale).max())
        ties[name + "_flips"] = int((idx.long().view(h3.shape[0], h3.shape[2]) != h3.argmax(dim=1)).sum())
    return got


def forward64_eval(x_rows, centers, sd, G, S, K, dev, routing=None, grad=False, dtype=None):
    """(P,D) grouped rows / (M*S,3) centres -> (x, x_global, stats, q, ties) like helpers.forward64, BatchNorm in eval mode:
    `sd`'s running statistics are used and `stats` stays empty (there are no batch statistics).  `grad`: every parameter,
    the pre-BN biases too, requires grad."""
    import torch
    dtype = torch.float64 if dtype is None else dtype
    q = {k: torch.as_tensor(v).to(dev).to(dtype) for k, v in sd.items() if np.asarray(v).dtype.kind == "f"}
    if grad:
        for k in q:
            if "running" not in k:
                q[k].requires_grad_(True)
    ties = {}
    r = dict(routing or {})

    def bn(y, key):
        return bn_eval(y, q[key + ".weight"], q[key + ".bias"], q[key + ".running_mean"], q[key + ".running_var"])

    h = x_rows.to(dtype)
    for i, li in enumerate((0, 3, 6)):                                         # net3DV_1 (:43-58)
        W = q["net3DV_1.%d.weight" % li]
        z = bn(h @ W.reshape(W.shape[0], -1).t() + q["net3DV_1.%d.bias" % li], "net3DV_1.%d" % (li + 1))
        # the third layer's ReLU sits behind the max-pool in the kernels (monotone per channel): its decision is pinned there
        h = routed_relu(z, r.get("relu_sa%d" % (i + 1)), ties, "relu_sa%d" % (i + 1)) if i < 2 else z
    C1 = h.shape[1]
    MS = h.shape[0] // K
    pooled = routed_relu(routed_pool(h.view(MS, K, C1), r.get("sa_arg"), ties, "sa"), r.get("relu_sa3"), ties, "relu_sa3")
    h = torch.cat((centers.to(dtype), pooled), dim=1)                           # :219
    for i, li in enumerate((0, 3, 6)):                                         # net3DV_3 (:61-77)
        W = q["net3DV_3.%d.weight" % li]
        z = bn(h @ W.reshape(W.shape[0], -1).t() + q["net3DV_3.%d.bias" % li], "net3DV_3.%d" % (li + 1))
        h = routed_relu(z, r.get("relu_t%d" % (i + 1)), ties, "relu_t%d" % (i + 1)) if i < 2 else z
    C3 = h.shape[1]
    M = MS // S
    B = M // G
    x_pre = routed_relu(routed_pool(h.view(M, S, C3), r.get("seg_arg"), ties, "seg"), r.get("relu_t3"), ties, "relu_t3")   # :222
    xg_pre = routed_pool(x_pre.view(G, B, C3).transpose(0, 1), r.get("view_arg"), ties, "view")                           # :225-226
    fcm = r.get("relu_fc")                                                     # (M + B, C): view rows, then clip rows

    def head(t, key, mask):                                                    # netR_FC (:201-207): both calls share the statistics
        z = bn(t @ q["netR_FC.0.weight"].t() + q["netR_FC.0.bias"], "netR_FC.1")
        a = routed_relu(z, mask, ties, "relu_" + key)
        return a @ q["netR_FC.3.weight"].t() + q["netR_FC.3.bias"]
    x = head(x_pre, "fc_a", None if fcm is None else fcm[:M])
    xg = head(xg_pre, "fc_b", None if fcm is None else fcm[M:])
    return x, xg, {}, q, ties


def shifted_running_stats(sd, stats):
    """A copy of the state dict `sd` whose running statistics sit AWAY from the batch's own: mean = batch mean + 0.1 batch
    standard deviations, variance = 1.3 x the batch variance, from the `stats` of a train-mode helpers.forward64
    ({key: (mean, unbiased variance)}; netR_FC.1 takes the view rows' "fc_a").  A backward that used batch statistics, or kept
    a batch-statistic term, then misses the reference by far more than any tolerance."""
    import torch
    out = {k: (v.clone() if torch.is_tensor(v) else np.array(v)) for k, v in sd.items()}
    for key in BN_KEYS:
        mean, var = stats["fc_a" if key == "netR_FC.1" else key]
        like = torch.as_tensor(sd[key + ".running_mean"])
        out[key + ".running_mean"] = (mean + 0.1 * var.sqrt()).to(like.dtype).cpu()
        out[key + ".running_var"] = (1.3 * var).to(like.dtype).cpu()
    return out
