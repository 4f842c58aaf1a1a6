"""The fp64 reference of FusedSGD's update rules (SGD with momentum, LARS) in NumPy, shared by test_optim_sgd_cpu.py (which pins
it against torch.optim.SGD in fp64) and test_gpu_optim_sgd.py (which measures the kernels against it)."""
import numpy as np


def sgd_step(p, g, buf, lr, mu, wd, mask, nesterov, c=1.0, trust=None):
    """One step on lists of arrays, in the arrays' own dtype (fp64 arrays: the reference; fp32 arrays and fp32 scalars: the
    kernel's five lines, one rounding per operation).  g[i] None: the tensor is skipped.  Returns nothing: p and buf change in
    place.  `trust`: one ratio per tensor or None."""
    for i in range(len(p)):
        if g[i] is None:
            continue
        t = p[i].dtype.type
        gc = g[i] * t(c)
        d = gc + t(wd) * p[i] if mask[i] else gc
        d = d * (t(1.0) if trust is None else t(trust[i]))
        buf[i][...] = t(mu) * buf[i] + d
        p[i][...] = p[i] - t(lr) * (d + t(mu) * buf[i] if nesterov else buf[i])


def lars_trust(p, g, mask, eta, wd, c=1.0):
    """eta |p| / (c |g| + wd |p|) per tensor in fp64 on the masked tensors with non-zero norms, else 1 (None gradients: 1)."""
    out = []
    for pi, gi, m in zip(p, g, mask):
        if gi is None:
            out.append(1.0)
            continue
        wn = float(np.sqrt(np.sum(pi.astype(np.float64) ** 2)))
        gn = float(c) * float(np.sqrt(np.sum(gi.astype(np.float64) ** 2)))
        out.append(eta * wn / (gn + wd * wn) if (m and wn > 0 and gn > 0) else 1.0)
    return out


def lars_step(p, g, buf, lr, mu, wd, mask, nesterov, eta, c=1.0):
    sgd_step(p, g, buf, lr, mu, wd, mask, nesterov, c, lars_trust(p, g, mask, eta, wd, c))
