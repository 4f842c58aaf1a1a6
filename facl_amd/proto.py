"""Prototype contrastive term on the k-means centroids.  The reference has no counterpart: this is ProtoNCE (Li et al.
2021, "Prototypical Contrastive Learning") on the centroids that --class_ids cluster computes anyway.  Every row of the model's
stacked output is pulled toward the centroid of its clip's cluster and pushed from the other K - 1, each cluster with a
temperature from its own concentration.

``proto_nce`` is one fused launch (csrc/proto.hip: loss and d loss / d stacked in one pass over the rows) plus a one-wave
finishing launch; GPU only, there is no CPU path.  ``concentrations`` is host NumPy in fp64, an evaluation path like the scores
of cluster.py."""
import numpy as np
import torch

from . import _lib

K_MAX = 1024
C_MAX = 512

# (device, stream, M, C, K) -> (dstacked, loss, ws, err): allocated once and reused, so that a captured step replays against static
# memory.  NOT the stream's shared scratch workspace: the query forward leaves there what its backward reads
# (train_step.ContrastiveStep._encode_and_step), and this term runs between the two.
_BUFFERS = {}


def buffers(dev, M, C, K):
    """(dstacked (M, C), loss (1), workspace, err (1) int32) of the current stream for these sizes, created on first use.  err is
    sticky: the kernel ORs bit 0 into it for a class id >= K, and only ``raise_if_err`` clears it."""
    key = (dev.index, _lib.stream(), M, C, K)
    buf = _BUFFERS.get(key)
    if buf is None:
        nbytes = _lib.call_size("facl_proto_nce_ws_bytes", M, detail="M=%d" % M)
        buf = (_lib.empty((M, C), dtype=torch.float32, device=dev), _lib.empty((1,), dtype=torch.float32, device=dev),
               _lib.empty(((nbytes + 7) // 8,), dtype=torch.float64, device=dev), torch.zeros((1,), dtype=torch.int32, device=dev))
        _BUFFERS[key] = buf
    return buf


def raise_if_err(err, K, what="proto_nce"):
    """Reads the word (a host round trip: never inside a captured step), clears it, and raises naming the range."""
    e = int(err.item())
    if e:
        err.zero_()
        raise RuntimeError("%s: a class id lies outside the range [0, %d) of the prototypes (>= %d: err %d); its rows were "
                           "treated as unknown" % (what, K, K, e))


class _ProtoNCE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, stacked, classes, protos, proto_inv, scale):
        _lib.require_cuda(stacked, classes, protos, proto_inv, scale)
        if stacked.dim() != 2 or stacked.dtype != torch.float32:
            raise ValueError("stacked must be a 2-D float32 tensor (got %s %s)" % (tuple(stacked.shape), stacked.dtype))
        if stacked.stride(1) != 1 or stacked.stride(0) < stacked.shape[1] or stacked.stride(0) % 4:
            stacked = stacked.contiguous()
        M, C = stacked.shape
        if classes.dtype != torch.int32 or classes.dim() != 1 or not classes.is_contiguous() or classes.shape[0] < 1 \
                or M % classes.shape[0]:
            raise ValueError("classes must be a contiguous int32 (B,) tensor with B dividing the %d rows (got %s %s)"
                             % (M, classes.dtype, tuple(classes.shape)))
        B = classes.shape[0]
        if protos.dtype != torch.float32 or protos.dim() != 2 or protos.shape[1] != C or not protos.is_contiguous():
            raise ValueError("protos must be a contiguous float32 (K, %d) matrix (got %s %s)" % (C, protos.dtype, tuple(protos.shape)))
        K = protos.shape[0]
        for t, what in ((proto_inv, "proto_inv"), (scale, "scale")):
            if t.dtype != torch.float32 or tuple(t.shape) != (K,) or not t.is_contiguous():
                raise ValueError("%s must be contiguous float32 (%d,) (got %s %s)" % (what, K, t.dtype, tuple(t.shape)))
        dev = stacked.device
        with torch.cuda.device(dev):
            dstacked, loss, ws, err = buffers(dev, M, C, K)
            _lib.call("facl_proto_nce", stacked, M, stacked.stride(0), C, B, classes, protos, proto_inv, scale, K, loss,
                      dstacked, err, ws, detail="M=%d, C=%d, B=%d, K=%d" % (M, C, B, K))
        ctx.save_for_backward(dstacked)
        ctx.mark_non_differentiable(err)
        return loss.view(()), err

    @staticmethod
    def backward(ctx, dloss, _derr):
        d, = ctx.saved_tensors
        return d * dloss, None, None, None, None


def proto_nce_raw(stacked, classes, protos, proto_inv, scale):
    """(loss (), err (1) int32) without a host read-back: what a captured step calls.  The loss and the gradient live in buffers
    owned per (stream, M, C, K): a second call with the same sizes on the same stream overwrites the first one's."""
    return _ProtoNCE.apply(stacked, classes, protos, proto_inv, scale)


def proto_nce(stacked, classes, protos, proto_inv, scale):
    """The ProtoNCE term of (M, C) float32 rows `stacked` (row r belongs to clip r % B) against K prototypes -> scalar loss

        (1/M) sum over the rows r with 0 <= classes[r % B] < K of  logsumexp_k l_rk - l_{r, classes[r % B]},
        l_rk = scale_k <x_r / max(||x_r||, 1e-12), protos_k proto_inv_k>.

    classes (B) int32, negative = unknown: such a row adds nothing and still counts in M.  protos (K, C) un-normalised
    centroids, proto_inv (K) = cluster.row_inv(protos), scale (K) = 1 / phi_k (``concentrations``).  The prototypes are constants:
    only `stacked` receives a gradient, which the forward launch has already formed.  An id >= K raises, naming the range (the
    eager wrapper reads the kernel's err word; inside a captured step use ``proto_nce_raw``)."""
    loss, err = _ProtoNCE.apply(stacked, classes, protos, proto_inv, scale)
    if not torch.cuda.is_current_stream_capturing():
        raise_if_err(err, protos.shape[0])
    return loss


# ---- host: the concentration of every cluster (plain NumPy, fp64) -----------------------------------------------------------------
def concentrations(cos_own, labels, K, temperature=0.2, mode="cluster"):
    """scale (K,) float32 = 1 / phi_k.  mode 'fixed': phi_k = temperature.  mode 'cluster' (PCL): with d_i = sqrt(max(0, 2 - 2 cos_i))
    the distance of unit row i to its own unit centroid and Z_k the size of cluster k, phi_k = mean_{i in k} d_i / log(Z_k + 10);
    a cluster without rows, or with phi_k = 0, takes the largest phi of the others (all of them such: 1); then phi is clipped to
    its [10th, 90th] percentile (linear interpolation) and scaled so that mean(phi) = temperature."""
    K = int(K)
    temperature = float(temperature)
    if K < 1:
        raise ValueError("K must be >= 1 (got %d)" % K)
    if not (temperature > 0.0 and np.isfinite(temperature)):
        raise ValueError("temperature must be finite and > 0 (got %r)" % temperature)
    if mode == "fixed":
        return np.full((K,), 1.0 / temperature, dtype=np.float32)
    if mode != "cluster":
        raise ValueError("mode must be 'cluster' or 'fixed' (got %r)" % (mode,))
    cos = np.asarray(cos_own, dtype=np.float64).reshape(-1)
    lab = np.asarray(labels).astype(np.int64).reshape(-1)
    if cos.shape != lab.shape:
        raise ValueError("cos_own and labels differ in length (%d, %d)" % (cos.shape[0], lab.shape[0]))
    if lab.size and (lab.min() < 0 or lab.max() >= K):
        raise ValueError("labels must lie in [0, %d)" % K)
    d = np.sqrt(np.maximum(0.0, 2.0 - 2.0 * cos))
    Z = np.bincount(lab, minlength=K).astype(np.float64)
    phi = np.bincount(lab, weights=d, minlength=K) / np.maximum(Z, 1.0) / np.log(Z + 10.0)
    dead = (Z == 0) | ~(phi > 0.0)
    phi[dead] = phi[~dead].max() if (~dead).any() else 1.0
    phi = np.clip(phi, np.percentile(phi, 10), np.percentile(phi, 90))
    phi = phi * (temperature / phi.mean())
    return (1.0 / phi).astype(np.float32)
