"""Classifier head of supervised fine-tuning: the reference's probe head ``Final_FC``
(linear_classify/fc_model.py:12-25 -- F.normalize(x, dim=1), then Linear) on the encoder's own stacked, view-major
output, and the softmax cross-entropy of its logits.  The normalisation and the loss are the kernels of csrc/cls.hip,
the class probabilities and top-k lists of prediction those of csrc/predict.hip, the Linear layer is
``facl_amd.tail.linear`` (the exact-split MFMA GEMMs).  GPU only: there is no CPU path."""
import torch
import torch.nn as nn

from . import _lib
from . import tail as _tail
from .sa_mlp import _Workspace

FEATURE_DIM = 512          # width of a row of the encoder's stacked output (netR_FC.3)


class _GatherNorm(torch.autograd.Function):
    """(G*B + B, C) stacked rows (row g*B + b = view g of clip b, row G*B + b = the clip's global feature) ->
    (B, (G+1)*C) = F.normalize of the per-clip vector [x_view0 .. x_view(G-1), x_global], the layout
    ``extract_common.extract_batch`` produces, read in place (no permute / cat copy)."""

    @staticmethod
    def forward(ctx, stacked, G, B):
        _lib.require_cuda(stacked)
        stacked = stacked.contiguous()
        R, C = stacked.shape
        if R != G * B + B:
            raise ValueError("stacked has %d rows, expected G*B + B = %d" % (R, G * B + B))
        out = _lib.empty((B, (G + 1) * C), dtype=torch.float32, device=stacked.device)
        inv = _lib.empty((B,), dtype=torch.float32, device=stacked.device)
        _lib.call("facl_cls_gather_norm_fwd", stacked, G, B, C, out, inv, detail="G=%d, B=%d, C=%d" % (G, B, C))
        ctx.save_for_backward(out, inv)
        ctx.dims = (G, B, C)
        return out

    @staticmethod
    def backward(ctx, dout):
        out, inv = ctx.saved_tensors
        G, B, C = ctx.dims
        dout = dout.contiguous()
        dstacked = _lib.empty((G * B + B, C), dtype=torch.float32, device=dout.device)
        _lib.call("facl_cls_gather_norm_bwd", dout, out, inv, G, B, C, dstacked, detail="G=%d, B=%d, C=%d" % (G, B, C))
        return dstacked, None, None


def gather_norm(stacked, G, B):
    return _GatherNorm.apply(stacked, G, B)


class _SoftmaxCE(torch.autograd.Function):
    """Mean cross-entropy of (R, ncls) logits against int32 labels -> (loss (), stats (2) int32): stats[0] = rows whose argmax
    (the lowest class on equal logits) equals the label, stats[1] = rows whose label lies outside [0, ncls).  The gradient
    (softmax - onehot) / R comes out of the forward launch; the backward scales it by the incoming gradient (one elementwise launch)."""

    @staticmethod
    def forward(ctx, logits, labels):
        _lib.require_cuda(logits, labels)
        if logits.dim() != 2 or logits.dtype != torch.float32:
            raise ValueError("logits must be a 2-D float32 tensor (got %s %s)" % (tuple(logits.shape), logits.dtype))
        if logits.stride(1) != 1 or logits.stride(0) < logits.shape[1]:
            logits = logits.contiguous()
        R, ncls = logits.shape
        if labels.dtype != torch.int32 or labels.shape != (R,) or not labels.is_contiguous():
            raise ValueError("labels must be a contiguous int32 tensor of shape (%d,) (got %s %s)" % (R, tuple(labels.shape), labels.dtype))
        dev = logits.device
        ws = _Workspace.get(dev)
        loss = _lib.empty((1,), dtype=torch.float32, device=dev)
        stats = _lib.empty((2,), dtype=torch.int32, device=dev)
        want_grad = ctx.needs_input_grad[0]
        dlogits = _lib.empty((R, ncls), dtype=torch.float32, device=dev) if want_grad else None
        _lib.call("facl_softmax_ce", logits, logits.stride(0), labels, R, ncls, loss, dlogits, stats, ws,
                  detail="R=%d, ncls=%d" % (R, ncls))
        ctx.has_grad = want_grad
        if want_grad:
            ctx.save_for_backward(dlogits)
        ctx.mark_non_differentiable(stats)
        return loss.view(()), stats

    @staticmethod
    def backward(ctx, dloss, _dstats):
        if not ctx.has_grad:
            return None, None
        d, = ctx.saved_tensors
        return d * dloss, None


def softmax_ce(logits, labels):
    return _SoftmaxCE.apply(logits, labels)


def probs_acc(logits, acc=None, first=None):
    """Softmax of (R, ncls) float32 logits in fp64 (csrc/predict.hip), stored into a new (R, ncls) float64 tensor (`acc` None) or
    added to `acc` in place: the sum of the class probabilities over test-time draws.  `first` True with an `acc`: stored into
    it, whatever it held (the first draw into a preallocated tensor).  A row whose maximum is not finite becomes NaN.
    Returns `acc`."""
    _lib.require_cuda(logits, acc)
    if logits.dim() != 2 or logits.dtype != torch.float32:
        raise ValueError("logits must be a 2-D float32 tensor (got %s %s)" % (tuple(logits.shape), logits.dtype))
    if logits.stride(1) != 1 or logits.stride(0) < logits.shape[1]:
        logits = logits.contiguous()
    R, ncls = logits.shape
    first = acc is None if first is None else bool(first)
    if acc is None:
        if not first:
            raise ValueError("first=False needs the acc to add to")
        acc = _lib.empty((R, ncls), dtype=torch.float64, device=logits.device)
    elif acc.dtype != torch.float64 or acc.shape != (R, ncls) or not acc.is_contiguous():
        raise ValueError("acc must be a contiguous float64 tensor of shape (%d, %d) (got %s %s)" % (R, ncls, tuple(acc.shape), acc.dtype))
    _lib.call("facl_cls_probs_acc", logits, logits.stride(0), R, ncls, acc, int(first), detail="R=%d, ncls=%d" % (R, ncls))
    return acc


def topk(acc, ndraws, k, labels=None):
    """The k classes of largest `acc` (R, ncls) float64 per row under (value descending, class ascending) -> (top_p (R, k)
    float32 = acc / ndraws, top_c (R, k) int32, rank (R,) int32 or None without `labels`): rank = the classes that precede the
    label in that order (0 = a top-1 hit), -1 in a NaN row, -2 for a label outside [0, ncls)."""
    _lib.require_cuda(acc, labels)
    if acc.dim() != 2 or acc.dtype != torch.float64 or not acc.is_contiguous():
        raise ValueError("acc must be a contiguous 2-D float64 tensor (got %s %s)" % (tuple(acc.shape), acc.dtype))
    R, ncls = acc.shape
    if labels is not None and (labels.dtype != torch.int32 or labels.shape != (R,) or not labels.is_contiguous()):
        raise ValueError("labels must be a contiguous int32 tensor of shape (%d,) (got %s %s)" % (R, tuple(labels.shape), labels.dtype))
    ndraws, k = int(ndraws), int(k)
    dev = acc.device
    top_p = _lib.empty((R, max(k, 0)), dtype=torch.float32, device=dev)
    top_c = _lib.empty((R, max(k, 0)), dtype=torch.int32, device=dev)
    rank = _lib.empty((R,), dtype=torch.int32, device=dev) if labels is not None else None
    _lib.call("facl_cls_topk", acc, R, ncls, ndraws, k, labels, top_p, top_c, rank,
              detail="R=%d, ncls=%d, ndraws=%d, k=%d" % (R, ncls, ndraws, k))
    return top_p, top_c, rank


class ClipClassifier(nn.Module):
    """Final_FC on the model's stacked output: ``fc.weight`` (num_class, (num_crop+1)*512) ~ N(0, 0.01), zero ``fc.bias`` --
    the keys and the initialisation of ``linear_classify.Final_FC``, so the two load each other's state_dict."""

    def __init__(self, num_crop, num_class):
        super().__init__()
        if not 1 <= num_crop <= 64:
            raise ValueError("num_crop must be in 1..64 (got %d)" % num_crop)
        if not 2 <= num_class <= 1024:
            raise ValueError("num_class must be in 2..1024 (got %d)" % num_class)
        if num_class % 4:
            raise ValueError("num_class must be a multiple of 4 (got %d): the head's data and weight gradients run on "
                             "facl_gemm_dgrad / facl_gemm_wgrad, whose contraction width is a multiple of 4" % num_class)
        self.num_crop, self.num_class = int(num_crop), int(num_class)
        self.fc = nn.Linear((num_crop + 1) * FEATURE_DIM, num_class)      # parameter holder (fc.weight, fc.bias)
        self.fc.weight.data.normal_(mean=0.0, std=0.01)
        self.fc.bias.data.zero_()

    def forward(self, stacked, G, B):
        """(G*B + B, 512) stacked encoder output -> (B, num_class) logits."""
        if G != self.num_crop:
            raise RuntimeError("the head was built for %d views, got G=%d" % (self.num_crop, G))
        return _tail.linear(gather_norm(stacked, G, B), self.fc)

    def loss(self, logits, labels):
        """(mean cross-entropy (), stats (2) int32 = [hits, labels outside [0, num_class)])."""
        return softmax_ce(logits, labels)
