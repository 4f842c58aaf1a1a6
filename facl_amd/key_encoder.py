"""Momentum key encoder for the queue of negative keys (--key_encoder 1).

A second copy of the encoder whose parameters are the running average ``k <- m k + (1 - m) q`` of the trained ones (MoCo's
``encoder_k`` / ``_momentum_update_key_encoder``: parameters only, not buffers), updated by ONE HIP launch per step
(csrc/adam.hip: facl_ema_apply).  It supplies the rows the step stores in the queue, so that the rows of a long queue come from
weights that moved slowly instead of from the encoder as it was on the step that pushed them.  The copy never sees a gradient.
Its BatchNorm follows MoCo's convention: train() whenever the trained model is, batch statistics, its own running buffers and
``steps`` counters, updated by its own forwards."""
import copy

import torch

from . import _lib


class KeyEncoder:
    MAX_TENSORS = _lib.ADAM_MAX_TENSORS

    def __init__(self, netR, momentum):
        momentum = float(momentum)
        if not 0.0 <= momentum < 1.0:
            raise ValueError("the key momentum must be in [0, 1) (got %r)" % momentum)
        self.netR, self.momentum = netR, momentum
        # the last forward's output hangs on the model (a non-leaf tensor: not copyable, and not part of the model)
        stacked = netR.__dict__.pop("_stacked", None)
        try:
            self.key = copy.deepcopy(netR)
        finally:
            if stacked is not None:
                netR._stacked = stacked
        self.key.bn_reduce_fn = None
        for p in self.key.parameters():
            p.requires_grad_(False)
            p.grad = None
        pairs = list(zip(self.key.parameters(), netR.parameters()))
        if not pairs:
            raise ValueError("the model has no parameters")
        if len(pairs) > self.MAX_TENSORS:
            raise ValueError("the key encoder averages at most %d tensors per launch (the model has %d)"
                             % (self.MAX_TENSORS, len(pairs)))
        for k, q in pairs:
            _lib.require_cuda(k, q)
            if k.dtype != torch.float32 or q.dtype != torch.float32 or not k.is_contiguous() or not q.is_contiguous():
                raise TypeError("the key encoder needs contiguous float32 parameters")
        self.nt = len(pairs)
        self._pk, self._p = _lib.ptr_array([k for k, _ in pairs]), _lib.ptr_array([q for _, q in pairs])
        self._n = _lib.int_array([k.numel() for k, _ in pairs])

    def rows(self, xt, yt):
        """The copy's x_global rows (B, C) on the step's grouped input, before the row map of the loss modes; no graph."""
        if self.key.training != self.netR.training:
            self.key.train(self.netR.training)
        with torch.no_grad():
            return self.key(xt, yt, 1)[3]

    def update(self):
        """k <- m k + (1 - m) q over all parameters: one launch on the current stream."""
        _lib.call("facl_ema_apply", self.nt, self._pk, self._p, self._n, self.momentum,
                  detail="nt=%d, m=%r" % (self.nt, self.momentum))

    # ---- state: the copy's own, in the model's format
    def state_dict(self):
        return self.key.state_dict()

    def load_state_dict(self, sd, strict=True):
        return self.key.load_state_dict(sd, strict=strict)

    def _bn_modules(self):
        return [m for m in self.key.modules() if hasattr(m, "count_batch")]

    def snapshot(self):
        return ({k: v.detach().clone() for k, v in self.key.state_dict().items()}, [m.steps for m in self._bn_modules()])

    def restore(self, snap=None):
        """In place (a captured graph holds the addresses); ``None``: the trained model as it stands, which is what a new
        key encoder starts from."""
        if snap is None:
            tensors = self.netR.state_dict()
            steps = [m.steps for m in self.netR.modules() if hasattr(m, "count_batch")]
        else:
            tensors, steps = snap
        with torch.no_grad():
            cur = self.key.state_dict()
            for k, v in tensors.items():
                cur[k].copy_(v)
        for m, n in zip(self._bn_modules(), steps):
            m.steps = n
