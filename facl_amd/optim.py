"""Adam for the training step as ONE HIP launch over all parameter tensors (csrc/adam.hip).

Same update as ``torch.optim.Adam(params, lr, betas, eps)`` with weight_decay = 0, amsgrad = False, maximize = False
(cn3d_train_motion_GL.py:180: lr 3e-4, betas (0.5, 0.999), eps 1e-6); the step counter and the learning rate live on
the device, so a captured HIP graph advances its step counter by itself; learning-rate changes reach a replayed graph
through ``sync_lr()``.  Parameters without a gradient are skipped, like torch's.  The betas reach the kernels as fp32, so
``exp_avg_sq`` is torch's with beta2 = fp32(0.999), 1.3e-5 below torch's own; the parameter updates agree to rounding.

The optimizer recipe, every part off by default: ``weight_decay`` (decoupled, ``torch.optim.AdamW``'s update, on
the tensors of ``decay_mask``), ``max_grad_norm`` (``torch.nn.utils.clip_grad_norm_`` over all gradients of the step, the stored
gradients untouched) and a learning rate evaluated ON THE DEVICE from the step counter (``warmup_steps``, ``schedule="cosine"``
over ``decay_steps`` down to ``lr_min``; ``lr_at_step`` is its host closed form).  With all of it off ``step()`` issues
facl_adam_prep + facl_adam_apply as it always did; otherwise [facl_grad_sqnorm when clipping] + facl_adam_prep_ex +
facl_adamw_apply.  The schedule is a function of the saved step counter: state_dict() needs no new entry for it."""
import math

import torch

from . import _lib

SCHEDULES = {"step": 0, "cosine": 1}                      # include/facl_hip.h: FACL_LR_STEP, FACL_LR_COSINE
CHUNK = _lib.ADAM_CHUNK                                   # elements per fp64 partial of facl_grad_sqnorm


def lr_at_step(lr0, t, schedule="step", warmup_steps=0, decay_steps=0, lr_min=0.0):
    """The learning rate facl_adam_prep_ex applies at step `t` (1-based), in the kernel's own fp64 expressions.  `lr0`: the base
    rate -- under "step" whatever the host schedule (lr_for_epoch) supplies for that step.  The warm-up factor min(1, t / W)
    multiplies either schedule; "cosine" runs from lr0 at t = W to lr_min at t = T and stays there.  (The device holds lr0 as
    fp32: pass float(np.float32(lr0)) to reproduce its value to the last bit.)"""
    if schedule not in SCHEDULES:
        raise ValueError("schedule must be one of %s (got %r)" % (sorted(SCHEDULES), schedule))
    t, W, T, lr0, lr_min = float(t), int(warmup_steps), int(decay_steps), float(lr0), float(lr_min)
    warm = min(1.0, t / float(W)) if W > 0 else 1.0
    lr = lr0
    if schedule == "cosine":
        if T <= W:
            raise ValueError("cosine needs decay_steps > warmup_steps (got %d, %d)" % (T, W))
        tp, Tp = max(t - float(W), 0.0), float(T - W)
        lr = lr_min + (lr0 - lr_min) * 0.5 * (1.0 + math.cos(math.pi * min(tp, Tp) / Tp))
    return warm * lr


class FusedAdam:
    MAX_TENSORS = _lib.ADAM_MAX_TENSORS

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decay_mask=None, max_grad_norm=0.0,
                 schedule="step", warmup_steps=0, decay_steps=0, lr_min=0.0):
        """`decay_mask`: one bool per tensor of `params` (True: `weight_decay` applies), or None = the tensors with ndim >= 2
        (weight matrices and convolution kernels; no bias, no BatchNorm gamma / beta).  `max_grad_norm` 0 = no clipping."""
        params = list(params)
        if decay_mask is None:
            decay_mask = [p.ndim >= 2 for p in params]
        decay_mask = [bool(d) for d in decay_mask]
        if len(decay_mask) != len(params):
            raise ValueError("decay_mask has %d entries for %d tensors" % (len(decay_mask), len(params)))
        self.params = [p for p in params if p.requires_grad]
        if not self.params:
            raise ValueError("optimizer got an empty parameter list")
        if len(self.params) > self.MAX_TENSORS:
            raise ValueError("FusedAdam handles at most %d tensors per step" % self.MAX_TENSORS)
        for p in self.params:
            _lib.require_cuda(p)
            if p.dtype != torch.float32 or not p.is_contiguous():
                raise TypeError("FusedAdam needs contiguous float32 CUDA parameters")
        weight_decay, max_grad_norm, lr_min = float(weight_decay), float(max_grad_norm), float(lr_min)
        warmup_steps, decay_steps = int(warmup_steps), int(decay_steps)
        if not weight_decay >= 0.0 or math.isinf(weight_decay):                    # NaN fails the comparison
            raise ValueError("weight_decay must be finite and >= 0 (got %r)" % weight_decay)
        if not max_grad_norm >= 0.0:
            raise ValueError("max_grad_norm must be >= 0, 0 = off (got %r)" % max_grad_norm)
        if schedule not in SCHEDULES:
            raise ValueError("schedule must be one of %s (got %r)" % (sorted(SCHEDULES), schedule))
        if warmup_steps < 0:
            raise ValueError("warmup_steps must be >= 0 (got %d)" % warmup_steps)
        if not lr_min >= 0.0 or math.isinf(lr_min):
            raise ValueError("lr_min must be finite and >= 0 (got %r)" % lr_min)
        if schedule == "cosine" and decay_steps <= warmup_steps:
            raise ValueError("cosine needs decay_steps > warmup_steps (got %d, %d)" % (decay_steps, warmup_steps))
        dev = self.params[0].device
        self.betas, self.eps = (float(betas[0]), float(betas[1])), float(eps)
        self.weight_decay, self.max_grad_norm = weight_decay, max_grad_norm
        self.schedule, self.warmup_steps, self.decay_steps, self.lr_min = schedule, warmup_steps, decay_steps, lr_min
        self.recipe = bool(weight_decay or max_grad_norm or schedule != "step" or warmup_steps)
        self._decay = {p: d for p, d in zip(params, decay_mask) if p.requires_grad}
        self.param_groups = [{"lr": float(lr), "betas": self.betas, "eps": self.eps, "params": self.params}]
        self._lr_host = None
        self._lr = torch.zeros(1, dtype=torch.float32, device=dev)
        self._step = torch.zeros(1, dtype=torch.float32, device=dev)
        # (lr_t / (1 - b1^t), 1 / sqrt(1 - b2^t)) and, written by facl_adam_prep_ex only, (lr_t, clip coefficient, gradient norm)
        self._consts = torch.tensor([0.0, 0.0, 0.0, 1.0, 0.0], dtype=torch.float32, device=dev)
        self._partial = None
        if max_grad_norm:                                     # one fp64 partial per 2048-element chunk of the parameter list
            self._partial = torch.zeros(sum((p.numel() + CHUNK - 1) // CHUNK for p in self.params), dtype=torch.float64, device=dev)
        self.state = {p: {"exp_avg": torch.zeros_like(p), "exp_avg_sq": torch.zeros_like(p)} for p in self.params}

    def zero_grad(self, set_to_none=True):
        for p in self.params:
            if set_to_none:
                p.grad = None
            elif p.grad is not None:
                p.grad.zero_()

    def sync_lr(self):
        """Host -> device copy of ``param_groups[0]["lr"]`` when a schedule changed it.  step() calls it; a captured
        HIP graph holds no such fill, so whoever REPLAYS a graph with this optimizer inside must call it before each
        replay (train_step.GraphedStep does): the fill lands on the replay stream, ahead of the graph."""
        lr = float(self.param_groups[0]["lr"])
        if lr != self._lr_host:                              # host -> device only when the schedule changed it
            self._lr.fill_(lr)
            self._lr_host = lr

    # ---- device scalars of the last step (0-dimensional views: no copy is made here; read them after a synchronisation)
    def grad_norm(self):
        """The global gradient norm before clipping (0 while max_grad_norm is off: it is not computed then)."""
        return self._consts[4]

    def clip_coef(self):
        """min(1, max_grad_norm / (norm + 1e-6)); 1 while max_grad_norm is off."""
        return self._consts[3]

    def current_lr(self):
        """The learning rate the last step applied: the device-side schedule's, else the host-supplied one."""
        return self._consts[2] if self.recipe else self._lr[0]

    @torch.no_grad()
    def step(self):
        self.sync_lr()
        act = [p for p in self.params if p.grad is not None]
        if not act:
            return
        nt = len(act)
        grads = [p.grad if p.grad.is_contiguous() else p.grad.contiguous() for p in act]
        P, G = _lib.ptr_array(act), _lib.ptr_array(grads)
        M = _lib.ptr_array([self.state[p]["exp_avg"] for p in act])
        V = _lib.ptr_array([self.state[p]["exp_avg_sq"] for p in act])
        N = _lib.int_array([p.numel() for p in act])
        if not self.recipe:
            _lib.call("facl_adam_prep", self._lr, self._step, self.betas[0], self.betas[1], self._consts)
            _lib.call("facl_adam_apply", nt, P, G, M, V, N, self._consts, self.betas[0], self.betas[1], self.eps)
            return
        npartial = 0
        if self.max_grad_norm:
            npartial = sum((p.numel() + CHUNK - 1) // CHUNK for p in act)
            _lib.call("facl_grad_sqnorm", nt, G, N, self._partial)
        _lib.call("facl_adam_prep_ex", self._lr, self._step, self.betas[0], self.betas[1], self._partial, npartial,
                  self.max_grad_norm, SCHEDULES[self.schedule], self.warmup_steps, self.decay_steps, self.lr_min, self._consts)
        D = _lib.int_array([self._decay[p] for p in act])
        _lib.call("facl_adamw_apply", nt, P, G, M, V, N, D, self._consts, self.betas[0], self.betas[1], self.eps,
                  self.weight_decay)

    def state_dict(self):
        """torch.optim.Adam's layout (state by parameter index), so either optimizer can resume the other's run."""
        step = self._step.detach().clone().cpu()[0]
        return {"state": {i: {"step": step.clone(), "exp_avg": self.state[p]["exp_avg"], "exp_avg_sq": self.state[p]["exp_avg_sq"]}
                          for i, p in enumerate(self.params)},
                "param_groups": [{"lr": self.param_groups[0]["lr"], "betas": self.betas, "eps": self.eps,
                                  "weight_decay": self.weight_decay or 0, "amsgrad": False, "params": list(range(len(self.params)))}]}

    def load_state_dict(self, sd):
        for i, p in enumerate(self.params):
            s = sd["state"].get(i)
            if s is None:
                continue
            self.state[p]["exp_avg"].copy_(s["exp_avg"])
            self.state[p]["exp_avg_sq"].copy_(s["exp_avg_sq"])
            self._step.fill_(float(s["step"]))
        self.param_groups[0]["lr"] = sd["param_groups"][0]["lr"]


class FusedSGD:
    """SGD with momentum, and LARS, as ONE update launch over all parameter tensors (csrc/adam.hip).

    ``torch.optim.SGD(params, lr, momentum, dampening=0, nesterov=...)`` with L2 ``weight_decay`` on the tensors of ``decay_mask``
    only; ``lars=True`` multiplies every masked tensor's decayed gradient by its trust ratio ``lars_eta |p| / (|g| + wd |p|)`` in
    front of the momentum (You et al.'s layer-wise rate as SimCLR applies it: one mask keeps biases and BatchNorm out of both the
    decay and the adaptation).  The surface is FusedAdam's: the step counter and the rate live on the device, ``max_grad_norm``
    and the schedule are evaluated there by the same expressions, ``sync_lr()`` carries a host change to a replayed graph.
    Launches per step: facl_sgd_prep + facl_sgd_apply, with facl_grad_sqnorm in front when clipping and facl_tensor_sqnorms in
    front under LARS (its gradient partials serve the clip too).  Parameters without a gradient are skipped."""
    MAX_TENSORS = _lib.ADAM_MAX_TENSORS

    def __init__(self, params, lr=1e-3, momentum=0.9, nesterov=False, weight_decay=0.0, decay_mask=None, lars=False,
                 lars_eta=1e-3, max_grad_norm=0.0, schedule="step", warmup_steps=0, decay_steps=0, lr_min=0.0):
        """`decay_mask`: one bool per tensor of `params` (True: `weight_decay` and, under `lars`, the trust ratio apply), or None
        = the tensors with ndim >= 2.  `max_grad_norm` 0 = no clipping."""
        params = list(params)
        if decay_mask is None:
            decay_mask = [p.ndim >= 2 for p in params]
        decay_mask = [bool(d) for d in decay_mask]
        if len(decay_mask) != len(params):
            raise ValueError("decay_mask has %d entries for %d tensors" % (len(decay_mask), len(params)))
        self.params = [p for p in params if p.requires_grad]
        if not self.params:
            raise ValueError("optimizer got an empty parameter list")
        if len(self.params) > self.MAX_TENSORS:
            raise ValueError("FusedSGD handles at most %d tensors per step" % self.MAX_TENSORS)
        for p in self.params:
            _lib.require_cuda(p)
            if p.dtype != torch.float32 or not p.is_contiguous():
                raise TypeError("FusedSGD needs contiguous float32 CUDA parameters")
        momentum, weight_decay, lars_eta = float(momentum), float(weight_decay), float(lars_eta)
        max_grad_norm, lr_min = float(max_grad_norm), float(lr_min)
        warmup_steps, decay_steps = int(warmup_steps), int(decay_steps)
        if not 0.0 <= momentum < 1.0:                                              # NaN fails both comparisons
            raise ValueError("momentum must be in [0, 1) (got %r)" % momentum)
        if not weight_decay >= 0.0 or math.isinf(weight_decay):
            raise ValueError("weight_decay must be finite and >= 0 (got %r)" % weight_decay)
        if not lars_eta >= 0.0 or math.isinf(lars_eta) or (lars and not lars_eta > 0.0):
            raise ValueError("lars_eta must be finite and %s (got %r)" % ("> 0 under lars" if lars else ">= 0", lars_eta))
        if not max_grad_norm >= 0.0:
            raise ValueError("max_grad_norm must be >= 0, 0 = off (got %r)" % max_grad_norm)
        if schedule not in SCHEDULES:
            raise ValueError("schedule must be one of %s (got %r)" % (sorted(SCHEDULES), schedule))
        if warmup_steps < 0:
            raise ValueError("warmup_steps must be >= 0 (got %d)" % warmup_steps)
        if not lr_min >= 0.0 or math.isinf(lr_min):
            raise ValueError("lr_min must be finite and >= 0 (got %r)" % lr_min)
        if schedule == "cosine" and decay_steps <= warmup_steps:
            raise ValueError("cosine needs decay_steps > warmup_steps (got %d, %d)" % (decay_steps, warmup_steps))
        dev = self.params[0].device
        self.momentum, self.nesterov, self.weight_decay = momentum, bool(nesterov), weight_decay
        self.lars, self.lars_eta, self.max_grad_norm = bool(lars), lars_eta, max_grad_norm
        self.schedule, self.warmup_steps, self.decay_steps, self.lr_min = schedule, warmup_steps, decay_steps, lr_min
        self._decay = {p: d for p, d in zip(params, decay_mask) if p.requires_grad}
        self.param_groups = [{"lr": float(lr), "momentum": momentum, "dampening": 0, "weight_decay": weight_decay,
                              "nesterov": self.nesterov, "params": self.params}]
        self._lr_host = None
        self._lr = torch.zeros(1, dtype=torch.float32, device=dev)
        self._step = torch.zeros(1, dtype=torch.float32, device=dev)
        self._consts = torch.tensor([0.0, 0.0, 0.0, 1.0, 0.0], dtype=torch.float32, device=dev)     # (lr_t, 0, lr_t, c, norm)
        self._trust = torch.ones(len(self.params), dtype=torch.float32, device=dev)
        chunks = sum((p.numel() + CHUNK - 1) // CHUNK for p in self.params)      # one fp64 partial per 2048-element chunk
        self._partial_g = torch.zeros(chunks, dtype=torch.float64, device=dev) if (max_grad_norm or lars) else None
        self._partial_p = torch.zeros(chunks, dtype=torch.float64, device=dev) if lars else None
        self.state = {p: {"momentum_buffer": torch.zeros_like(p)} for p in self.params}

    zero_grad = FusedAdam.zero_grad
    sync_lr = FusedAdam.sync_lr
    grad_norm = FusedAdam.grad_norm
    clip_coef = FusedAdam.clip_coef

    def current_lr(self):
        """The learning rate the last step applied (a 0-dimensional device view)."""
        return self._consts[2]

    def trust_ratios(self):
        """A device view of one float per tensor of the last step, in its order (the parameters that had a gradient): LARS's
        trust ratio, 1 on the unmasked tensors and on those whose weight or gradient norm is 0; all 1 for plain SGD."""
        return self._trust[:len(self.last_mask)] if self.last_mask else self._trust

    last_mask = ()                                            # the mask flags of the last step's tensors, in its order

    @torch.no_grad()
    def step(self):
        self.sync_lr()
        act = [p for p in self.params if p.grad is not None]
        if not act:
            return
        nt = len(act)
        self.last_mask = [bool(self._decay[p]) for p in act]
        grads = [p.grad if p.grad.is_contiguous() else p.grad.contiguous() for p in act]
        P, G = _lib.ptr_array(act), _lib.ptr_array(grads)
        B = _lib.ptr_array([self.state[p]["momentum_buffer"] for p in act])
        N = _lib.int_array([p.numel() for p in act])
        D = _lib.int_array([self._decay[p] for p in act])
        clip = bool(self.max_grad_norm)
        npartial = sum((p.numel() + CHUNK - 1) // CHUNK for p in act) if (clip or self.lars) else 0
        if self.lars:
            _lib.call("facl_tensor_sqnorms", nt, P, G, N, self._partial_p, self._partial_g)
        elif clip:
            _lib.call("facl_grad_sqnorm", nt, G, N, self._partial_g)
        trust = self._trust if self.lars else None
        _lib.call("facl_sgd_prep", self._lr, self._step, self._partial_g, self._partial_p, npartial, nt, N, D,
                  self.max_grad_norm, int(clip), SCHEDULES[self.schedule], self.warmup_steps, self.decay_steps, self.lr_min,
                  self.lars_eta, self.weight_decay, self._consts, trust)
        _lib.call("facl_sgd_apply", nt, P, G, B, N, D, self._consts, trust, self.momentum, self.weight_decay, int(self.nesterov))

    def state_dict(self):
        """torch.optim.SGD's layout (momentum_buffer by parameter index; lr, momentum, dampening 0, weight_decay, nesterov in the
        group) plus a `step` per entry, from which the device-side schedule continues."""
        step = self._step.detach().clone().cpu()[0]
        return {"state": {i: {"step": step.clone(), "momentum_buffer": self.state[p]["momentum_buffer"]}
                          for i, p in enumerate(self.params)},
                "param_groups": [{"lr": self.param_groups[0]["lr"], "momentum": self.momentum, "dampening": 0,
                                  "weight_decay": self.weight_decay, "nesterov": self.nesterov,
                                  "params": list(range(len(self.params)))}]}

    def load_state_dict(self, sd):
        for i, p in enumerate(self.params):
            s = sd["state"].get(i)
            if s is None:
                continue
            self.state[p]["momentum_buffer"].copy_(s["momentum_buffer"])
            self._step.fill_(float(s["step"]))
        self.param_groups[0]["lr"] = sd["param_groups"][0]["lr"]
