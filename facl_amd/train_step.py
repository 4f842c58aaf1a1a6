"""The training iteration: the frame every step shares, the grouper of two of them, the contrastive step, the HIP-graph replay."""
import functools
import os
import time

import numpy as np
import torch

from . import dist as fdist
from .train_flags import with_defaults
from .utils_my import check_class_positives, contrastive_losses_stacked, group_points_3DV, is_default_loss_mode, knn_radius_group


def group_views(data1, opt, r2=None):
    """The grouper of training and extraction over view-major (M,N,D) rows (the second path: or a clip-major (B,G,N,D)
    batch).  `r2` None: the reference's literals, K=64 and r^2=0.06 at N=512 (:230), group_points_3DV_2048's 0.16 otherwise."""
    if r2 is None and opt.SAMPLE_NUM == 512:
        return group_points_3DV(data1, opt)
    opt.INPUT_FEATURE_NUM = data1.shape[-1]
    return knn_radius_group(data1, opt.sample_num_level1, opt.knn_K, 0.16 if r2 is None else r2)


def draw_order(G, order=None):
    """The circle loss's permutation (:297-298) when none is given: ONE shuffle from NumPy's global stream, which a resume state captures."""
    if order is None:
        order = np.arange(0, G, 1)
        np.random.shuffle(order)
    return order


class TrainStep:
    """What every training iteration has; a subclass defines `run(out_points, order)`, the device-only body (no host round trips)
    that GraphedStep captures, and says what a replay of it must carry besides model and optimizer (`encoders`, `carried_state`)."""

    def __init__(self, netR, optimizer, num_crop):
        self.netR, self.optimizer, self.G = netR, optimizer, num_crop
        self.epoch, self._one = 0, None
        self.rank = torch.distributed.get_rank() if fdist.is_distributed() else 0
        self.grad_sync = fdist.GradSync(list(netR.named_parameters())) if fdist.is_distributed() else None

    def __call__(self, out_points, epoch=0, order=None):
        order = draw_order(self.G, order)
        if not torch.is_tensor(order):
            order = torch.as_tensor(np.asarray(order), dtype=torch.long).to(out_points.device)
        self.epoch = epoch
        return self.run(out_points, order)

    def backward_and_update(self, loss):
        self.optimizer.zero_grad(set_to_none=True)
        if self._one is None or self._one.device != loss.device:
            self._one = torch.ones((), dtype=torch.float32, device=loss.device)    # the seed of backward(): no fill launch per step
        loss.backward(self._one)
        if self.grad_sync is not None:
            self.grad_sync.finish()                                                # tail bucket overlapped with the SA backward
        self.optimizer.step()

    # ---- what a replay (GraphedStep) and the epoch loop must know about the step besides model and optimizer
    def encoders(self):
        """The networks whose BatchNorm layers count their batches on the host, and which an epoch switches to train()."""
        return [self.netR]

    def carried_state(self):
        """{name: object with snapshot() / restore(snap), or None while it does not exist} of what the step keeps between iterations."""
        return {}


class GroupedStep(TrainStep):
    """A step whose encoder takes grouped views: the reference's grouper (and the optional FPS reorder) in front of it."""

    def __init__(self, netR, optimizer, opt, num_crop, group_radius=None, fps_reorder=False):
        super().__init__(netR, optimizer, num_crop)
        self.opt, self.r2, self.fps_reorder = opt, group_radius, fps_reorder

    def group(self, data1):
        return group_views(data1, self.opt, self.r2)

    def grouped(self, out_points):
        """(xt, yt, clips) of `out_points`: the loader's clip-major (B,G,N,D) batch, or -- 3-dimensional -- the view-major
        (G*B,N,D) rows that facl_amd.views.build_views writes directly (the permute + reshape of :226 already done)."""
        if out_points.dim() == 3:
            B = out_points.shape[0] // self.G
            data1 = out_points if out_points.dtype == torch.float32 else out_points.float()
        else:
            B, _, N, D = out_points.shape
            data1 = out_points                     # clip-major batch: the grouping kernel reads view-major in place ...
            if self.fps_reorder or out_points.dtype != torch.float32 or (self.r2 is None and self.opt.SAMPLE_NUM == 512):
                data1 = out_points.permute(1, 0, 2, 3).reshape(-1, N, D).float()  # ... or :226-228 (view-major rows)
        if self.fps_reorder:                                                       # FPS picks first (start index 0)
            from .fps import fps_sample_data
            data1 = fps_sample_data(data1, self.opt.sample_num_level1,
                                    start_idx=torch.zeros(data1.shape[0], dtype=torch.int32, device=data1.device))
        return self.group(data1) + (B,)


class ContrastiveStep(GroupedStep):
    """One training iteration = the loop body of cn3d_train_motion_GL.py:224-335."""

    def __init__(self, netR, optimizer, opt, num_crop, group_radius=None, fps_reorder=False, swa_if=0, cld_if=0):
        super().__init__(netR, optimizer, opt, num_crop, group_radius, fps_reorder)
        self.swa_if, self.cld_if, self.swav_state = int(swa_if), int(cld_if), None
        flags = with_defaults(opt)                 # a namespace from before a flag holds the parser's default: the reference's loss
        # loss modes (utils_my.contrastive_losses_stacked)
        self.loss_mode = dict(normalize=bool(flags.loss_normalize), temperature=float(flags.loss_temperature), mask=flags.loss_mask)
        # cross-batch queue of negative keys (facl_amd/neg_queue.py): created on the first step, pushed at the end of every step
        self.neg_queue, self.queue = int(flags.neg_queue), None
        if self.neg_queue and fdist.is_distributed():
            raise RuntimeError("the negative queue runs on one rank only")
        # class-aware mask: the class ids of the batch's clips (< 0: unknown), a static tensor that the caller fills in place
        # before each call (like FineTuneStep.labels), so that a replayed graph reads the current batch's
        self.clip_classes = None
        if self.loss_mode["mask"] == "class":
            if fdist.is_distributed():
                raise RuntimeError("the class-aware loss mask runs on one rank only")
            self.clip_classes = torch.full((int(opt.batchSize),), -1, dtype=torch.int32, device=next(netR.parameters()).device)
        # momentum key encoder (facl_amd/key_encoder.py): created on the first step; its rows are the ones the queue stores
        self.key_momentum = float(flags.key_momentum) if int(flags.key_encoder) else None
        self.key_encoder = None
        if self.key_momentum is not None and not self.neg_queue:
            raise RuntimeError("the key encoder supplies the rows of the negative queue: it needs neg_queue > 0")
        # class-mates as extra positives (utils_my: class_positives); beside loss_mode, which stays the dict of the three modes
        self.class_positives = check_class_positives(flags.class_positives, self.loss_mode["mask"])
        # prototype contrastive term (facl_amd/proto.py): static tensors that the caller fills in place after every clustering
        # (set_prototypes), so that a replayed graph reads the current centroids; zeros / ones do nothing while every id is -1
        self.proto_weight = float(flags.proto_weight)
        self.prototypes = self.proto_inv = self.proto_scale = self.proto_err = None
        if self.proto_weight > 0:
            if self.clip_classes is None:
                raise RuntimeError("the prototype term reads the clips' cluster ids: it needs the class-aware loss mask")
            from .cls_head import FEATURE_DIM
            dev, K = self.clip_classes.device, int(opt.clusters)
            self.prototypes = torch.zeros((K, FEATURE_DIM), dtype=torch.float32, device=dev)
            self.proto_inv = torch.ones((K,), dtype=torch.float32, device=dev)
            self.proto_scale = torch.ones((K,), dtype=torch.float32, device=dev)

    def set_prototypes(self, centroids, scale):
        """After a clustering: the (K, 512) centroids and their (K,) scales 1 / phi_k go IN PLACE into the step's static tensors."""
        from .cluster import row_inv
        self.prototypes.copy_(centroids)
        self.proto_inv.copy_(row_inv(self.prototypes))
        self.proto_scale.copy_(torch.as_tensor(scale, dtype=torch.float32))

    def check_proto_err(self):
        """Outside the step (a host read-back): raises when a clip's id was >= K since the last check."""
        if self.proto_err is not None:
            from .proto import raise_if_err
            raise_if_err(self.proto_err, self.prototypes.shape[0], "--proto_weight")

    def encoders(self):
        """The model and, once it exists, the key copy (MoCo's convention: it normalises with batch statistics too)."""
        return [self.netR] + ([] if self.key_encoder is None else [self.key_encoder.key])

    def carried_state(self):
        """Both are created by the first step; restore(None) empties the queue / sets the key copy equal to the model AS RESTORED."""
        return {"queue": self.queue, "key_encoder": self.key_encoder}

    # ---- the state the step keeps between iterations besides model and optimizer (facl_amd/train_state.py)
    def state_dict(self):
        """{queue: {buf, state}, key_encoder: its state_dict, swav: {queue, filled}}, each None while it does not exist.  The
        tensors are the live ones (like FusedAdam.state_dict()'s moments): train_state.assemble copies them."""
        queue = None if self.queue is None else {"buf": self.queue.buf, "state": self.queue.state}
        if queue is not None and self.queue.ids is not None:
            queue["ids"] = self.queue.ids
        key = None if self.key_encoder is None else self.key_encoder.state_dict()
        sw = self.swav_state
        swav = None if sw is None or sw.queue is None else {"queue": sw.queue, "filled": int(sw.filled)}
        return {"queue": queue, "key_encoder": key, "swav": swav}

    def load_state_dict(self, sd):
        """Creates queue, key encoder and SwAV queue HERE, before the first batch: the step itself creates them lazily, and
        GraphedStep(restore=True) takes a queue or key encoder that does not exist yet for "empty" / "equal to the model" and
        restores exactly that after its warm-up steps."""
        device = next(self.netR.parameters()).device
        B = self.opt.batchSize
        if sd["queue"] is not None:
            from .neg_queue import NegativeQueue
            buf = sd["queue"]["buf"]
            if buf.dim() != 2 or buf.shape[0] != self.neg_queue:
                raise RuntimeError("the saved queue holds %s rows, this step --neg_queue %d" % (tuple(buf.shape)[:1], self.neg_queue))
            with_ids = self.loss_mode["mask"] == "class"
            if with_ids and sd["queue"].get("ids") is None:
                raise RuntimeError("the saved queue holds no class ids of its rows (ids): a run with --loss_mask class needs them")
            self.queue = NegativeQueue(buf.shape[0], buf.shape[1], B, device, with_ids=with_ids)
            self.queue.restore((buf.to(device), sd["queue"]["state"].to(device))
                               + ((sd["queue"]["ids"].to(device),) if with_ids else ()))
        if sd["key_encoder"] is not None:
            if self.key_momentum is None:
                raise RuntimeError("the state holds a key encoder, this step runs with --key_encoder 0")
            from .key_encoder import KeyEncoder
            self.key_encoder = KeyEncoder(self.netR, self.key_momentum)
            self.key_encoder.load_state_dict(sd["key_encoder"], strict=True)  # the BatchNorm `steps`: num_batches_tracked's load hook
        if sd["swav"] is not None:
            from . import swav_cld
            q = sd["swav"]["queue"]
            if self.swav_state is None:
                self.swav_state = swav_cld.SwavState(B, self.G, q.shape[2], queue_length=q.shape[1])
            sw = self.swav_state
            if tuple(q.shape) != (sw.G - 1, sw.queue_length, sw.dim):
                raise RuntimeError("the saved SwAV queue is %s, this step's %s" % (tuple(q.shape), (sw.G - 1, sw.queue_length, sw.dim)))
            sw.queue = q.to(device).clone()
            sw.filled = int(sd["swav"]["filled"])

    def run(self, out_points, order):
        xt, yt, B = self.grouped(out_points)
        out = self._encode_and_step(xt, yt, B, order)
        if self.key_encoder is not None:
            self.key_encoder.update()              # after Adam: the average MoCo takes at the start of the next step
        if self.queue is not None:
            self.queue.push()                      # this step's x_global rows, after the backward has read the queue
        return out

    def _encode_and_step(self, xt, yt, B, order):
        netR, G = self.netR, self.G
        # The key forward runs BEFORE the query forward: the passes share the stream's scratch workspace, and the query forward
        # leaves there (and in what autograd saved) what its backward reads -- nothing may run between the two
        key_rows = None
        if self.key_momentum is not None:
            if self.key_encoder is None:
                from .key_encoder import KeyEncoder
                self.key_encoder = KeyEncoder(netR, self.key_momentum)
            key_rows = self.key_encoder.rows(xt, yt)
        x, code, x_nor, x_global = netR(xt, yt, 1)                                 # :234
        if fdist.is_distributed() and not is_default_loss_mode(**self.loss_mode):
            # the loss modes map the rows first: this rank's view rows are normalised / scaled locally, THEN gathered
            x_keys = lambda n_views: fdist.all_gather_view_major(n_views, G)
        else:
            x_keys = fdist.all_gather_view_major(x, G)
        off = self.rank * B
        if self.neg_queue and self.queue is None:
            from .neg_queue import NegativeQueue
            self.queue = NegativeQueue(self.neg_queue, netR._stacked.shape[1], B, netR._stacked.device,
                                       with_ids=self.clip_classes is not None)
        if self.clip_classes is not None and B != self.clip_classes.shape[0]:
            raise RuntimeError("a batch of %d clips, the step holds %d class ids" % (B, self.clip_classes.shape[0]))
        # global (:265-287) + circle (:290-316) losses: similarity GEMMs + one HIP kernel each (csrc/loss.hip)
        from .tail import precision as _precision
        with _precision(getattr(netR, "precision", "f32")):    # the similarity GEMMs follow the model's arithmetic
            loss_c, loss_circle, loss = contrastive_losses_stacked(G, netR._stacked, order, x_keys=None if x_keys is x else x_keys,
                                                                   clip_offset=off, with_sum=True, **self.loss_mode,
                                                                   **({} if self.queue is None else {"queue": self.queue}),
                                                                   **({} if self.clip_classes is None else {"classes": self.clip_classes}),
                                                                   **({} if not self.class_positives else {"class_positives": self.class_positives}),
                                                                   **({} if key_rows is None else {"queue_rows": key_rows}))
        # loss = loss_circle + loss_c (:329; swa, CLD terms are 0 ...): the fp32 sum comes out of the loss launch itself
        if self.swa_if:                                                            # ... unless switched on: :239-263
            from . import swav_cld
            if self.swav_state is None:
                self.swav_state = swav_cld.SwavState(B, G, x_nor.shape[1])
            self.swav_state.maybe_create(self.epoch, x.device)
            loss = loss + 0.6 * swav_cld.swav_loss(code, x_nor, netR.mapping.weight, self.swav_state)
        if self.cld_if:                                                            # :319-326
            from . import swav_cld
            loss = loss + swav_cld.cld_loss(x_nor, B, G)
        if self.proto_weight > 0:                                                  # no counterpart in the reference
            from .proto import proto_nce_raw
            loss_p, self.proto_err = proto_nce_raw(netR._stacked, self.clip_classes, self.prototypes, self.proto_inv, self.proto_scale)
            loss = loss + self.proto_weight * loss_p
        self.backward_and_update(loss)
        return loss, loss_c, loss_circle


class GraphCaptureFailed(RuntimeError):
    """The step could not be captured (or its replay did not reproduce the eager step).  Model, BatchNorm buffers and
    optimizer state are back at their values from before the attempt.  Under data parallelism EVERY rank raises it at the
    same point of the collective sequence (facl_amd/dist.py: GraphSegments' failure protocol), so all ranks may continue
    together on eager launches; any other exception out of GraphedStep under world > 1 is not agreed on and must end the rank."""


@functools.lru_cache(maxsize=None)
def _capture_stream(dev):
    """One side stream per device for warm-up + capture (the scratch workspace of the HIP passes is keyed by stream:
    a fresh stream per GraphedStep would pin another workspace each time)."""
    return torch.cuda.Stream(device=dev)


class GraphedStep:
    """The whole training iteration (grouping -> forward -> losses -> backward -> Adam) of a TrainStep captured once into a HIP
    graph and replayed: ~250 kernel launches per step collapse into one graph launch, so the step is no longer bound
    by host launch latency.  Under data parallelism the capture is cut at every collective and the kernel segments between
    them replay as graphs (collectives stay eager: facl_amd/dist.py: GraphSegments); the optimizer must keep its step counter on the device
    (facl_amd.optim.FusedAdam, or torch.optim.Adam(capturable=True, lr=<tensor>)).  Learning-rate changes between
    replays: FusedAdam's device-side lr is refreshed before every replay (`sync_lr`); with torch's capturable Adam only
    a TENSOR lr updated in place is seen by the graph.

    Failure: GraphCaptureFailed, with the training state restored (the three warm-up calls are REAL optimizer steps).  Under
    data parallelism the segmented replay is additionally VALIDATED before it is trusted: one eager step and one replayed
    step from the same state must give the same loss on every rank (`validate`, default on when distributed)."""

    def __init__(self, step, example_points, G, restore=False, validate=None):
        """`restore`: put parameters, BatchNorm buffers and optimizer state back to what they were before the three
        warm-up steps, so that a training run continues exactly where an eager run would be."""
        self.step, self.G = step, G
        dev = example_points.device
        self.points = example_points.clone()
        self.order = torch.arange(G, dtype=torch.long, device=dev)
        self.graph = self.segments = None
        self.full_dp_graph = False
        distributed = fdist.is_distributed()
        validate = distributed if validate is None else validate
        snap = self._snapshot()
        try:
            self._capture(distributed, dev)
            if validate and (self.segments is not None or self.full_dp_graph):
                self._validate()
        except Exception:
            self.graph = self.segments = None
            torch.cuda.synchronize()
            self._restore(snap)                          # three real optimizer steps (and maybe more) ran on `example_points`
            step.optimizer.zero_grad(set_to_none=True)
            if step.grad_sync is not None:
                step.grad_sync.reset()
            raise
        if restore:
            self._restore(snap)

    # ---- training state = parameters + BatchNorm buffers (+ their host-side counters) + optimizer state + what the step carries
    def _snapshot(self):
        step = self.step
        net = {k: v.detach().clone() for k, v in step.netR.state_dict().items()}
        opt = None
        if hasattr(step.optimizer, "_step"):             # FusedAdam.state_dict() shares its moment tensors: deep copy
            sd = step.optimizer.state_dict()
            opt = {"state": {i: {k: v.clone() for k, v in st.items()} for i, st in sd["state"].items()},
                   "param_groups": sd["param_groups"]}
        carried = {k: None if v is None else v.snapshot() for k, v in step.carried_state().items()}
        return net, opt, [(m, m.steps) for m in self._bn_modules([step.netR])], carried or None     # None: nothing carried

    def _restore(self, snap):
        net, opt, steps, carried = snap
        with torch.no_grad():                            # in place: a captured graph holds the addresses of these tensors
            cur = self.step.netR.state_dict()
            for k, v in net.items():
                cur[k].copy_(v)
        for m, n in steps:
            m.steps = n
        if opt is not None:
            self.step.optimizer.load_state_dict(opt)
        for k, v in self.step.carried_state().items():   # after the model: the warm-up steps are real steps, and a piece they
            if v is not None:                            # created goes back to None's meaning (TrainStep.carried_state)
                v.restore((carried or {}).get(k))

    def _capture_graph(self, s):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            self.out = self.step.run(self.points, self.order)
        return graph

    def _capture(self, distributed, dev):
        step = self.step
        s = _capture_stream(dev)
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):                       # warm-up on a side stream (allocator + lazy inits)
            for _ in range(3):
                step.run(self.points, self.order)
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        # The capture pass runs the Python forward (no kernel executes), so the host-side num_batches_tracked counters
        # would run ahead of the running-statistics updates: restore them afterwards.  NOTE: the 3 warm-up calls above
        # are REAL optimizer steps on `example_points` (they also settle the allocator and Adam's lazy state).
        saved = [(m, m.steps) for m in self._bn_modules()]
        if distributed and os.environ.get("FACL_DP_GRAPH", "segments") == "full":
            # OPT-IN experiment (never the default): the collectives are captured INSIDE one graph (torch's RCCL process group
            # joins a stream capture the way it does on NCCL), so the data-parallel step has no cut at all.  Rehearsed with a
            # 1-rank RCCL group only (bench.py --rehearse-dp 1); with N > 1 ranks it has never run: the validation below
            # (eager step == replayed step, voted across ranks) is what stands between a wrong replay and the measurement.
            # (facl_amd/dist.py: full_graph_env -- the watchdog must have retired the warm-up's eager collectives before a
            # captured one is issued: it polls every ~100 ms)
            time.sleep(0.5)
            try:
                graph, err = self._capture_graph(s), ""
            except Exception as e:
                graph, err = None, "%s: %s" % (type(e).__name__, e)
            if not fdist.vote(graph is not None):
                raise GraphCaptureFailed("full-graph capture of the data-parallel step failed on some rank%s" % (" (here: %s)" % err if err else ""))
            self.graph = graph
            self.full_dp_graph = True
        elif distributed:
            # data parallel: the capture is cut at every collective (facl_amd/dist.py: GraphSegments) -- kernel segments
            # replay as graphs, the collectives in between are ordinary eager RCCL calls on the same stream
            rec = fdist.GraphSegments()
            s.wait_stream(torch.cuda.current_stream())
            try:
                with torch.cuda.stream(s):
                    self.out = fdist.run_capture(rec, lambda: step.run(self.points, self.order), step.rank)
            except fdist.CaptureFailed as e:             # agreed on by every rank (facl_amd/dist.py: run_capture)
                raise GraphCaptureFailed(str(e)) from e
            self.segments = rec
            torch.cuda.current_stream().wait_stream(s)
            torch.cuda.synchronize()
        else:
            try:
                self.graph = self._capture_graph(s)
            except Exception as e:
                raise GraphCaptureFailed("graph capture failed: %s: %s" % (type(e).__name__, e)) from e
        for m, n in saved:
            m.steps = n

    def _validate(self):
        """One eager step and one replayed step from the same state must agree (they run the same kernels in the same
        order: the losses are equal to the last bits) -- on EVERY rank, or nobody replays.  What this catches is what a
        one-GPU rehearsal cannot: an ordering lost between the collective library's stream and the next graph segment."""
        step = self.step
        snap = self._snapshot()
        loss_e = float(step.run(self.points, self.order)[0])
        self._restore(snap)
        (self.graph if self.segments is None else self.segments).replay()
        loss_g = float(self.out[0])
        self._restore(snap)
        ok = loss_e == loss_e and abs(loss_e - loss_g) <= 1e-5 * abs(loss_e)
        if not fdist.vote(ok):
            raise GraphCaptureFailed("replayed graph segments do not reproduce the eager step (this rank: eager loss %r, "
                                     "replayed %r)" % (loss_e, loss_g))

    def _bn_modules(self, nets=None):
        """The host-side BatchNorm counters a replay has to advance: those of the step's encoders, or of `nets`."""
        return [m for net in (self.step.encoders() if nets is None else nets) for m in net.modules() if hasattr(m, "count_batch")]

    def __call__(self, out_points, epoch=0, order=None):
        order = draw_order(self.G, order)
        self.points.copy_(out_points, non_blocking=True)
        self.order.copy_(torch.as_tensor(np.asarray(order), dtype=torch.long), non_blocking=True)
        self.step.epoch = epoch
        if hasattr(self.step.optimizer, "sync_lr"):
            self.step.optimizer.sync_lr()                # a StepLR change made since the capture reaches k_adam_prep
        (self.graph if self.segments is None else self.segments).replay()
        for m in self._bn_modules():                     # host-side num_batches_tracked (netR_FC.1 counts twice)
            m.count_batch()
        for net in self.step.encoders():
            net.netR_FC[1].count_batch()
        return self.out
