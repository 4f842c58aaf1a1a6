"""Shared body of the two training entries (the reference ships two scripts that differ in three
lines: default ``branch_choose``, data root and checkpoint file name -- cn3d_train_apperance_GL.py:135,161,341): data side, epoch
loop, ``run``; the flags and checks of ``train_flags`` and the step and replay of ``train_step`` stay importable from here."""
import contextlib
import logging
import os
import random
import time

import numpy as np
import torch

from . import cn3d_model_conbag as MODELL
from . import dist as fdist
from .train_flags import (OPTIM_FLAGS, VIEW_RECIPE_DEFAULTS, VIEW_RECIPE_FLAGS, _check_cosine_span, add_view_recipe_flags,  # noqa: F401
                          build_parser, check_class_mask_flags, check_cluster_id_flags, check_key_flags, check_knn_flags,
                          check_loss_flags, check_optim_flags, check_proto_flags, check_queue_flags, check_resident_flags,
                          check_sgd_flags, check_state_flags, check_train_flags, check_view_flags, describe_optimizer,
                          make_optimizer, optim_recipe, optimizer_flags, train_parser, view_recipe, with_defaults)
from .train_step import ContrastiveStep, GraphCaptureFailed, GraphedStep, TrainStep, group_views  # noqa: F401


def synthetic_batch(B, G, N, D, device, generator=None):
    """(B,G,N,D) float32 iid U[-0.5,0.5), the bench / parity input distribution."""
    return torch.rand(B, G, N, D, device=device, generator=generator) - 0.5


def appearance_batch(B, G, N, D, device, generator=None):
    """(B,G,N,D) float32 appearance-style synthetic clips (BASELINE configs[2]; SURVEY hard part 7).

    What the appearance branch feeds the same model (cn3D_data_set.py:125-137, generate_NTU.py:249-264): per clip ONE
    voxelised body surface -- 30 mm voxels normalised by the body height, i.e. coordinates on a ~1/64 grid with y in
    [-0.5,0.5], a narrower x and a thin depth relief, 4th channel an appearance value in [-0.5,0.5] -- and every view
    = N rows drawn WITH replacement from it (get_data_train, :287-318), so clouds contain duplicated rows (exact
    distance ties in the kNN) and grid-aligned neighbours.  Views g >= 1 are jittered (sigma 0.01, clip 0.05, :767-778),
    odd views x-mirrored (:708-713); view 0 is the raw resample and keeps its exact duplicates."""
    P0 = max(64, int(0.6 * N))
    r = lambda *shape: torch.rand(*shape, device=device, generator=generator)
    bx = (r(B, P0) - 0.5) * 0.44
    by = r(B, P0) - 0.5
    bz = 0.08 * torch.sin(6.0 * bx) * torch.cos(4.0 * by) + (r(B, P0) - 0.5) * 0.04
    base = torch.stack((bx, by, bz), dim=-1)
    base = torch.round(base * 64.0) / 64.0                                     # voxel grid
    if D == 4:
        app = torch.round((r(B, P0, 1) - 0.5) * 16.0) / 16.0
        base = torch.cat((base, app), dim=-1)
    idx = torch.randint(0, P0, (B, G, N), device=device, generator=generator)
    out = torch.gather(base.unsqueeze(1).expand(B, G, P0, D), 2, idx.unsqueeze(-1).expand(B, G, N, D)).clone()
    if G > 1:
        noise = (0.01 * torch.randn(B, G - 1, N, 3, device=device, generator=generator)).clamp_(-0.05, 0.05)
        out[:, 1:, :, :3] += noise
        out[:, 1::2, :, 0] *= -1.0
    return out.float()


def lr_for_epoch(base_lr, epoch, step_size=4, gamma=0.7):
    """StepLR(4, 0.7) stepped with the explicit epoch every iteration (:181,:333) = closed form."""
    return base_lr * gamma ** (epoch // step_size)


def load_resume_state(opt):
    """The state --resume names, on the CPU and checked against this run's options, with its path -- or (None, None) when
    `auto` finds no state.  `auto` skips a newest state that does not load (a damaged file), with a warning, for the next older."""
    from . import train_state
    if not opt.resume:
        return None, None
    if opt.resume != "auto":
        paths = [opt.resume]
    else:
        paths = [p for _, p in reversed(train_state.list_states(opt.save_root_dir))]
        if not paths:
            print("resume: no state under %s, starting from scratch" % opt.save_root_dir)
            return None, None
    for n, path in enumerate(paths):
        try:
            state = train_state.load_state(path)
        except train_state.StateUnreadable as e:
            if n + 1 == len(paths):
                raise
            print("warning: %s; trying %s" % (e, paths[n + 1]))
            continue
        train_state.check_compatible(state["flags"], opt)
        return state, path


def key_checkpoint_name(path):
    """<name>_key.pth beside the query checkpoint <name>.pth."""
    stem, ext = os.path.splitext(path)
    return stem + "_key" + ext


def save_checkpoint(netR, step, path):
    """The model's state_dict and, beside it, the key encoder's in the same format (extract_* / finetune --checkpoint load it)."""
    torch.save(netR.state_dict(), path)
    if step.key_encoder is not None:
        torch.save(step.key_encoder.state_dict(), key_checkpoint_name(path))


def split_class_ids(labels, fraction, seed):
    """The class id of every clip of a labelled split as the class-aware mask sees it: the clip's label inside the stratified
    `label_subset` (facl_amd/finetune.py: nested in `fraction` for one seed), -1 outside.  (N,) int32; pure host code."""
    from .finetune import label_subset
    labels = np.asarray(labels, dtype=np.int64).reshape(-1)
    ids = np.full(labels.shape, -1, dtype=np.int32)
    keep = label_subset(labels, fraction, seed)
    ids[keep] = labels[keep]
    return ids


def class_id_table(opt, source):
    """--loss_mask class: {v_name: class id} of the train clips as the run starts (None without the mask), announced."""
    if opt.loss_mask != 'class':
        return None
    if opt.class_ids == 'cluster':
        # no label is read: every clip is unknown (the class mask is then the exclude mask) until the first clustering
        class_of = {source.index.v_name(int(v)): -1 for v in source.split}
        print('class mask: cluster ids, %d clusters, every %d epoch(s); %d train clips unknown until the first clustering'
              % (opt.clusters, opt.cluster_every, len(class_of)))
    else:
        # every clip trains; the stratified subset keeps its label as class id, every other clip is unknown (-1)
        ids = split_class_ids([source.index.label(int(v)) for v in source.split], opt.label_fraction, opt.label_seed)
        class_of = {source.index.v_name(int(v)): int(c) for v, c in zip(source.split, ids)}
        print('class mask: %d of %d train clips labelled, %d classes' % (int((ids >= 0).sum()), len(ids), len(np.unique(ids[ids >= 0]))))
    if opt.class_positives:
        print('class positives: weight %g' % opt.class_positives)
    return class_of


@contextlib.contextmanager
def eval_mode(netR):
    """eval() and no_grad() for the block; the model returns to the mode it was in, also when the block raises."""
    was_training = netR.training
    netR.eval()
    try:
        with torch.no_grad():
            yield
    finally:
        netR.train(was_training)


def extract_monitor_splits(netR, opt, device, test=True, what="--knn_every"):
    """[(features, labels, v_names)] of the train split and, with `test`, the test split of <data_root>/raw, extracted in memory
    exactly as facl_amd.extract_common.run_disk extracts them (eval(), its own view seed 2000 and generator, train first: the
    train features do not depend on `test`).  Reads no training RNG stream and, in eval(), updates no running statistic; runs on
    ordinary eager launches, so its tensors come from the default allocator pool, never from a captured step's.  The model
    returns to the mode it was in."""
    from . import dataset as fds
    from .extract_common import extract_split
    index = fds.ClipIndex.from_dir(os.path.join(opt.data_root, fds.EXTRACT_LIST_DIR), opt.dataset)
    rng = np.random.RandomState(2000)
    splits = [index.select(opt.split, full_train=bool(opt.full_train))] + ([index.select(opt.split, test=True)] if test else [])
    with eval_mode(netR):
        data = []
        for split in splits:
            if not len(split):
                raise RuntimeError("%s: a split of %s has no clips" % (what, opt.data_root))
            f = extract_split(netR, opt, device, index, split, rng)
            y = torch.as_tensor([index.label(v) for v in split], dtype=torch.int64, device=device)
            data.append((f, y, [index.v_name(v) for v in split]))
    return data


def knn_monitor(netR, opt, device, data=None):
    """Weighted-kNN test top-1 (%) of the model as it stands, test against the train bank; `data`: what
    `extract_monitor_splits` returned for both splits (None: extracted here)."""
    from .knn_eval import knn_top1
    (ftr, ytr, _), (fte, yte, _) = extract_monitor_splits(netR, opt, device) if data is None else data
    return knn_top1(fte, yte, ftr, ytr, k=opt.knn_k, T=opt.knn_T)


def recluster(step, class_of, feats, names, K, iters=50, restarts=1, seed=0):
    """--class_ids cluster: spherical k-means of the global chunk (the last 512 columns) of the extracted train features
    `feats` (clips, (num_crop+1)*512); `class_of` {v_name: id} is replaced IN PLACE by the cluster ids of `names` (-1 for a clip
    that was not extracted).  Cluster numbers of two clusterings are unrelated, so the id ring of the step's queue goes back to
    unknown: stale ids would mask or attract the wrong rows, unknown ones leave them ordinary negatives until fresh pushes
    replace them; the rows and {head, valid} stay.  Returns (labels as a host array, info of facl_amd.cluster.kmeans); the
    (K, 512) un-normalised centroids that produced the labels ride along as info["centroids"] (the prototypes of --proto_weight)."""
    from . import cluster as fcl
    labels, cent, info = fcl.kmeans(feats[:, feats.shape[1] - 512:], K, iters=iters, restarts=restarts, seed=seed)
    info["centroids"] = cent
    ids = labels.cpu().numpy()
    for n in class_of:
        class_of[n] = -1
    for n, c in zip(names, ids):
        if n in class_of:
            class_of[n] = int(c)
    if step.queue is not None and step.queue.ids is not None:
        step.queue.ids.fill_(-1)
    return ids, info


def recluster_after_epoch(step, class_of, opt, device, epoch, test):
    """--class_ids cluster, after an epoch: extracts the train split (with `test` the test split too, for the kNN monitor),
    re-clusters it, refreshes the prototypes of --proto_weight, logs both.  Returns what `extract_monitor_splits` returned."""
    from . import cluster as fcl

    def report(line):
        logging.info('{} --epoch{} =={}'.format('Valid', epoch, line))
        print('epoch:', epoch, line)
    data = extract_monitor_splits(step.netR, opt, device, test=test, what="--class_ids cluster")
    ftr, ytr, names = data[0]
    ids, info = recluster(step, class_of, ftr, names, opt.clusters, opt.cluster_iters, opt.cluster_restarts, opt.cluster_seed + epoch)
    # the split is labelled on disk anyway: acc / nmi against the true labels are printed as a monitor ONLY -- the
    # training never sees those labels, its class ids are the cluster numbers above
    table = fcl.contingency(ids, ytr.cpu().numpy())
    sizes = np.sort(info['sizes'])
    report('clusters: %d objective: %.6f iters: %d sizes min/median/max: %d/%g/%d | acc: %.2f nmi: %.4f'
           % (opt.clusters, info['objective'], info['n_iter'], sizes[0], float(np.median(sizes)), sizes[-1],
              fcl.matched_accuracy(table), fcl.nmi(table)))
    if step.proto_weight > 0:
        # the ids a step saw so far came from the previous clustering (or were -1): any of them >= K raises here
        step.check_proto_err()
        from .knn_eval import knn_topk
        from .proto import concentrations
        cos_own = knn_topk(ftr[:, ftr.shape[1] - 512:], info["centroids"], 1)[0][:, 0]
        scale = concentrations(cos_own.cpu().numpy(), ids, opt.clusters, opt.proto_temperature, opt.proto_concentration)
        step.set_prototypes(info["centroids"], scale)
        phi = 1.0 / scale.astype(np.float64)
        report('prototypes: %d concentration min/mean/max: %.6g/%.6g/%.6g' % (opt.clusters, phi.min(), phi.mean(), phi.max()))
    return data


def setup_run(opt):
    """Seeds (shared across ranks: the circle-loss permutation is the same on all of them), output folder, log file."""
    opt.manualSeed = 1
    random.seed(opt.manualSeed)
    torch.manual_seed(opt.manualSeed)
    np.random.seed(opt.manualSeed)
    os.makedirs(opt.save_root_dir, exist_ok=True)
    if opt.log_file:
        logging.basicConfig(format='%(asctime)s %(message)s', datefmt='%Y/%m/%d %H:%M:%S',
                            filename=opt.log_file, level=logging.INFO)
    logging.info('======================================================')


class TrainBatches:
    """--synthetic 0, the reference's loader (cn3d_train_*_GL.py:161-172: the listed folder, shuffle + drop_last): the training
    split on disk (--resident 1: ingested here, once) and this rank's batches of every epoch.  `too_few`: the caller's wording
    of the refusal, a % template over clips / batch / world; `subset(index, split)` narrows the split (fine-tuning's labels)."""

    def __init__(self, opt, device, rank, world, too_few, subset=None, report_ingest=False):
        from . import dataset as fds
        self.opt, self.device, self.rank, self.world = opt, device, rank, world
        self.index = fds.ClipIndex.from_dir(os.path.join(opt.data_root, fds.TRAIN_LIST_DIR[opt.branch_choose]), opt.dataset)
        fds.check_same_index_on_all_ranks(self.index, device)
        split = np.asarray(self.index.select(opt.split, full_train=bool(opt.full_train)), dtype=np.int64)
        self.split = split if subset is None else subset(self.index, split)
        self.steps = len(self.split) // (opt.batchSize * world)
        if opt.max_steps_per_epoch > 0:
            self.steps = min(self.steps, opt.max_steps_per_epoch)
        if self.steps < 1:
            raise RuntimeError(too_few % dict(clips=len(self.split), batch=opt.batchSize, world=world))
        self.view_rng = np.random.RandomState(2000 + rank)    # --view_rng numpy: the generator the views draw from
        self.recipe = view_recipe(opt)
        self.resident = None
        if opt.resident:
            # every rank holds the whole split: the permutation is over the whole split, a rank's shard changes every epoch
            from . import resident as fres
            t_in = time.time()
            res = self.resident = fres.ResidentClips(
                self.index, opt.data_root, opt.branch_choose, self.split, device, max_gb=opt.resident_max_gb,
                reserve=fres.step_reserve_bytes(opt.batchSize, opt.num_crop, opt.SAMPLE_NUM))
            torch.cuda.synchronize()
            if report_ingest:
                print('resident: %d clips, %.3f GB, %.2f s' % (res.n, res.bytes['total'] / 1e9, time.time() - t_in))

    def epoch(self, epoch, hold_first=False):
        """Iterator over the epoch's ((G*B, N, 4) view-major views, v_names, labels); the caller close()s it (that stops
        the epoch's producer thread).  `hold_first`: the producer waits after batch 0 (a graph capture runs on it)."""
        from . import dataset as fds, resident as fres
        opt = self.opt
        pos = fds.train_batches(len(self.split), opt.batchSize, self.world, self.rank, opt.manualSeed, epoch)[:self.steps]
        vids = [self.split[p] for p in pos]
        if self.resident is not None:
            return fres.ResidentBatches(self.resident, vids, seed=2000, epoch=epoch,
                                        num_crop=opt.num_crop, num_point=opt.SAMPLE_NUM, recipe=self.recipe)
        disk = fds.DiskBatches(self.index, opt.data_root, opt.branch_choose, vids, opt.view_rng, self.device,
                               rng=self.view_rng, seed=2000, epoch=epoch, prefetch=bool(opt.prefetch),
                               num_crop=opt.num_crop, num_point=opt.SAMPLE_NUM, recipe=self.recipe)
        disk.hold_first = hold_first
        return iter(disk)


def wants_graph(opt):
    """--graph 1 replays the default loss only (swa_if = cld_if = 0); cleared once a capture has failed."""
    return bool(opt.graph) and not (opt.swa_if or opt.cld_if)


def capture_or_eager(step, out_points, opt):
    """`step` captured on the first batch (state restored: the same trajectory as eager), or `step` itself."""
    if not wants_graph(opt):
        return step
    try:
        return GraphedStep(step, out_points, step.G, restore=True)
    except GraphCaptureFailed as e:
        # the state is restored and EVERY rank is here (see GraphCaptureFailed): all continue on eager launches.  Anything
        # else propagates: the rank exits non-zero and the launcher stops the others
        print("graph capture failed (%s); running eager" % e)
        opt.graph = 0
        return step


def check_finite_loss(lv, epoch, i):
    """Inputs / a checkpoint with NaN or inf (the arithmetic itself has no range limit): no training on garbage."""
    if lv != lv or lv in (float("inf"), float("-inf")):
        raise FloatingPointError("non-finite loss %r at epoch %d, iteration %d" % (lv, epoch, i))


def trust_ratio_tail(optimizer):
    """' | trust ratio min/median/max: a/b/c' over the tensors that LARS adapted in the last step (read after a synchronisation)."""
    r = optimizer.trust_ratios().cpu()
    r = r[torch.tensor(optimizer.last_mask, dtype=torch.bool)]
    if not r.numel():
        return ' | trust ratio min/median/max: -/-/-'
    return ' | trust ratio min/median/max: %.4g/%.4g/%.4g' % (float(r.min()), float(r.median()), float(r.max()))


def train_epochs(opt, step, source, world, lr_step, next_batch, after_epoch, after_step=None, start_epoch=0, end_of_epoch=None):
    """The epoch loop of the training entries under StepLR(`lr_step`, 0.7).  `source`: the TrainBatches of --synthetic 0, else
    None (--steps_per_epoch steps).  The entries differ in `next_batch(disk, epoch, i)` -> the step's input (`disk`: the epoch's
    iterator of `source`, or None), `after_step(what the step returned)` and `after_epoch(epoch, mean_loss, clips_per_s)` --
    with --clip_grad_norm on or under --optim lars it gets a fourth argument, the ' | grad norm ...' / ' | trust ratio ...' tail of
    the epoch line.  Under --lr_schedule cosine
    the optimizer keeps the base rate and its device-side schedule does the rest.
    `start_epoch`: the first epoch run (a resumed run's).  `end_of_epoch(epoch)`: called last in every epoch, when the epoch's
    producer thread has stopped, so that the view generator's state is the one the next epoch starts from."""
    steps = opt.steps_per_epoch if source is None else source.steps
    run_step = step
    recipe = with_defaults(opt)                          # a namespace from before the recipe flags: the reference's StepLR
    cosine, max_norm = recipe.lr_schedule == "cosine", float(recipe.clip_grad_norm)
    lars = optimizer_flags(opt).optim == "lars"
    for epoch in range(start_epoch, opt.nepoch):
        for net in step.encoders():                      # MoCo's convention: the key copy normalises with batch statistics too
            net.train()
        for g in step.optimizer.param_groups:
            # cosine: the base rate; the device evaluates the schedule from its own step counter (facl_adam_prep_ex)
            g["lr"] = opt.learning_rate if cosine else lr_for_epoch(opt.learning_rate, epoch, lr_step)
        loss_sigma, t0 = 0.0, time.time()
        norms, clipped = [], 0
        disk = None if source is None else source.epoch(epoch, hold_first=run_step is step and wants_graph(opt))
        for i in range(steps):
            out_points = next_batch(disk, epoch, i)
            if run_step is step:                         # capture on the first batch
                run_step = capture_or_eager(step, out_points, opt)
            out = run_step(out_points, epoch)
            torch.cuda.synchronize()
            lv = out[0].item()
            check_finite_loss(lv, epoch, i)
            if max_norm:                                 # the step's pre-clip norm: two device scalars, already synchronised
                norms.append(float(step.optimizer.grad_norm()))
                clipped += float(step.optimizer.clip_coef()) < 1.0
            if after_step is not None:
                after_step(out)
            loss_sigma += lv
        if disk is not None:
            disk.close()
        extra = ()
        if max_norm:
            extra = (' | grad norm mean/max: %.4g/%.4g, clipped %d/%d steps' % (sum(norms) / steps, max(norms), clipped, steps),)
        if lars:                                         # the last step's ratios of the adapted tensors: one read per epoch
            extra = (''.join(extra) + trust_ratio_tail(step.optimizer),)
        after_epoch(epoch, loss_sigma / steps, opt.batchSize * steps * world / (time.time() - t0), *extra)
        if end_of_epoch is not None:
            end_of_epoch(epoch)


def run(default_branch, ckpt_pattern, args=None):
    # ---- flags (everything here raises before the device is touched)
    opt = train_parser(default_branch).parse_args(args)
    print(opt)
    check_train_flags(opt)
    recipe = view_recipe(opt)
    if opt.synthetic != 1:
        print(recipe.describe())
    from . import train_state
    flags = train_state.flags_of(opt)                  # as given: the grouper writes the reference's literals into `opt` later
    resumed, resumed_path = load_resume_state(opt)     # on the CPU, refused here if its options differ from this run's
    # ---- device
    local = int(os.environ.get("LOCAL_RANK", opt.main_gpu))
    torch.cuda.set_device(local)               # before the process group: RCCL binds its communicator to the current device
    device = torch.device("cuda", local)
    rank, world = fdist.init_from_env()
    setup_run(opt)
    # ---- model, source, optimizer, step
    num_crop = opt.num_crop
    netR = MODELL.PointNet_Plus(opt, gost=num_crop).to(device)
    netR.precision = opt.precision
    netR.bn_reduce_fn = fdist.make_bn_reduce_fn()
    source = TrainBatches(opt, device, rank, world, report_ingest=rank == 0, too_few="the split has %(clips)d clips: fewer "
                          "than one batch of %(batch)d per rank x %(world)d ranks") if opt.synthetic == 0 else None
    steps = opt.steps_per_epoch if source is None else source.steps
    # cn3d_train_motion_GL.py:180: the same update as torch.optim.Adam, all tensors in one HIP launch (facl_amd/optim.py); the
    # recipe flags (all off by default) add decay, clipping and the device-side schedule, which counts in steps of an epoch
    # --optim sgd / lars: FusedSGD on the same kernels' table, with the same clipping and schedule
    optimizer = make_optimizer(opt, netR.parameters(), steps)
    if rank == 0 and describe_optimizer(opt):
        print(describe_optimizer(opt))
    step = ContrastiveStep(netR, optimizer, opt, num_crop, opt.group_radius, bool(opt.fps_reorder), opt.swa_if, opt.cld_if)
    gen = torch.Generator(device=device)
    gen.manual_seed(1000 + rank)
    view_rng = np.random.RandomState(2000 + rank)         # --synthetic 2: the generator the view construction draws from
    source_rng = None if source is None else source.view_rng
    class_of = class_id_table(opt, source)

    def next_batch(disk, epoch, i):
        if opt.synthetic == 0:
            views, names, _ = next(disk)              # (G*B, N, 4) view-major views of the next batch
            if class_of is not None:                  # in place: a replayed graph reads this tensor
                step.clip_classes.copy_(torch.as_tensor([class_of[n] for n in names], dtype=torch.int32))
            return views
        if opt.synthetic == 2:
            # the loop body from the loader's output on (:224-228): raw clips -> the augmented views of every clip,
            # built on the GPU in one launch, view-major float32 (facl_amd/views.py; draws in the reference's NumPy order)
            from .views import build_views, synthetic_raw_clip
            base = ((epoch * opt.steps_per_epoch + i) * world + rank) * opt.batchSize
            clips = [synthetic_raw_clip(base + b) for b in range(opt.batchSize)]
            # --view_rng numpy: the reference's NumPy stream (a seed reproduces its views; ~0.2 ms of host draws per clip);
            # device: the same distributions drawn by a torch generator on the GPU (no per-clip host work)
            return build_views(clips, view_rng, device, device_rng=gen if opt.view_rng == "device" else None,
                               philox=(2000, epoch, [base + b for b in range(opt.batchSize)])
                               if opt.view_rng == "philox" else None, num_crop=num_crop, num_point=opt.SAMPLE_NUM,
                               recipe=recipe)
        if opt.synthetic == 1:
            return synthetic_batch(opt.batchSize, num_crop, opt.SAMPLE_NUM, opt.INPUT_FEATURE_NUM, device, gen)
        raise RuntimeError("--synthetic must be 0 (the dataset on disk), 1 or 2")

    def after_epoch(epoch, mean_loss, clips, grad_norms=''):
        logging.info('{} --epoch{} ==Average loss:{}'.format('Valid', epoch, mean_loss))
        if rank == 0:
            print('epoch:', epoch, 'loss mode is :', 1, '--loss:', mean_loss, '| clips/s: %.1f%s' % (clips, grad_norms))
        knn_now = bool(opt.knn_every) and (epoch + 1) % opt.knn_every == 0
        cluster_now = opt.class_ids == 'cluster' and (epoch + 1) % opt.cluster_every == 0
        data = recluster_after_epoch(step, class_of, opt, device, epoch, test=knn_now) if cluster_now else None  # one extraction
        if knn_now:
            top1 = knn_monitor(netR, opt, device, data)
            logging.info('{} --epoch{} ==knn top1:{}'.format('Valid', epoch, top1))
            print('epoch:', epoch, 'knn top1:', top1)
        if rank == 0 and epoch % 5 == 0:
            save_checkpoint(netR, step, ckpt_pattern % (opt.save_root_dir, epoch))

    def end_of_epoch(epoch):
        if not (opt.save_state_every and rank == 0 and (epoch + 1) % opt.save_state_every == 0):
            return
        t_w = time.time()
        state = train_state.assemble(epoch, (epoch + 1) * steps, flags, netR.state_dict(),
                                     optimizer.state_dict(), step.state_dict(), train_state.capture_rng(gen, view_rng, source_rng))
        path = train_state.state_path(opt.save_root_dir, epoch)
        train_state.write_atomic(state, path)
        train_state.prune(opt.save_root_dir, opt.keep_states)
        print('state: %s, %.1f MB, %.2f s' % (path, os.path.getsize(path) / 1e6, time.time() - t_w))

    # ---- resume
    start_epoch = 0
    if resumed is not None:
        # after setup_run has reseeded and every lazily created piece can be created eagerly (ContrastiveStep.load_state_dict)
        netR.load_state_dict(resumed["model"], strict=True)
        optimizer.load_state_dict(resumed["optimizer"])
        step.load_state_dict(resumed)
        train_state.apply_rng(resumed["rng"], gen, view_rng, source_rng)
        start_epoch = resumed["epoch"] + 1
        print('resumed from %s: epoch %d' % (resumed_path, start_epoch))
    # ---- loop
    train_epochs(opt, step, source, world, lr_step=4, next_batch=next_batch, after_epoch=after_epoch,
                 start_epoch=start_epoch, end_of_epoch=end_of_epoch)
    return netR
