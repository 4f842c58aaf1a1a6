"""Supervised fine-tuning of the encoder on a classifier head: the third evaluation protocol beside the
linear probe (``facl_amd.linear_classify``) and the weighted kNN (``facl_amd.knn_eval``), which both freeze the encoder.
From a pre-trained checkpoint, from scratch (no checkpoint), or on a stratified fraction of the labels (semi-supervised).

    python -m facl_amd.finetune --synthetic 0 --data_root ../ntu/3DV_ntu60 --checkpoint corr_GL_95.pth --label_fraction 0.1

The head is the reference's probe head ``Final_FC`` (linear_classify/fc_model.py:12-25) reading the encoder's stacked
output in place (facl_amd/cls_head.py, csrc/cls.hip); the step replays as one HIP graph through ``train_step.GraphedStep``."""
import logging
import math
import os

import numpy as np
import torch

from . import cn3d_model_conbag as MODELL
from .cls_head import ClipClassifier
from .extract_common import ordered_views
from .train_common import TrainBatches, eval_mode, setup_run, synthetic_batch, train_epochs
from .train_flags import check_finetune_flags, check_finetune_train_flags, finetune_parser, optim_recipe, view_recipe  # noqa: F401
from .train_flags import describe_optimizer, finetune_train_parser, make_optimizer
from .train_step import GroupedStep

HEAD_PREFIX = "head."


class FineTuneNet(MODELL.PointNet_Plus):
    """PointNet_Plus that owns its ClipClassifier as ``head``: whatever snapshots ``netR.state_dict()`` (GraphedStep) or
    moves / switches the model covers the head too.  The encoder keeps its 52 keys; the head adds head.fc.weight / head.fc.bias."""

    def __init__(self, opt, num_class, gost=10, **kw):
        super().__init__(opt, gost=gost, **kw)
        self.head = ClipClassifier(gost, num_class)

    def encoder_parameters(self):
        return [p for n, p in self.named_parameters() if not n.startswith(HEAD_PREFIX)]

    def encoder_state_dict(self):
        """The encoder keys only: loadable by PointNet_Plus, the extraction entries and --checkpoint here."""
        return {k: v for k, v in self.state_dict().items() if not k.startswith(HEAD_PREFIX)}

    def head_state_dict(self):
        """fc.weight / fc.bias: loadable by linear_classify.Final_FC."""
        return self.head.state_dict()

    def load_encoder_state_dict(self, sd):
        res = self.load_state_dict(sd, strict=False)
        missing = [k for k in res.missing_keys if not k.startswith(HEAD_PREFIX)]
        if missing or res.unexpected_keys:
            raise RuntimeError("the checkpoint is not an encoder state_dict of this model: missing %s, unexpected %s"
                               % (missing, list(res.unexpected_keys)))


class FineTuneStep(GroupedStep):
    """One supervised iteration: grouping (GroupedStep.grouped) -> encoder forward -> head -> cross-entropy -> backward
    -> FusedAdam, with no host round trip (`run` is what GraphedStep captures).  The labels come from the static int32
    device tensor ``self.labels`` (batch,), which the caller fills in place before each call; `order` is ignored.

    ``freeze_bn``: the model is put in eval() for the step, so every BatchNorm is the constant affine of its running statistics
    (which the step leaves untouched) and the backward runs the frozen closed forms.  Such a step runs on eager
    launches only: capturing a step whose model is in eval() is refused here."""

    def __init__(self, netR, optimizer, opt, num_crop, group_radius=None, fps_reorder=False, freeze_bn=False):
        super().__init__(netR, optimizer, opt, num_crop, group_radius, fps_reorder)
        self.labels = torch.zeros(opt.batchSize, dtype=torch.int32, device=next(netR.parameters()).device)
        self.freeze_bn = bool(freeze_bn)

    def run(self, out_points, order):
        if self.freeze_bn:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("a step with frozen BatchNorm (model in eval()) runs eager: it is not captured into a graph")
            self.netR.eval()                                # the epoch loop switches to train() at the start of every epoch
        netR = self.netR
        xt, yt, B = self.grouped(out_points)
        if B > self.labels.shape[0]:
            raise RuntimeError("a batch of %d clips, the step holds %d labels" % (B, self.labels.shape[0]))
        netR(xt, yt, 1)
        logits = netR.head(netR._stacked, self.G, B)
        loss, stats = netR.head.loss(logits, self.labels[:B])
        self.backward_and_update(loss)
        return loss, logits, stats


def label_subset(labels, fraction, seed):
    """Stratified subset of a labelled split: per class (ascending), the first max(1, ceil(fraction * n_c)) entries of a
    RandomState(seed) permutation of that class's clips, the clips taken in ascending dataset index.  The permutations do not
    depend on `fraction`, so with one seed the subset at f1 is contained in the subset at f2 for f1 < f2; fraction = 1 gives
    the whole split.  Returns the sorted positions into `labels`.  Pure host code."""
    fraction = float(fraction)
    if not 0.0 < fraction <= 1.0:
        raise ValueError("label_fraction must be in (0, 1] (got %r)" % fraction)
    labels = np.asarray(labels).reshape(-1)
    rs = np.random.RandomState(seed)
    keep = []
    for c in np.unique(labels):
        idx = np.flatnonzero(labels == c)
        perm = rs.permutation(len(idx))
        keep.append(idx[perm[:max(1, int(math.ceil(fraction * len(idx))))]])
    return np.sort(np.concatenate(keep)) if keep else np.zeros((0,), dtype=np.int64)


def _raise_bad_labels(bad, num_class, where):
    raise RuntimeError("%d label(s) of %s lie outside [0, %d): raise --num_class or check --dataset" % (bad, where, num_class))


def evaluate(netR, step, opt, device):
    """Test top-1 (%) of the model as it stands: the test split of <data_root>/raw in eval(), batches and views as
    extract_split draws them (extract_common.ordered_views with its own generator), hits from the loss kernel's stats[0].
    The model returns to the mode it was in."""
    from . import dataset as fds
    index = fds.ClipIndex.from_dir(os.path.join(opt.data_root, fds.EXTRACT_LIST_DIR), opt.dataset)
    split = index.select(opt.split, test=True)
    if not len(split):
        raise RuntimeError("--eval_every: the test split of %s has no clips" % opt.data_root)
    total = torch.zeros(2, dtype=torch.int64, device=device)
    with eval_mode(netR):
        for views, names, labels in ordered_views(opt, device, index, split, np.random.RandomState(2000)):
            xt, yt = step.group(views if views.dtype == torch.float32 else views.float())
            netR(xt, yt, 1)
            logits = netR.head(netR._stacked, opt.num_crop, len(names))
            y = torch.as_tensor(labels, dtype=torch.int32).to(device)
            total += netR.head.loss(logits, y)[1]
    hits, bad = (int(v) for v in total.cpu())
    if bad:
        _raise_bad_labels(bad, opt.num_class, "the test split")
    return 100.0 * hits / len(split)


def main(args=None):
    """Returns the last test top-1 (%), or None when no evaluation ran."""
    opt = finetune_train_parser().parse_args(args)
    print(opt)
    check_finetune_train_flags(opt)
    if opt.synthetic != 1:
        print(view_recipe(opt).describe())
    torch.cuda.set_device(opt.main_gpu)
    device = torch.device("cuda", opt.main_gpu)
    setup_run(opt)

    num_crop = opt.num_crop
    netR = FineTuneNet(opt, opt.num_class, gost=num_crop)
    if opt.checkpoint:
        netR.load_encoder_state_dict(torch.load(opt.checkpoint, map_location="cpu", weights_only=True))
    netR = netR.to(device)
    netR.precision = opt.precision

    def labelled(index, split):
        keep = split[label_subset([index.label(int(v)) for v in split], opt.label_fraction, opt.label_seed)]
        print('labelled clips: %d of %d' % (len(keep), len(split)))
        return keep

    source = TrainBatches(opt, device, 0, 1, subset=labelled, too_few="the labelled subset has %(clips)d clips: fewer than "
                          "one batch of %(batch)d") if opt.synthetic == 0 else None
    steps_per_epoch = opt.steps_per_epoch if source is None else source.steps
    optimizer = make_optimizer(opt, netR.parameters(), steps_per_epoch)
    if describe_optimizer(opt):
        print(describe_optimizer(opt))
    step = FineTuneStep(netR, optimizer, opt, num_crop, opt.group_radius, bool(opt.fps_reorder), freeze_bn=bool(opt.freeze_bn))
    if opt.freeze_bn:
        opt.graph = 0                                    # no capture of a step whose model is in eval()
        msg = 'BatchNorm frozen: running statistics of %s kept; step runs eager' % opt.checkpoint
        logging.info(msg)
        print(msg)
    gen = torch.Generator(device=device)
    gen.manual_seed(1000)
    hits, top1 = 0, None

    def next_batch(disk, epoch, i):
        if disk is not None:
            out_points, _, labels = next(disk)
            labels = torch.as_tensor(labels, dtype=torch.int32)
        else:
            out_points = synthetic_batch(opt.batchSize, num_crop, opt.SAMPLE_NUM, opt.INPUT_FEATURE_NUM, device, gen)
            labels = torch.randint(0, opt.num_class, (opt.batchSize,), device=device, generator=gen).to(torch.int32)
        step.labels.copy_(labels)
        return out_points

    def after_step(out):
        nonlocal hits
        h, bad = (int(v) for v in out[2].cpu())
        if bad:
            _raise_bad_labels(bad, opt.num_class, "the train split")
        hits += h

    def after_epoch(epoch, mean_loss, clips, grad_norms=''):
        nonlocal hits, top1
        train_top1, hits = 100.0 * hits / (opt.batchSize * steps_per_epoch), 0
        logging.info('{} --epoch{} ==Average loss:{} train top1:{}'.format('Valid', epoch, mean_loss, train_top1))
        print('epoch:', epoch, '--loss:', mean_loss, 'train top1:', train_top1, '| clips/s: %.1f%s' % (clips, grad_norms))
        if opt.synthetic == 0 and opt.eval_every and (epoch + 1) % opt.eval_every == 0:
            top1 = evaluate(netR, step, opt, device)
            logging.info('{} --epoch{} ==test top1:{}'.format('Valid', epoch, top1))
            print('epoch:', epoch, 'test top1:', top1)
        if epoch % 5 == 0 or epoch == opt.nepoch - 1:
            torch.save(netR.encoder_state_dict(), '%s/finetune_enc_%d.pth' % (opt.save_root_dir, epoch))
            torch.save(netR.head_state_dict(), '%s/finetune_fc_%d.pth' % (opt.save_root_dir, epoch))

    train_epochs(opt, step, source, world=1, lr_step=5, next_batch=next_batch, after_epoch=after_epoch, after_step=after_step)
    return top1


if __name__ == '__main__':
    main()
