"""Shared body of the two training entries (the reference ships two scripts that differ in three
lines: default ``branch_choose``, data root and checkpoint file name -- cn3d_train_apperance_GL.py:135,161,341)."""
import argparse
import contextlib
import logging
import math
import os
import random
import time

import numpy as np
import torch

from . import cn3d_model_conbag as MODELL
from . import dist as fdist
from .utils_my import check_class_positives, check_loss_mode, contrastive_losses_stacked, group_points_3DV, is_default_loss_mode, knn_radius_group


def build_parser(default_branch):
    """Flags of cn3d_train_motion_GL.py:77-135 (names, types and defaults unchanged) plus the additions
    marked NEW: synthetic data (the NTU files are not redistributable), real grouping parameters
    (the reference overrides knn_K / ball_radius with literals inside the grouper, utils_my.py:260-261)."""
    p = argparse.ArgumentParser(description="Training")
    p.add_argument('--batchSize', type=int, default=64, help='input batch size')
    p.add_argument('--nepoch', type=int, default=100, help='number of epochs to train for')
    p.add_argument('--INPUT_FEATURE_NUM', type=int, default=4, help='number of input point features')
    p.add_argument('--temperal_num', type=int, default=3, help='number of input point features')
    p.add_argument('--pooling', type=str, default='concatenation')
    p.add_argument('--dataset', type=str, default='ntu60')
    p.add_argument('--weight_decay', type=float, default=0.0008, help='weight decay (SGD only)')
    p.add_argument('--learning_rate', type=float, default=0.0003, help='learning rate at t=0')
    p.add_argument('--momentum', type=float, default=0.9, help='momentum (SGD only)')
    p.add_argument('--workers', type=int, default=0, help='number of data loading workers')
    p.add_argument('--root_path', type=str, default='../ntu/ntu60_new2/raw/', help='preprocess folder')
    p.add_argument('--depth_path', type=str, default='', help='raw_depth_png')
    p.add_argument('--save_root_dir', type=str, default='../ntu/ntu60_new2/model/', help='output folder')
    p.add_argument('--model', type=str, default='', help='model name for training resume')
    p.add_argument('--optimizer', type=str, default='', help='optimizer name for training resume')
    p.add_argument('--ngpu', type=int, default=1, help='# GPUs')
    p.add_argument('--main_gpu', type=int, default=0, help='main GPU id')
    p.add_argument('--emb_dims', type=int, default=1024)
    p.add_argument('--k', type=int, default=20)
    p.add_argument('--dropout', type=float, default=0.05)
    p.add_argument('--learning_rate_decay', type=float, default=1e-7)
    p.add_argument('--size', type=str, default='full')
    p.add_argument('--SAMPLE_NUM', type=int, default=512, help='number of sample points')
    p.add_argument('--Num_Class', type=int, default=512, help='number of outputs')
    p.add_argument('--knn_K', type=int, default=64, help='K for knn search')
    p.add_argument('--sample_num_level1', type=int, default=64, help='number of first layer groups')
    p.add_argument('--sample_num_level2', type=int, default=64, help='number of second layer groups')
    p.add_argument('--ball_radius', type=float, default=0.16, help='square of radius for ball query in level 1')
    p.add_argument('--ball_radius2', type=float, default=0.25, help='square of radius for ball query in level 2')
    p.add_argument('--ex_feature', type=int, default=7)
    p.add_argument('--save_feature_dir', type=str, default='../ntu/ntu60_new2/features/')
    p.add_argument('--save_label_dir', type=str, default='../ntu/ntu60_new2/labels/')
    p.add_argument('--branch_choose', type=str, default=default_branch)
    # NEW
    p.add_argument('--synthetic', type=int, default=1,
                   help='NEW: 0 = the 3DV clips on disk under --data_root (facl_amd/dataset.py); 1 = iid U[-0.5,0.5) clouds (no NTU data here); 2 = synthetic RAW clips (the four (rows, 8) clouds the '
                        'loader reads per video) through the GPU view construction (facl_amd.views.build_views = the dataset '
                        "class's get_data_train, cn3D_data_set.py:285-350).  0 and 2 need --INPUT_FEATURE_NUM 4 and --num_crop 10 --SAMPLE_NUM 512, "
                        'the reference\'s loader; with --view_rng philox any --num_crop 1..64 and --SAMPLE_NUM 64..4096 (multiples of 64)')
    p.add_argument('--view_rng', type=str, default='numpy', choices=('numpy', 'device', 'philox'),
                   help='NEW (--synthetic 0 / 2): numpy = draw the view construction\'s random numbers on the host in the reference\'s '
                        'NumPy order; device = draw them on the GPU (same distributions, another stream; --synthetic 2 only); '
                        'philox = counter-based draws on the GPU keyed by (seed, epoch, dataset index of the clip); the only stream '
                        'with views beyond 10 x 512 (view v = kind v %% 10 in round v // 10: facl_amd/philox.py)')
    p.add_argument('--data_root', type=str, default='../ntu/3DV_ntu60',
                   help='NEW (--synthetic 0): the dataset root, the literal prefix ../ntu/3DV_ntu60 of the reference\'s paths')
    p.add_argument('--split', type=str, default='view', choices=('view', 'subject', 'set'),
                   help='NEW (--synthetic 0): cross-view (the reference\'s literal DATA_CROSS_VIEW=True), cross-subject or cross-set')
    p.add_argument('--full_train', type=int, default=1,
                   help='NEW (--split subject): 1 = all training performers (literal full_train=True), 0 = without the validation ones')
    p.add_argument('--max_steps_per_epoch', type=int, default=0,
                   help='NEW (--synthetic 0): cap on the steps of an epoch (len(split) // (batchSize * world)); 0 = no cap')
    p.add_argument('--prefetch', type=int, default=1,
                   help='NEW (--synthetic 0): 1 = load and draw batch i+1 on a producer thread while step i runs')
    p.add_argument('--resident', type=int, default=0, choices=(0, 1),
                   help='NEW (--synthetic 0 --view_rng philox): 1 = load the training split ONCE into device memory and build '
                        'every batch\'s views there by index (facl_amd/resident.py): no file is read and no clip data is copied '
                        'after the ingest; the views equal --resident 0\'s bit for bit.  Refuses when the split does not fit')
    p.add_argument('--resident_max_gb', type=float, default=0.0,
                   help='NEW (--resident 1): bound on the resident pool in GiB; 0 = automatic (free device memory minus the '
                        'reserve kept for the training step, facl_amd.resident.STEP_RESERVE_BYTES)')
    p.add_argument('--num_crop', type=int, default=10, help='NEW: views per clip (literal 10 at :189)')
    p.add_argument('--steps_per_epoch', type=int, default=8, help='NEW: synthetic iterations per epoch')
    p.add_argument('--group_radius', type=float, default=None,
                   help='NEW: r^2 of the grouper (default: the reference literals 0.06 at N=512, 0.16 otherwise)')
    p.add_argument('--log_file', type=str, default='', help='NEW: log path (reference: ../ntu/ntu60_new2/30_0425.log)')
    p.add_argument('--swa_if', type=int, default=0, help='NEW: 1 = add 0.6 * the SwAV term (literal swa_if = 0 at :238)')
    p.add_argument('--cld_if', type=int, default=0, help='NEW: 1 = add the CLD k-means term (literal cld_if = 0 at :319)')
    p.add_argument('--precision', type=str, default='f32', choices=('f32', 'x3b', 'x3'),
                   help='NEW: arithmetic of the dense contractions (facl_amd.tail.precision): f32 = fp32-grade (default); '
                        'x3b = three bf16 products in the backward GEMMs only (features / loss unchanged); x3 = everywhere')
    p.add_argument('--graph', type=int, default=1,
                   help='NEW: 1 = replay the iteration as HIP graph(s) (train_common.GraphedStep; the eager loop is host-bound at '
                        'this step time); needs the default loss (swa_if = cld_if = 0).  0 = eager launches')
    p.add_argument('--fps_reorder', type=int, default=0,
                   help='NEW: 1 = FPS-reorder every view on the GPU before grouping (cn3D_data_set.py:665-672; the '
                        'reference assumes FPS-ordered clouds but its live loader never calls it)')
    p.add_argument('--knn_every', type=int, default=0,
                   help='NEW (--synthetic 0, one rank): after every E-th epoch extract the train and test splits in memory and '
                        'log the weighted-kNN test top-1 against the train bank (facl_amd/knn_eval.py) as "knn top1"; 0 = off')
    p.add_argument('--knn_k', type=int, default=20, help='NEW (--knn_every): neighbours per query (1..64)')
    p.add_argument('--knn_T', type=float, default=0.1, help='NEW (--knn_every): temperature of the exp(s / T) vote')
    p.add_argument('--loss_normalize', type=int, default=0, choices=(0, 1),
                   help='NEW: 1 = L2-normalise every embedding row in front of the global / circle losses (cosine similarity); '
                        '0 = raw dot products (the reference)')
    p.add_argument('--loss_temperature', type=float, default=1.0,
                   help='NEW: the similarities of the global / circle losses are divided by this temperature (reference: 1)')
    p.add_argument('--loss_mask', type=str, default='zero', choices=('zero', 'exclude', 'class'),
                   help='NEW: same-clip key columns of the global / circle losses: zero = multiplied by 0, they stay in the '
                        'softmax as exp(0) (the reference); exclude = taken out of the log-sum-exp (negatives only); class '
                        '(--synthetic 0, one rank) = exclude, and the keys and queue rows of clips known to share the '
                        'anchor\'s action leave it too; --label_fraction of the train clips are "known"')
    p.add_argument('--class_positives', type=float, default=0.0,
                   help='NEW (--loss_mask class): lambda > 0 = the keys and queue rows that the class mask removes for sharing '
                        'the anchor\'s action are extra positives of the global / circle losses, through their mean term and '
                        'with weight lambda against the clip\'s own positives; 0 = off')
    p.add_argument('--label_fraction', type=float, default=1.0,
                   help='NEW: 0 < f <= 1, the stratified fraction of the train split whose labels are used (label_subset)')
    p.add_argument('--label_seed', type=int, default=0, help='NEW: seed of the per-class permutations of --label_fraction')
    p.add_argument('--class_ids', type=str, default='labels', choices=('labels', 'cluster'),
                   help='NEW (--loss_mask class): labels = the class ids are the action labels of --label_fraction of the clips; '
                        'cluster = no label is read: after every --cluster_every-th epoch the train split is extracted in memory '
                        'and clustered by spherical k-means (facl_amd/cluster.py), and the cluster ids are the class ids; every '
                        'clip is unknown until the first clustering')
    p.add_argument('--clusters', type=int, default=0, help='NEW (--class_ids cluster): K of the k-means, 2..1024')
    p.add_argument('--cluster_every', type=int, default=0, help='NEW (--class_ids cluster): re-cluster after every E-th epoch, E >= 1')
    p.add_argument('--cluster_iters', type=int, default=50, help='NEW (--class_ids cluster): centroid updates per restart at most')
    p.add_argument('--cluster_restarts', type=int, default=1, help='NEW (--class_ids cluster): restarts of every clustering')
    p.add_argument('--cluster_seed', type=int, default=0, help='NEW (--class_ids cluster): the clustering after epoch e draws its initial rows with seed + e')
    p.add_argument('--proto_weight', type=float, default=0.0,
                   help='NEW (--class_ids cluster): w > 0 = add w x the prototype contrastive term (ProtoNCE, facl_amd/proto.py) on '
                        'the centroids of the last clustering: every row of the stacked output against its clip\'s own centroid and '
                        'the other K - 1; zero until the first clustering; 0 = off')
    p.add_argument('--proto_temperature', type=float, default=0.2,
                   help='NEW (--proto_weight): the mean of the per-cluster temperatures phi_k (the temperature itself under fixed)')
    p.add_argument('--proto_concentration', type=str, default='cluster', choices=('cluster', 'fixed'),
                   help='NEW (--proto_weight): cluster = phi_k from the cluster\'s own concentration (PCL: mean distance to the '
                        'centroid / log(size + 10), clipped to the 10th..90th percentile, mean = --proto_temperature); fixed = '
                        'every phi_k = --proto_temperature')
    p.add_argument('--neg_queue', type=int, default=0,
                   help='NEW (one rank): L > 0 = the global / circle losses also see the x_global rows of the last L clips as '
                        'negatives (a device-side ring buffer, facl_amd/neg_queue.py); a multiple of --batchSize; 0 = off')
    p.add_argument('--key_encoder', type=int, default=0, choices=(0, 1),
                   help='NEW (--neg_queue L > 0): 1 = the rows stored in the queue come from a momentum-averaged copy of the '
                        'encoder (facl_amd/key_encoder.py), saved beside every checkpoint as <name>_key.pth; 0 = from the '
                        'trained encoder')
    p.add_argument('--key_momentum', type=float, default=0.999,
                   help='NEW (--key_encoder 1): m of key <- m key + (1 - m) model after every optimizer step, 0 <= m < 1')
    p.add_argument('--save_state_every', type=int, default=0,
                   help='NEW (one rank): after every E-th epoch write the full training state -- model, Adam, negative queue, key '
                        'encoder, SwAV queue, every RNG stream -- as <save_root_dir>/state_<epoch>.pth (facl_amd/train_state.py); '
                        '0 = off')
    p.add_argument('--keep_states', type=int, default=2, help='NEW (--save_state_every): the K newest states are kept; 0 = all')
    p.add_argument('--resume', type=str, default='',
                   help='NEW (one rank): a state_<epoch>.pth to continue from, bit-exactly as if the run had never stopped, or '
                        '"auto" = the newest state under --save_root_dir (none there: the run starts from scratch)')
    p.add_argument('--adamw_decay', type=float, default=0.0,
                   help='NEW (one rank): decoupled weight decay of the optimizer (torch.optim.AdamW\'s update) on every weight '
                        'matrix and convolution kernel; biases and BatchNorm gamma / beta are not decayed; 0 = off')
    p.add_argument('--clip_grad_norm', type=float, default=0.0,
                   help='NEW (one rank): the gradients of a step are scaled so that their global L2 norm is at most this value '
                        '(torch.nn.utils.clip_grad_norm_), and the epoch line reports the norms; 0 = off')
    p.add_argument('--lr_schedule', type=str, default='step', choices=('step', 'cosine'),
                   help='NEW (one rank for cosine): step = StepLR per epoch (the reference); cosine = half a cosine per optimizer '
                        'step from --learning_rate down to --lr_min over --lr_decay_epochs, evaluated on the device')
    p.add_argument('--warmup_steps', type=int, default=0,
                   help='NEW (one rank): the learning rate of either schedule is multiplied by min(1, t / W) at optimizer step t')
    p.add_argument('--lr_decay_epochs', type=int, default=0,
                   help='NEW (--lr_schedule cosine, required >= 1 there): the cosine reaches --lr_min after this many epochs '
                        '(x the steps of an epoch, warm-up included) and stays there')
    p.add_argument('--lr_min', type=float, default=0.0, help='NEW (--lr_schedule cosine): the rate the cosine ends at')
    add_view_recipe_flags(p)
    return p


VIEW_RECIPE_FLAGS = ("view_kinds", "jitter_sigma", "jitter_clip", "rot_range", "scale_lo", "scale_hi", "tilt_angle")
VIEW_RECIPE_DEFAULTS = ("reference", 0.01, 0.05, 0.8, 0.5, 1.5, 0.25)       # = facl_amd.philox.DEFAULT_STRENGTHS


def add_view_recipe_flags(p):
    """The view recipe of --view_rng philox (facl_amd.philox.Recipe): the kinds of a round and six strengths."""
    p.add_argument('--view_kinds', type=str, default='reference',
                   help='NEW (--view_rng philox): the kinds of a round, 1..12 comma-separated names; view v is of the kind at '
                        'position v %% L in round v // L.  raw, mirror, key, key_mirror, rot, t4, t7, res30, res10: the '
                        'reference\'s views; jitter, scale, tilt_neg, tilt_pos: transforms it defines and never wires in.  '
                        'reference = raw,mirror,key,key_mirror,rot,rot,t4,t7,res30,res10.  A view\'s draws depend on the kinds '
                        'before it in the list')
    p.add_argument('--jitter_sigma', type=float, default=0.01, help='NEW (--view_rng philox): sigma of the jitter, >= 0 (literal 0.01 at :765)')
    p.add_argument('--jitter_clip', type=float, default=0.05, help='NEW (--view_rng philox): the jitter is clipped to +- this, > 0 (literal 0.05 at :765)')
    p.add_argument('--rot_range', type=float, default=0.8,
                   help='NEW (--view_rng philox): a rot view turns about y by (u - 0.5) * pi * this, in [0, 2] (literal 0.8 at :739)')
    p.add_argument('--scale_lo', type=float, default=0.5, help='NEW (--view_rng philox): a scale view multiplies xyz by s in [scale_lo, scale_hi) (literal 0.5 at :759)')
    p.add_argument('--scale_hi', type=float, default=1.5, help='NEW (--view_rng philox): see --scale_lo (literal 1.5 at :759)')
    p.add_argument('--tilt_angle', type=float, default=0.25,
                   help='NEW (--view_rng philox): tilt_neg / tilt_pos turn about y by -/+ pi * this (literal 0.25 at :723)')


def view_recipe(opt):
    """The facl_amd.philox.Recipe of the seven flags (a namespace without them: the default), checked.  Any non-default value
    needs the counter-based draws on clips: refused with --view_rng numpy / device and with --synthetic 1.  Touches no device."""
    from .philox import Recipe
    given = [getattr(opt, k, d) for k, d in zip(VIEW_RECIPE_FLAGS, VIEW_RECIPE_DEFAULTS)]
    try:
        recipe = Recipe.parse(given[0], **dict(zip(VIEW_RECIPE_FLAGS[1:], given[1:])))
    except ValueError as e:
        raise RuntimeError(str(e)) from None
    if not recipe.is_default():
        changed = ", ".join("--%s %s" % (k, v) for k, v, d in zip(VIEW_RECIPE_FLAGS, given, VIEW_RECIPE_DEFAULTS) if v != d)
        if getattr(opt, "synthetic", 0) == 1:
            raise RuntimeError("%s with --synthetic 1: iid clouds are no views of a clip, and the reference's stream defines its "
                               "ten views only; a view recipe needs --synthetic 0 or 2 with --view_rng philox" % changed)
        if opt.view_rng != 'philox':
            raise RuntimeError("%s with --view_rng %s: the reference's stream defines its ten views only (the kinds and "
                               "strengths of cn3D_data_set.py:285-350); another recipe needs --view_rng philox, whose "
                               "counter-based draws cover it" % (changed, opt.view_rng))
    return recipe


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


def group_views(data1, opt, r2=None):
    """The grouper of training and extraction over view-major (M,N,D) rows (the second path: or a clip-major (B,G,N,D)
    batch).  `r2` None: the reference's literals, K=64 and r^2=0.06 at N=512 (:230), group_points_3DV_2048's 0.16 otherwise."""
    if r2 is None and opt.SAMPLE_NUM == 512:
        return group_points_3DV(data1, opt)
    opt.INPUT_FEATURE_NUM = data1.shape[-1]
    return knn_radius_group(data1, opt.sample_num_level1, opt.knn_K, 0.16 if r2 is None else r2)


class ContrastiveStep:
    """One training iteration = the loop body of cn3d_train_motion_GL.py:224-335."""

    def __init__(self, netR, optimizer, opt, num_crop, group_radius=None, fps_reorder=False, swa_if=0, cld_if=0):
        self.netR, self.optimizer, self.opt, self.G = netR, optimizer, opt, num_crop
        self.swa_if, self.cld_if = int(swa_if), int(cld_if)
        self.swav_state = None
        self.epoch = 0
        self.r2 = group_radius
        self.fps_reorder = fps_reorder
        self._one = None
        # loss modes (utils_my.contrastive_losses_stacked); namespaces from before the flags hold the reference's loss
        self.loss_mode = dict(normalize=bool(getattr(opt, "loss_normalize", 0)),
                              temperature=float(getattr(opt, "loss_temperature", 1.0)), mask=getattr(opt, "loss_mask", "zero"))
        # cross-batch queue of negative keys (facl_amd/neg_queue.py): created on the first step, pushed at the end of every step
        self.neg_queue = int(getattr(opt, "neg_queue", 0))
        self.queue = None
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
        self.key_momentum = float(getattr(opt, "key_momentum", 0.999)) if int(getattr(opt, "key_encoder", 0)) else None
        self.key_encoder = None
        if self.key_momentum is not None and not self.neg_queue:
            raise RuntimeError("the key encoder supplies the rows of the negative queue: it needs neg_queue > 0")
        # class-mates as extra positives (utils_my: class_positives); beside loss_mode, which stays the dict of the three modes
        self.class_positives = check_class_positives(getattr(opt, "class_positives", 0.0), self.loss_mode["mask"])
        # prototype contrastive term (facl_amd/proto.py): static tensors that the caller fills in place after every clustering
        # (set_prototypes), so that a replayed graph reads the current centroids; zeros / ones do nothing while every id is -1
        self.proto_weight = float(getattr(opt, "proto_weight", 0.0))
        self.prototypes = self.proto_inv = self.proto_scale = self.proto_err = None
        if self.proto_weight > 0:
            if self.clip_classes is None:
                raise RuntimeError("the prototype term reads the clips' cluster ids: it needs the class-aware loss mask")
            from .cls_head import FEATURE_DIM
            dev, K = self.clip_classes.device, int(opt.clusters)
            self.prototypes = torch.zeros((K, FEATURE_DIM), dtype=torch.float32, device=dev)
            self.proto_inv = torch.ones((K,), dtype=torch.float32, device=dev)
            self.proto_scale = torch.ones((K,), dtype=torch.float32, device=dev)
        self.rank = torch.distributed.get_rank() if fdist.is_distributed() else 0
        self.grad_sync = fdist.GradSync(list(netR.named_parameters())) if fdist.is_distributed() else None

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

    def group(self, data1):
        return group_views(data1, self.opt, self.r2)

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

    def __call__(self, out_points, epoch=0, order=None):
        netR, G = self.netR, self.G
        if order is None:
            order = np.arange(0, G, 1)
            np.random.shuffle(order)                                               # :297-298
        if not torch.is_tensor(order):
            order = torch.as_tensor(np.asarray(order), dtype=torch.long).to(out_points.device)
        self.epoch = epoch
        return self.run(out_points, order)

    def run(self, out_points, order):
        """Device-only body (no host round trips): this is what GraphedStep captures into a HIP graph.
        `out_points`: the loader's clip-major (B,G,N,D) batch, or -- 3-dimensional -- the view-major (G*B,N,D) rows that
        facl_amd.views.build_views writes directly (the permute + reshape of :226 already done)."""
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
        xt, yt = self.group(data1)
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
        self.optimizer.zero_grad(set_to_none=True)
        if self._one is None or self._one.device != loss.device:
            self._one = torch.ones((), dtype=torch.float32, device=loss.device)    # the seed of backward(): no fill launch per step
        loss.backward(self._one)
        if self.grad_sync is not None:
            self.grad_sync.finish()                                                # tail bucket overlapped with the SA backward
        self.optimizer.step()
        return loss, loss_c, loss_circle


class GraphCaptureFailed(RuntimeError):
    """The step could not be captured (or its replay did not reproduce the eager step).  Model, BatchNorm buffers and
    optimizer state are back at their values from before the attempt.  Under data parallelism EVERY rank raises it at the
    same point of the collective sequence (facl_amd/dist.py: GraphSegments' failure protocol), so all ranks may continue
    together on eager launches; any other exception out of GraphedStep under world > 1 is not agreed on and must end the rank."""


_CAPTURE_STREAMS = {}


def _capture_stream(dev):
    """One side stream per device for warm-up + capture (the scratch workspace of the HIP passes is keyed by stream:
    a fresh stream per GraphedStep would pin another workspace each time)."""
    key = (dev.type, dev.index)
    if key not in _CAPTURE_STREAMS:
        _CAPTURE_STREAMS[key] = torch.cuda.Stream(device=dev)
    return _CAPTURE_STREAMS[key]


class GraphedStep:
    """The whole training iteration (grouping -> forward -> losses -> backward -> Adam) captured once into a HIP
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
        distributed = fdist.is_distributed()
        validate = distributed if validate is None else validate
        snap = self._snapshot()
        try:
            self._capture(distributed, dev)
            if validate and (self.segments is not None or getattr(self, "full_dp_graph", False)):
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

    # ---- training state = parameters + BatchNorm buffers (+ their host-side counters) + optimizer state
    def _snapshot(self):
        step = self.step
        net = {k: v.detach().clone() for k, v in step.netR.state_dict().items()}
        opt = None
        if hasattr(step.optimizer, "_step"):             # FusedAdam.state_dict() shares its moment tensors: deep copy
            sd = step.optimizer.state_dict()
            opt = {"state": {i: {k: v.clone() for k, v in st.items()} for i, st in sd["state"].items()},
                   "param_groups": sd["param_groups"]}
        queue = getattr(step, "queue", None)             # a step class without the attribute (dense.DenseStep) has no queue
        queue = None if queue is None else queue.snapshot()              # None: no step has run yet, the queue is empty
        key = getattr(step, "key_encoder", None)         # likewise; None: no step has run yet, the copy would equal the model
        key = None if key is None else key.snapshot()
        return net, opt, [(m, m.steps) for m in self._bn_modules(False)], queue, key

    def _restore(self, snap):
        net, opt, steps, queue, key = snap
        if getattr(self.step, "queue", None) is not None:                # the warm-up steps are real steps: their rows leave the queue again
            self.step.queue.restore(queue)
        with torch.no_grad():                            # in place: a captured graph holds the addresses of these tensors
            cur = self.step.netR.state_dict()
            for k, v in net.items():
                cur[k].copy_(v)
        for m, n in steps:
            m.steps = n
        if opt is not None:
            self.step.optimizer.load_state_dict(opt)
        if getattr(self.step, "key_encoder", None) is not None:          # after the model: None takes the restored model's state
            self.step.key_encoder.restore(key)

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
            import time
            time.sleep(0.5)
            graph = torch.cuda.CUDAGraph()
            try:
                with torch.cuda.graph(graph, stream=s):
                    self.out = step.run(self.points, self.order)
            except Exception as e:
                ok = False
                err = "%s: %s" % (type(e).__name__, e)
            else:
                ok, err = True, ""
            if not fdist.vote(ok):
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
            graph = torch.cuda.CUDAGraph()
            try:
                with torch.cuda.graph(graph, stream=s):
                    self.out = step.run(self.points, self.order)
            except Exception as e:
                raise GraphCaptureFailed("graph capture failed: %s: %s" % (type(e).__name__, e)) from e
            self.graph = graph
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
        if self.segments is not None:
            self.segments.replay()
        else:
            self.graph.replay()
        loss_g = float(self.out[0])
        self._restore(snap)
        ok = loss_e == loss_e and abs(loss_e - loss_g) <= 1e-5 * abs(loss_e)
        if not fdist.vote(ok):
            raise GraphCaptureFailed("replayed graph segments do not reproduce the eager step (this rank: eager loss %r, "
                                     "replayed %r)" % (loss_e, loss_g))

    def _encoders(self, with_key=True):
        key = getattr(self.step, "key_encoder", None) if with_key else None
        return [self.step.netR] + ([] if key is None else [key.key])

    def _bn_modules(self, with_key=True):
        """The host-side BatchNorm counters a replay has to advance: the model's and, once it exists, the key encoder's."""
        return [m for net in self._encoders(with_key) for m in net.modules() if hasattr(m, "count_batch")]

    def __call__(self, out_points, epoch=0, order=None):
        if order is None:
            order = np.arange(0, self.G, 1)
            np.random.shuffle(order)
        self.points.copy_(out_points, non_blocking=True)
        self.order.copy_(torch.as_tensor(np.asarray(order), dtype=torch.long), non_blocking=True)
        self.step.epoch = epoch
        sync = getattr(self.step.optimizer, "sync_lr", None)
        if sync is not None:
            sync()                                       # a StepLR change made since the capture reaches k_adam_prep
        if self.segments is not None:
            self.segments.replay()
        else:
            self.graph.replay()
        for m in self._bn_modules():                     # host-side num_batches_tracked (netR_FC.1 counts twice)
            m.count_batch()
        for net in self._encoders():
            net.netR_FC[1].count_batch()
        return self.out


def lr_for_epoch(base_lr, epoch, step_size=4, gamma=0.7):
    """StepLR(4, 0.7) stepped with the explicit epoch every iteration (:181,:333) = closed form."""
    return base_lr * gamma ** (epoch // step_size)


def check_view_flags(opt):
    """--synthetic 0 / 2 build views from clips: 4 channels; 10 views of 512 points on the reference's streams, any size of
    the kernels' domain on the counter-based one; the view recipe (`view_recipe`) on the counter-based one only.  Raises
    before the device is touched."""
    view_recipe(opt)
    if opt.synthetic not in (0, 2):
        return
    what = "--synthetic %d" % opt.synthetic
    if opt.synthetic == 0 and opt.view_rng == 'device':
        raise RuntimeError("--synthetic 0 draws with --view_rng numpy or philox")
    if opt.INPUT_FEATURE_NUM != 4:
        raise RuntimeError("%s builds views of 4 channels: use --INPUT_FEATURE_NUM 4" % what)
    if opt.view_rng == 'philox':
        from .views import check_view_size
        try:
            check_view_size(opt.num_crop, opt.SAMPLE_NUM)
        except ValueError as e:
            raise RuntimeError("%s --view_rng philox: --num_crop 1..64 and --SAMPLE_NUM 64..4096 in multiples of 64 (%s)"
                               % (what, e)) from None
    elif (opt.num_crop, opt.SAMPLE_NUM) != (10, 512):
        raise RuntimeError("%s --view_rng %s: the reference's stream defines 10 views of 512 points only (its loader draws a "
                           "literal 512, cn3D_data_set.py:24): use --num_crop 10 --SAMPLE_NUM 512, or --view_rng philox, "
                           "whose counter-based recipe covers other sizes" % (what, opt.view_rng))


def check_resident_flags(opt):
    """--resident 1 needs the clips on disk and the counter-based draws; raises before the device is touched."""
    if not opt.resident:
        return
    if opt.synthetic != 0:
        raise RuntimeError("--resident 1 keeps the 3DV clips of --data_root in device memory: it needs --synthetic 0 "
                           "(got --synthetic %d, which reads no clip)" % opt.synthetic)
    if opt.view_rng != 'philox':
        raise RuntimeError("--resident 1 needs --view_rng philox: --view_rng %s draws every clip's random numbers on the host "
                           "per batch, which is the per-batch host work that resident clips remove" % opt.view_rng)


def check_knn_flags(opt, world=None):
    """--knn_every E > 0 needs the clips on disk and one rank (the sharded monitor does not exist); raises before the device
    is touched (`world` None: the launcher's WORLD_SIZE)."""
    if opt.knn_every < 0:
        raise RuntimeError("--knn_every must be >= 0 (got %d)" % opt.knn_every)
    if not opt.knn_every:
        return
    if opt.synthetic != 0:
        raise RuntimeError("--knn_every %d evaluates the train and test splits of --data_root: it needs --synthetic 0 "
                           "(got --synthetic %d, which has no labelled clips)" % (opt.knn_every, opt.synthetic))
    world = fdist.env_world_size() if world is None else world
    if world > 1:
        raise RuntimeError("--knn_every %d runs on one rank only (got %d ranks): the sharded monitor is not implemented"
                           % (opt.knn_every, world))
    if not 1 <= opt.knn_k <= 64:
        raise RuntimeError("--knn_k must be in 1..64 (got %d)" % opt.knn_k)
    if not opt.knn_T > 0:
        raise RuntimeError("--knn_T must be positive (got %r)" % opt.knn_T)


def check_queue_flags(opt, world=None):
    """--neg_queue L: L >= 0, a multiple of --batchSize (a push of one batch never wraps inside itself), one rank (a gathered
    push would add a collective to the step).  Raises before the device is touched (`world` None: the launcher's WORLD_SIZE)."""
    if opt.neg_queue < 0:
        raise RuntimeError("--neg_queue must be >= 0 (got %d)" % opt.neg_queue)
    if not opt.neg_queue:
        return
    if opt.neg_queue % opt.batchSize:
        raise RuntimeError("--neg_queue %d must be a multiple of --batchSize %d: every step stores one row per clip, and a "
                           "push must not wrap inside itself" % (opt.neg_queue, opt.batchSize))
    world = fdist.env_world_size() if world is None else world
    if world > 1:
        raise RuntimeError("--neg_queue %d runs on one rank only (got %d ranks): the gathered queue is not implemented"
                           % (opt.neg_queue, world))


def check_key_flags(opt, world=None):
    """--key_encoder 1 needs a queue to fill (--neg_queue L > 0), 0 <= --key_momentum < 1 and one rank (the queue's own limit).
    Raises before the device is touched (`world` None: the launcher's WORLD_SIZE)."""
    if not opt.key_encoder:
        return
    if not opt.neg_queue:
        raise RuntimeError("--key_encoder 1 supplies the rows of the negative queue: without --neg_queue L > 0 nothing would "
                           "read its keys")
    if not 0.0 <= opt.key_momentum < 1.0:                    # NaN fails both comparisons
        raise RuntimeError("--key_momentum must be in [0, 1) (got %r): at 1 the key encoder would never move" % opt.key_momentum)
    world = fdist.env_world_size() if world is None else world
    if world > 1:
        raise RuntimeError("--key_encoder 1 runs on one rank only (got %d ranks), like the queue it fills" % world)


def check_state_flags(opt, world=None):
    """--save_state_every E >= 0, --keep_states K >= 0; either of --save_state_every / --resume needs one rank (the per-rank
    generators are not in a rank-0 file).  Raises before the device is touched (`world` None: the launcher's WORLD_SIZE)."""
    if opt.save_state_every < 0 or opt.keep_states < 0:
        raise RuntimeError("--save_state_every and --keep_states must be >= 0 (got %d, %d)" % (opt.save_state_every, opt.keep_states))
    world = fdist.env_world_size() if world is None else world
    if world > 1:
        for flag, on in (("--resume %s" % opt.resume, bool(opt.resume)),
                         ("--save_state_every %d" % opt.save_state_every, bool(opt.save_state_every))):
            if on:
                raise RuntimeError("%s runs on one rank only (got %d ranks): the per-rank generators are not in a state file"
                                   % (flag, world))


OPTIM_FLAGS = ("adamw_decay", "clip_grad_norm", "lr_schedule", "warmup_steps", "lr_decay_epochs", "lr_min")


def _check_cosine_span(opt, steps):
    T = opt.lr_decay_epochs * steps
    if T <= opt.warmup_steps:
        raise RuntimeError("--lr_decay_epochs %d x %d steps per epoch = %d steps must exceed --warmup_steps %d: the cosine "
                           "starts where the warm-up ends" % (opt.lr_decay_epochs, steps, T, opt.warmup_steps))
    return T


def check_optim_flags(opt, world=None):
    """The optimizer recipe (facl_amd/optim.py): --adamw_decay, --clip_grad_norm, --lr_min finite and >= 0, --warmup_steps and
    --lr_decay_epochs >= 0; cosine needs --lr_decay_epochs >= 1 and more steps than the warm-up has (with --synthetic 0 the
    steps of an epoch are known only once the split is read: optim_recipe checks again); --lr_decay_epochs / --lr_min belong to
    cosine; one rank.  Raises before the device is touched (`world` None: the launcher's WORLD_SIZE)."""
    for name in ("adamw_decay", "clip_grad_norm", "lr_min"):
        v = getattr(opt, name)
        if not 0.0 <= v < float("inf"):                      # NaN fails both comparisons
            raise RuntimeError("--%s must be finite and >= 0 (got %r)" % (name, v))
    for name in ("warmup_steps", "lr_decay_epochs"):
        if getattr(opt, name) < 0:
            raise RuntimeError("--%s must be >= 0 (got %d)" % (name, getattr(opt, name)))
    if opt.lr_schedule == "cosine":
        if opt.lr_decay_epochs < 1:
            raise RuntimeError("--lr_schedule cosine needs --lr_decay_epochs >= 1 (got %d): the epochs over which the rate falls "
                               "to --lr_min" % opt.lr_decay_epochs)
        if opt.synthetic != 0:
            _check_cosine_span(opt, opt.steps_per_epoch)
    else:
        if opt.lr_decay_epochs:
            raise RuntimeError("--lr_decay_epochs %d is the span of --lr_schedule cosine (got --lr_schedule %s)"
                               % (opt.lr_decay_epochs, opt.lr_schedule))
        if opt.lr_min:
            raise RuntimeError("--lr_min %r is the end of --lr_schedule cosine (got --lr_schedule %s)" % (opt.lr_min, opt.lr_schedule))
    world = fdist.env_world_size() if world is None else world
    if world > 1:
        defaults = build_parser('0').parse_args([])
        for name in OPTIM_FLAGS:
            if getattr(opt, name) != getattr(defaults, name):
                raise RuntimeError("--%s %s runs on one rank only (got %d ranks): the optimizer recipe has never run "
                                   "data-parallel" % (name, getattr(opt, name), world))


def optim_recipe(opt, steps):
    """FusedAdam's keyword arguments for the recipe flags; `steps`: optimizer steps per epoch (T = --lr_decay_epochs x steps)."""
    kw = dict(weight_decay=opt.adamw_decay, max_grad_norm=opt.clip_grad_norm, schedule=opt.lr_schedule,
              warmup_steps=opt.warmup_steps, lr_min=opt.lr_min)
    if opt.lr_schedule == "cosine":
        kw["decay_steps"] = _check_cosine_span(opt, steps)
    return kw


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


def check_loss_flags(opt, world=None):
    """--loss_temperature finite and positive; --loss_mask exclude needs a negative, i.e. batch x world >= 2 key clips.  Raises
    before the device is touched (`world` None: the launcher's WORLD_SIZE)."""
    world = fdist.env_world_size() if world is None else world
    try:
        check_loss_mode(opt.loss_temperature, opt.loss_mask, opt.batchSize * world)
    except ValueError as e:
        raise RuntimeError("--loss_temperature / --loss_mask: %s" % e) from None


def check_class_mask_flags(opt, world=None):
    """--loss_mask class: one rank, labelled clips (--synthetic 0) and 0 < --label_fraction <= 1; --class_positives finite, >= 0
    and > 0 only with that mask.  Raises before the device is touched (`world` None: the launcher's WORLD_SIZE)."""
    try:
        check_class_positives(getattr(opt, "class_positives", 0.0), opt.loss_mask)
    except ValueError as e:
        raise RuntimeError("--class_positives: %s" % e) from None
    check_cluster_id_flags(opt, world)
    if opt.loss_mask != 'class':
        return
    world = fdist.env_world_size() if world is None else world
    if world > 1:
        raise RuntimeError("--loss_mask class runs on one rank only (got %d ranks): gathered class ids are not implemented" % world)
    if opt.synthetic != 0:
        raise RuntimeError("--loss_mask class masks the keys of clips with the anchor's action label: it needs --synthetic 0 "
                           "(got --synthetic %d, which has no labelled clips)" % opt.synthetic)
    if not 0.0 < opt.label_fraction <= 1.0:                  # NaN fails both comparisons
        raise RuntimeError("--label_fraction must be in (0, 1] (got %r)" % opt.label_fraction)


def check_cluster_id_flags(opt, world=None):
    """--class_ids cluster: the class ids of --loss_mask class are k-means cluster ids of the train split on disk.  Needs that
    mask, --synthetic 0, one rank, 2 <= --clusters <= 1024, --cluster_every >= 1; reads no label, so --label_fraction /
    --label_seed stay at their defaults; the ids are not in a state file, so neither --save_state_every nor --resume.  Raises
    before the device is touched (`world` None: the launcher's WORLD_SIZE); namespaces from before the flag hold `labels`."""
    if getattr(opt, "class_ids", "labels") != 'cluster':
        return
    if opt.loss_mask != 'class':
        raise RuntimeError("--class_ids cluster supplies the ids of --loss_mask class (got --loss_mask %s): nothing else reads them"
                           % opt.loss_mask)
    if opt.synthetic != 0:
        raise RuntimeError("--class_ids cluster extracts and clusters the train split of --data_root: it needs --synthetic 0 "
                           "(got --synthetic %d, which has no clips on disk)" % opt.synthetic)
    world = fdist.env_world_size() if world is None else world
    if world > 1:
        raise RuntimeError("--class_ids cluster runs on one rank only (got %d ranks): the sharded extraction is not implemented" % world)
    if not 2 <= opt.clusters <= 1024:
        raise RuntimeError("--class_ids cluster needs --clusters K in 2..1024 (got %d)" % opt.clusters)
    if opt.cluster_every < 1:
        raise RuntimeError("--class_ids cluster needs --cluster_every E >= 1 (got %d)" % opt.cluster_every)
    if opt.cluster_iters < 1 or opt.cluster_restarts < 1:
        raise RuntimeError("--cluster_iters and --cluster_restarts must be >= 1 (got %d, %d)" % (opt.cluster_iters, opt.cluster_restarts))
    if opt.label_fraction != 1.0 or opt.label_seed != 0:
        raise RuntimeError("--class_ids cluster reads no label: --label_fraction %r / --label_seed %d select labels and have "
                           "nothing to act on" % (opt.label_fraction, opt.label_seed))
    if opt.save_state_every or opt.resume:
        raise RuntimeError("--class_ids cluster with --save_state_every / --resume: the cluster ids of the clips are not part "
                           "of a state file, so a resumed run could not continue with them")


def check_proto_flags(opt, world=None):
    """--proto_weight w: finite and >= 0, and w > 0 only with --class_ids cluster, whose centroids are the prototypes (that flag
    already implies one rank, --synthetic 0, --loss_mask class and no state files); --proto_temperature finite and > 0.  Raises
    before the device is touched; namespaces from before the flags hold the defaults."""
    w, t = float(getattr(opt, "proto_weight", 0.0)), float(getattr(opt, "proto_temperature", 0.2))
    if not (w >= 0.0 and math.isfinite(w)):                  # NaN fails the comparison
        raise RuntimeError("--proto_weight must be finite and >= 0 (got %r)" % w)
    if not (t > 0.0 and math.isfinite(t)):
        raise RuntimeError("--proto_temperature must be finite and > 0 (got %r)" % t)
    if w > 0 and getattr(opt, "class_ids", "labels") != 'cluster':
        raise RuntimeError("--proto_weight %g needs --class_ids cluster: the prototypes are the centroids of its k-means" % w)
    if w > 0:
        check_cluster_id_flags(opt, world)


def split_class_ids(labels, fraction, seed):
    """The class id of every clip of a labelled split as the class-aware mask sees it: the clip's label inside the stratified
    `label_subset` (facl_amd/finetune.py: nested in `fraction` for one seed), -1 outside.  (N,) int32; pure host code."""
    from .finetune import label_subset
    labels = np.asarray(labels, dtype=np.int64).reshape(-1)
    ids = np.full(labels.shape, -1, dtype=np.int32)
    keep = label_subset(labels, fraction, seed)
    ids[keep] = labels[keep]
    return ids


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
    queue = getattr(step, "queue", None)
    if queue is not None and queue.ids is not None:
        queue.ids.fill_(-1)
    return ids, info


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


def train_epochs(opt, step, source, world, lr_step, next_batch, after_epoch, after_step=None, start_epoch=0, end_of_epoch=None):
    """The epoch loop of the training entries under StepLR(`lr_step`, 0.7).  `source`: the TrainBatches of --synthetic 0, else
    None (--steps_per_epoch steps).  The entries differ in `next_batch(disk, epoch, i)` -> the step's input (`disk`: the epoch's
    iterator of `source`, or None), `after_step(what the step returned)` and `after_epoch(epoch, mean_loss, clips_per_s)` --
    with --clip_grad_norm on it gets a fourth argument, the ' | grad norm ...' tail of the epoch line.  Under --lr_schedule cosine
    the optimizer keeps the base rate and its device-side schedule does the rest.
    `start_epoch`: the first epoch run (a resumed run's).  `end_of_epoch(epoch)`: called last in every epoch, when the epoch's
    producer thread has stopped, so that the view generator's state is the one the next epoch starts from."""
    steps = opt.steps_per_epoch if source is None else source.steps
    run_step = step
    cosine = getattr(opt, "lr_schedule", "step") == "cosine"     # namespaces from before the recipe flags: the reference's StepLR
    max_norm = float(getattr(opt, "clip_grad_norm", 0.0))
    for epoch in range(start_epoch, opt.nepoch):
        step.netR.train()
        if getattr(step, "key_encoder", None) is not None:
            step.key_encoder.key.train()                 # MoCo's convention: the key copy normalises with batch statistics too
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
        after_epoch(epoch, loss_sigma / steps, opt.batchSize * steps * world / (time.time() - t0), *extra)
        if end_of_epoch is not None:
            end_of_epoch(epoch)


def run(default_branch, ckpt_pattern, args=None):
    opt = build_parser(default_branch).parse_args(args)
    print(opt)
    check_resident_flags(opt)
    check_view_flags(opt)
    check_knn_flags(opt)
    check_loss_flags(opt)
    check_class_mask_flags(opt)
    check_proto_flags(opt)
    check_queue_flags(opt)
    check_key_flags(opt)
    check_state_flags(opt)
    check_optim_flags(opt)
    recipe = view_recipe(opt)
    if opt.synthetic != 1:
        print(recipe.describe())
    from . import train_state
    flags = train_state.flags_of(opt)                  # as given: the grouper writes the reference's literals into `opt` later
    resumed, resumed_path = load_resume_state(opt)     # on the CPU, refused here if its options differ from this run's
    local = int(os.environ.get("LOCAL_RANK", opt.main_gpu))
    torch.cuda.set_device(local)               # before the process group: RCCL binds its communicator to the current device
    device = torch.device("cuda", local)
    rank, world = fdist.init_from_env()
    setup_run(opt)

    num_crop = opt.num_crop
    netR = MODELL.PointNet_Plus(opt, gost=num_crop).to(device)
    netR.precision = opt.precision
    netR.bn_reduce_fn = fdist.make_bn_reduce_fn()
    source = TrainBatches(opt, device, rank, world, report_ingest=rank == 0, too_few="the split has %(clips)d clips: fewer "
                          "than one batch of %(batch)d per rank x %(world)d ranks") if opt.synthetic == 0 else None
    steps = opt.steps_per_epoch if source is None else source.steps
    # cn3d_train_motion_GL.py:180: the same update as torch.optim.Adam, all tensors in one HIP launch (facl_amd/optim.py); the
    # recipe flags (all off by default) add decay, clipping and the device-side schedule, which counts in steps of an epoch
    from .optim import FusedAdam
    optimizer = FusedAdam(netR.parameters(), lr=opt.learning_rate, betas=(0.5, 0.999), eps=1e-06, **optim_recipe(opt, steps))
    step = ContrastiveStep(netR, optimizer, opt, num_crop, opt.group_radius, bool(opt.fps_reorder), opt.swa_if, opt.cld_if)
    gen = torch.Generator(device=device)
    gen.manual_seed(1000 + rank)
    view_rng = np.random.RandomState(2000 + rank)         # --synthetic 2: the generator the view construction draws from
    class_of = None
    if opt.loss_mask == 'class' and opt.class_ids == 'cluster':
        # no label is read: every clip is unknown (the class mask is then the exclude mask) until the first clustering
        class_of = {source.index.v_name(int(v)): -1 for v in source.split}
        print('class mask: cluster ids, %d clusters, every %d epoch(s); %d train clips unknown until the first clustering'
              % (opt.clusters, opt.cluster_every, len(class_of)))
        if opt.class_positives:
            print('class positives: weight %g' % opt.class_positives)
    elif opt.loss_mask == 'class':
        # every clip trains; the stratified subset keeps its label as class id, every other clip is unknown (-1)
        ids = split_class_ids([source.index.label(int(v)) for v in source.split], opt.label_fraction, opt.label_seed)
        class_of = {source.index.v_name(int(v)): int(c) for v, c in zip(source.split, ids)}
        print('class mask: %d of %d train clips labelled, %d classes' % (int((ids >= 0).sum()), len(ids), len(np.unique(ids[ids >= 0]))))
        if opt.class_positives:
            print('class positives: weight %g' % opt.class_positives)

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
        data = None
        if cluster_now:                                      # the train split is extracted once for both monitors
            data = extract_monitor_splits(netR, opt, device, test=knn_now, what="--class_ids cluster")
            ftr, ytr, names = data[0]
            ids, info = recluster(step, class_of, ftr, names, opt.clusters, opt.cluster_iters, opt.cluster_restarts,
                                  opt.cluster_seed + epoch)
            # the split is labelled on disk anyway: acc / nmi against the true labels are printed as a monitor ONLY -- the
            # training never sees those labels, its class ids are the cluster numbers above
            from . import cluster as fcl
            table = fcl.contingency(ids, ytr.cpu().numpy())
            sizes = np.sort(info['sizes'])
            line = ('clusters: %d objective: %.6f iters: %d sizes min/median/max: %d/%g/%d | acc: %.2f nmi: %.4f'
                    % (opt.clusters, info['objective'], info['n_iter'], sizes[0], float(np.median(sizes)), sizes[-1],
                       fcl.matched_accuracy(table), fcl.nmi(table)))
            logging.info('{} --epoch{} =={}'.format('Valid', epoch, line))
            print('epoch:', epoch, line)
            if step.proto_weight > 0:
                # the ids a step saw so far came from the previous clustering (or were -1): any of them >= K raises here
                step.check_proto_err()
                from .knn_eval import knn_topk
                from .proto import concentrations
                cos_own = knn_topk(ftr[:, ftr.shape[1] - 512:], info["centroids"], 1)[0][:, 0]
                scale = concentrations(cos_own.cpu().numpy(), ids, opt.clusters, opt.proto_temperature, opt.proto_concentration)
                step.set_prototypes(info["centroids"], scale)
                phi = 1.0 / scale.astype(np.float64)
                line = 'prototypes: %d concentration min/mean/max: %.6g/%.6g/%.6g' % (opt.clusters, phi.min(), phi.mean(), phi.max())
                logging.info('{} --epoch{} =={}'.format('Valid', epoch, line))
                print('epoch:', epoch, line)
        if knn_now:
            top1 = knn_monitor(netR, opt, device, data)
            logging.info('{} --epoch{} ==knn top1:{}'.format('Valid', epoch, top1))
            print('epoch:', epoch, 'knn top1:', top1)
        if rank == 0 and epoch % 5 == 0:
            path = ckpt_pattern % (opt.save_root_dir, epoch)
            torch.save(netR.state_dict(), path)
            if step.key_encoder is not None:                 # the model's format: extract_* / finetune --checkpoint load it
                torch.save(step.key_encoder.state_dict(), key_checkpoint_name(path))

    source_rng = None if source is None else source.view_rng

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

    start_epoch = 0
    if resumed is not None:
        # after setup_run has reseeded and every lazily created piece can be created eagerly (ContrastiveStep.load_state_dict)
        netR.load_state_dict(resumed["model"], strict=True)
        optimizer.load_state_dict(resumed["optimizer"])
        step.load_state_dict(resumed)
        train_state.apply_rng(resumed["rng"], gen, view_rng, source_rng)
        start_epoch = resumed["epoch"] + 1
        print('resumed from %s: epoch %d' % (resumed_path, start_epoch))
    train_epochs(opt, step, source, world, lr_step=4, next_batch=next_batch, after_epoch=after_epoch,
                 start_epoch=start_epoch, end_of_epoch=end_of_epoch)
    return netR
