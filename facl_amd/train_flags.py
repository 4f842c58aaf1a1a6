"""The flags of the training entries: parser, defaults and checks.  No torch, no HIP library at module level (a check imports its own)."""
import argparse
import math
import os


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


def add_optimizer_flags(p):
    """--optim and the four flags of SGD / LARS (facl_amd.optim.FusedSGD), the training entries' own: build_parser is
    also the parser of the extraction and prediction entries, which have no optimizer.  The reference's --momentum and
    --weight_decay stay parsed and unread; where `p` has them their help says so."""
    p.add_argument('--optim', type=str, default='adam', choices=('adam', 'sgd', 'lars'),
                   help='NEW (one rank for sgd / lars): adam = the reference\'s Adam; sgd = SGD with momentum; lars = SGD with '
                        'momentum on layer-wise adapted gradients (facl_amd.optim.FusedSGD); --clip_grad_norm and the schedule '
                        'flags apply to all three')
    p.add_argument('--sgd_momentum', type=float, default=0.9, help='NEW (--optim sgd / lars): the momentum, 0 <= m < 1')
    p.add_argument('--sgd_nesterov', type=int, default=0, choices=(0, 1), help='NEW (--optim sgd / lars): 1 = Nesterov momentum')
    p.add_argument('--sgd_weight_decay', type=float, default=0.0,
                   help='NEW (--optim sgd / lars): L2 weight decay on every weight matrix and convolution kernel; biases and '
                        'BatchNorm gamma / beta are not decayed')
    p.add_argument('--lars_eta', type=float, default=0.001,
                   help='NEW (--optim lars): the trust coefficient of eta |w| / (|g| + wd |w|), on the tensors that are decayed')
    unread = {"momentum": "--sgd_momentum", "weight_decay": "--sgd_weight_decay"}
    for a in p._actions:
        if a.dest in unread:
            a.help += "; parsed and never read, as in the reference: %s is the live one" % unread[a.dest]
    return p


def train_parser(default_branch):
    """The parser of the two pre-training entries: build_parser's flags and the optimizer's."""
    return add_optimizer_flags(build_parser(default_branch))


def finetune_train_parser():
    """The parser of the fine-tuning entry: finetune_parser's flags and the optimizer's."""
    return add_optimizer_flags(finetune_parser())


def finetune_parser():
    p = build_parser('0')
    p.description = "Supervised fine-tuning"
    p.add_argument('--checkpoint', type=str, default='', help='NEW: encoder state_dict to start from; empty = from scratch')
    p.add_argument('--num_class', type=int, default=0, help='NEW: classes of the head (0 = 60 for ntu60, 120 for ntu120)')
    # --label_fraction / --label_seed: build_parser's (the pre-training entries read them for --loss_mask class); here they
    # narrow the train split to the labelled subset
    p.add_argument('--eval_every', type=int, default=1, help='NEW (--synthetic 0): test top-1 after every E-th epoch; 0 = off')
    p.add_argument('--freeze_bn', type=int, default=0, choices=(0, 1),
                   help='NEW: 1 = fine-tune with frozen BatchNorm: the model stays in eval() for the training step, the running '
                        'statistics of --checkpoint (required) are kept, all weights train; the step runs eager')
    return p


# ---- the one source of defaults: the parsers' own, computed once
FLAG_DEFAULTS = vars(finetune_parser().parse_args([]))         # build_parser's flags and the four of fine-tuning
VIEW_RECIPE_FLAGS = ("view_kinds", "jitter_sigma", "jitter_clip", "rot_range", "scale_lo", "scale_hi", "tilt_angle")
VIEW_RECIPE_DEFAULTS = tuple(FLAG_DEFAULTS[k] for k in VIEW_RECIPE_FLAGS)   # = ("reference",) + facl_amd.philox.DEFAULT_STRENGTHS
OPTIM_FLAGS = ("adamw_decay", "clip_grad_norm", "lr_schedule", "warmup_steps", "lr_decay_epochs", "lr_min")
SGD_FLAGS = ("sgd_momentum", "sgd_nesterov", "sgd_weight_decay", "lars_eta")        # read under --optim sgd / lars only
OPTIMIZER_FLAG_DEFAULTS = vars(add_optimizer_flags(argparse.ArgumentParser()).parse_args([]))   # --optim and the four


def with_defaults(opt):
    """A new namespace of every flag: `opt`'s value where it has the name (bench.py builds a bare one), else the parser's default."""
    return argparse.Namespace(**{k: getattr(opt, k, d) for k, d in FLAG_DEFAULTS.items()})


def env_world_size():
    """The launcher's WORLD_SIZE (torch.distributed.run); 1 without a launcher."""
    return int(os.environ.get("WORLD_SIZE", "1"))


def optimizer_flags(opt):
    """A new namespace of --optim and the four SGD flags: `opt`'s value where it has the name (a namespace of build_parser or a
    bare one has none), else the parser's default, Adam."""
    return argparse.Namespace(**{k: getattr(opt, k, d) for k, d in OPTIMIZER_FLAG_DEFAULTS.items()})


def one_rank_only(flag, clause, world=None):
    """The refusal of what has never run data-parallel: `flag` as the user wrote it, `clause` the reason with its punctuation."""
    world = env_world_size() if world is None else world
    if world > 1:
        raise RuntimeError("%s runs on one rank only (got %d ranks)%s" % (flag, world, clause))


def view_recipe(opt):
    """The facl_amd.philox.Recipe of the seven flags (a namespace without them: the default), checked.  Any non-default value
    needs the counter-based draws on clips: refused with --view_rng numpy / device and with --synthetic 1.  Touches no device."""
    from .philox import Recipe
    o = with_defaults(opt)
    given = [getattr(o, k) for k in VIEW_RECIPE_FLAGS]
    try:
        recipe = Recipe.parse(given[0], **dict(zip(VIEW_RECIPE_FLAGS[1:], given[1:])))
    except ValueError as e:
        raise RuntimeError(str(e)) from None
    if not recipe.is_default():
        changed = ", ".join("--%s %s" % (k, v) for k, v, d in zip(VIEW_RECIPE_FLAGS, given, VIEW_RECIPE_DEFAULTS) if v != d)
        if o.synthetic == 1:
            raise RuntimeError("%s with --synthetic 1: iid clouds are no views of a clip, and the reference's stream defines its "
                               "ten views only; a view recipe needs --synthetic 0 or 2 with --view_rng philox" % changed)
        if o.view_rng != 'philox':
            raise RuntimeError("%s with --view_rng %s: the reference's stream defines its ten views only (the kinds and "
                               "strengths of cn3D_data_set.py:285-350); another recipe needs --view_rng philox, whose "
                               "counter-based draws cover it" % (changed, o.view_rng))
    return recipe


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
    one_rank_only("--knn_every %d" % opt.knn_every, ": the sharded monitor is not implemented", world)
    if not 1 <= opt.knn_k <= 64:
        raise RuntimeError("--knn_k must be in 1..64 (got %d)" % opt.knn_k)
    if not opt.knn_T > 0:
        raise RuntimeError("--knn_T must be positive (got %r)" % opt.knn_T)


def check_loss_flags(opt, world=None):
    """--loss_temperature finite and positive; --loss_mask exclude needs a negative, i.e. batch x world >= 2 key clips.  Raises
    before the device is touched (`world` None: the launcher's WORLD_SIZE)."""
    from .utils_my import check_loss_mode
    world = env_world_size() if world is None else world
    try:
        check_loss_mode(opt.loss_temperature, opt.loss_mask, opt.batchSize * world)
    except ValueError as e:
        raise RuntimeError("--loss_temperature / --loss_mask: %s" % e) from None


def check_class_mask_flags(opt, world=None):
    """--loss_mask class: one rank, labelled clips (--synthetic 0) and 0 < --label_fraction <= 1; --class_positives finite, >= 0
    and > 0 only with that mask.  Raises before the device is touched (`world` None: the launcher's WORLD_SIZE)."""
    from .utils_my import check_class_positives
    try:
        check_class_positives(with_defaults(opt).class_positives, opt.loss_mask)
    except ValueError as e:
        raise RuntimeError("--class_positives: %s" % e) from None
    check_cluster_id_flags(opt, world)
    if opt.loss_mask != 'class':
        return
    one_rank_only("--loss_mask class", ": gathered class ids are not implemented", world)
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
    if with_defaults(opt).class_ids != 'cluster':
        return
    if opt.loss_mask != 'class':
        raise RuntimeError("--class_ids cluster supplies the ids of --loss_mask class (got --loss_mask %s): nothing else reads them"
                           % opt.loss_mask)
    if opt.synthetic != 0:
        raise RuntimeError("--class_ids cluster extracts and clusters the train split of --data_root: it needs --synthetic 0 "
                           "(got --synthetic %d, which has no clips on disk)" % opt.synthetic)
    one_rank_only("--class_ids cluster", ": the sharded extraction is not implemented", world)
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
    o = with_defaults(opt)
    w, t = float(o.proto_weight), float(o.proto_temperature)
    if not (w >= 0.0 and math.isfinite(w)):                  # NaN fails the comparison
        raise RuntimeError("--proto_weight must be finite and >= 0 (got %r)" % w)
    if not (t > 0.0 and math.isfinite(t)):
        raise RuntimeError("--proto_temperature must be finite and > 0 (got %r)" % t)
    if w > 0 and o.class_ids != 'cluster':
        raise RuntimeError("--proto_weight %g needs --class_ids cluster: the prototypes are the centroids of its k-means" % w)
    if w > 0:
        check_cluster_id_flags(opt, world)


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
    one_rank_only("--neg_queue %d" % opt.neg_queue, ": the gathered queue is not implemented", world)


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
    one_rank_only("--key_encoder 1", ", like the queue it fills", world)


def check_state_flags(opt, world=None):
    """--save_state_every E >= 0, --keep_states K >= 0; either of --save_state_every / --resume needs one rank (the per-rank
    generators are not in a rank-0 file).  Raises before the device is touched (`world` None: the launcher's WORLD_SIZE)."""
    if opt.save_state_every < 0 or opt.keep_states < 0:
        raise RuntimeError("--save_state_every and --keep_states must be >= 0 (got %d, %d)" % (opt.save_state_every, opt.keep_states))
    for flag, on in (("--resume %s" % opt.resume, bool(opt.resume)),
                     ("--save_state_every %d" % opt.save_state_every, bool(opt.save_state_every))):
        if on:
            one_rank_only(flag, ": the per-rank generators are not in a state file", world)


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
    for name in OPTIM_FLAGS:
        if getattr(opt, name) != FLAG_DEFAULTS[name]:
            one_rank_only("--%s %s" % (name, getattr(opt, name)), ": the optimizer recipe has never run data-parallel", world)


def check_sgd_flags(opt, world=None):
    """--optim sgd / lars: one rank; --sgd_momentum in [0, 1), --sgd_weight_decay and --lars_eta finite and >= 0, eta > 0 under lars;
    --adamw_decay is Adam's decay and is refused.  --optim adam: the four flags stay at their defaults.  Raises before the device
    is touched (`world` None: the launcher's WORLD_SIZE); namespaces without the flags hold the defaults."""
    o = optimizer_flags(opt)
    adamw_decay = with_defaults(opt).adamw_decay
    if o.optim == "adam":
        for name in SGD_FLAGS:
            if getattr(o, name) != OPTIMIZER_FLAG_DEFAULTS[name]:
                raise RuntimeError("--%s %s belongs to --optim sgd / lars (got --optim adam, which does not read it)"
                                   % (name, getattr(o, name)))
        return
    if o.optim not in ("sgd", "lars"):
        raise RuntimeError("--optim must be adam, sgd or lars (got %r)" % (o.optim,))
    one_rank_only("--optim %s" % o.optim, ": the optimizer has never run data-parallel", world)
    if adamw_decay:
        raise RuntimeError("--adamw_decay %r is the decoupled decay of --optim adam: --optim %s takes --sgd_weight_decay"
                           % (adamw_decay, o.optim))
    if not 0.0 <= o.sgd_momentum < 1.0:                      # NaN fails both comparisons
        raise RuntimeError("--sgd_momentum must be in [0, 1) (got %r)" % o.sgd_momentum)
    for name in ("sgd_weight_decay", "lars_eta"):
        v = getattr(o, name)
        if not 0.0 <= v < float("inf"):
            raise RuntimeError("--%s must be finite and >= 0 (got %r)" % (name, v))
    if o.optim == "lars" and not o.lars_eta > 0.0:
        raise RuntimeError("--optim lars needs --lars_eta > 0 (got %r): at 0 no masked tensor would move" % o.lars_eta)


def optim_recipe(opt, steps):
    """FusedAdam's keyword arguments for the recipe flags; `steps`: optimizer steps per epoch (T = --lr_decay_epochs x steps)."""
    kw = dict(weight_decay=opt.adamw_decay, max_grad_norm=opt.clip_grad_norm, schedule=opt.lr_schedule,
              warmup_steps=opt.warmup_steps, lr_min=opt.lr_min)
    if opt.lr_schedule == "cosine":
        kw["decay_steps"] = _check_cosine_span(opt, steps)
    return kw


def describe_optimizer(opt):
    """The entries' line about an optimizer other than Adam; None under --optim adam."""
    o = optimizer_flags(opt)
    if o.optim == "adam":
        return None
    return "optimizer: %s momentum %g nesterov %d weight decay %g%s" % (
        o.optim, o.sgd_momentum, o.sgd_nesterov, o.sgd_weight_decay, " eta %g" % o.lars_eta if o.optim == "lars" else "")


def make_optimizer(opt, params, steps):
    """The optimizer of the training entries for --optim: FusedAdam as cn3d_train_motion_GL.py:180 sets it (lr, betas (0.5, 0.999),
    eps 1e-6) with the recipe flags, or FusedSGD (plain / LARS) with the same clipping and schedule.  `steps`: optimizer steps per
    epoch.  A namespace without --optim gets Adam."""
    from .optim import FusedAdam, FusedSGD
    o = optimizer_flags(opt)
    kw = optim_recipe(opt, steps)
    if o.optim == "adam":
        return FusedAdam(params, lr=opt.learning_rate, betas=(0.5, 0.999), eps=1e-06, **kw)
    kw.pop("weight_decay")                                   # --adamw_decay: refused with these (check_sgd_flags)
    return FusedSGD(params, lr=opt.learning_rate, momentum=o.sgd_momentum, nesterov=bool(o.sgd_nesterov),
                    weight_decay=o.sgd_weight_decay, lars=o.optim == "lars", lars_eta=o.lars_eta, **kw)


def check_train_flags(opt, world=None):
    """Every check of the pre-training entries; a run with two mistakes reports the first in this order: the data (resident clips,
    views), the monitor, the loss (modes, class mask and ids, prototypes), its queue and key encoder, state files, the optimizer."""
    check_resident_flags(opt)
    check_view_flags(opt)
    for check in (check_knn_flags, check_loss_flags, check_class_mask_flags, check_proto_flags, check_queue_flags,
                  check_key_flags, check_state_flags, check_optim_flags, check_sgd_flags):
        check(opt, world)


# ---- fine-tuning: the inherited flags that belong to the contrastive loss are refused when they leave their parser default
_XENT_ONLY = ": fine-tuning has the cross-entropy only"
FINETUNE_REFUSED = (                                          # (the flags as the user writes them, their names, the clause)
    ("--knn_every", ("knn_every",), " belongs to the pre-training entries; fine-tuning reports its own test top-1 (--eval_every)"),
    ("--swa_if / --cld_if", ("swa_if", "cld_if"), " are terms of the contrastive loss" + _XENT_ONLY),
    ("--loss_normalize / --loss_temperature / --loss_mask", ("loss_normalize", "loss_temperature", "loss_mask"),
     " shape the contrastive loss" + _XENT_ONLY),
    ("--class_positives", ("class_positives",), " adds positives to the contrastive loss" + _XENT_ONLY),
    ("--class_ids", ("class_ids",), " supplies the class ids of the contrastive loss's mask" + _XENT_ONLY),
    ("--proto_weight", ("proto_weight",), " adds the prototype term to the contrastive loss" + _XENT_ONLY),
    ("--neg_queue", ("neg_queue",), " holds negatives of the contrastive loss" + _XENT_ONLY),
    ("--key_encoder", ("key_encoder",), " fills the negative queue of the contrastive loss" + _XENT_ONLY),
)


def check_finetune_flags(opt, world=None):
    """One rank, labelled clips or synthetic ones; raises before the device is touched (`world` None: the launcher's WORLD_SIZE)."""
    one_rank_only("fine-tuning", ": data-parallel fine-tuning is not implemented", world)
    if opt.synthetic not in (0, 1):
        raise RuntimeError("fine-tuning reads the labelled clips of --data_root (--synthetic 0) or synthetic clouds with "
                           "random labels (--synthetic 1); got --synthetic %d" % opt.synthetic)
    if not 0.0 < opt.label_fraction <= 1.0:
        raise RuntimeError("--label_fraction must be in (0, 1] (got %r)" % opt.label_fraction)
    if opt.eval_every < 0:
        raise RuntimeError("--eval_every must be >= 0 (got %d)" % opt.eval_every)
    o = with_defaults(opt)
    for flags, names, clause in FINETUNE_REFUSED:
        if any(getattr(o, n) != FLAG_DEFAULTS[n] for n in names):
            raise RuntimeError(flags + clause)
    if not opt.num_class:
        opt.num_class = 60 if opt.dataset == 'ntu60' else 120
    if not 2 <= opt.num_class <= 1024 or opt.num_class % 4:
        raise RuntimeError("--num_class must be a multiple of 4 in 2..1024 (got %d)" % opt.num_class)
    if not 1 <= opt.num_crop <= 64:
        raise RuntimeError("--num_crop must be in 1..64 (got %d)" % opt.num_crop)
    if o.freeze_bn and not opt.checkpoint:
        raise RuntimeError("--freeze_bn 1 keeps the running statistics of a pre-trained encoder: it needs --checkpoint (the "
                           "initial statistics, mean 0 and variance 1, describe no data)")


def check_finetune_train_flags(opt, world=None):
    """check_train_flags' counterpart for the fine-tuning entry: its own check first (it settles the one rank)."""
    check_finetune_flags(opt, world)
    check_resident_flags(opt)
    check_view_flags(opt)
    check_optim_flags(opt, world=1)
    check_sgd_flags(opt, world=1)
