"""Shared body of the feature-extraction entries: counterpart of the loop of
training_code/extract_motion_feature.py:143-221 -- load a checkpoint into PointNet_Plus, eval() (BatchNorm folded from
the running statistics: the SA point-MLP then runs as fwd2 + fwd3 + pool with no statistics passes), group, forward,
``cat((x, x_global), 0)`` -> one (num_crop+1)*512 float32 vector per clip."""
import os

import numpy as np
import torch

from . import cn3d_model_conbag as MM
from .train_common import synthetic_batch
from .train_flags import build_parser, check_view_flags, view_recipe
from .train_step import group_views


def save_single_feature(feature, save_path, name, num_crop=11):
    """extract_motion_feature.py:217-221: (num_crop*B, 512) rows [view-major x | x_global] -> per-clip vectors."""
    feature = feature.reshape(num_crop, -1, 512).transpose(1, 0, 2).reshape(-1, num_crop * 512)
    for batch_i in range(feature.shape[0]):
        np.save(os.path.join(save_path, name[batch_i] + '.npy'), feature[batch_i])
    return feature


def extract_batch(netR, out_points, opt, group_radius=None):
    """(B,G,N,D) clips -> (B, (G+1)*512) features, exactly the reference's per-batch body (:171-182)."""
    B, G, N, D = out_points.shape
    data1 = out_points.permute(1, 0, 2, 3).reshape(-1, N, D).float()
    xt, yt = group_views(data1, opt, group_radius)
    x, _, _, x_global = netR(xt, yt)
    feat = torch.cat((x, x_global), dim=0)
    return feat.reshape(G + 1, B, 512).permute(1, 0, 2).reshape(B, (G + 1) * 512)


def run(default_branch, default_ckpt, args=None):
    p = build_parser(default_branch)
    p.add_argument('--checkpoint', type=str, default=default_ckpt, help='NEW: state_dict to load (reference: literal path)')
    p.add_argument('--save_path', type=str, default='', help='NEW: output folder for <clip>.npy (reference: literal path)')
    p.add_argument('--num_batches', type=int, default=2, help='NEW: synthetic batches to extract')
    opt = p.parse_args(args)
    view_recipe(opt)                              # refuses a bad recipe before the device is touched
    device = torch.device("cuda", opt.main_gpu)
    torch.cuda.set_device(device)
    netR = MM.PointNet_Plus(opt, gost=opt.num_crop)
    netR.load_state_dict(torch.load(opt.checkpoint, map_location="cpu", weights_only=True))
    netR = netR.to(device).eval()
    if opt.save_path:
        os.makedirs(opt.save_path, exist_ok=True)
    if opt.synthetic == 0:
        return run_disk(netR, opt, device)
    gen = torch.Generator(device=device)
    gen.manual_seed(7)
    feats = []
    with torch.no_grad():
        for i in range(opt.num_batches):
            pts = synthetic_batch(opt.batchSize, opt.num_crop, opt.SAMPLE_NUM, opt.INPUT_FEATURE_NUM, device, gen)
            f = extract_batch(netR, pts, opt, opt.group_radius).cpu().numpy()
            feats.append(f)
            if opt.save_path:
                for b in range(f.shape[0]):
                    np.save(os.path.join(opt.save_path, 'synthetic_%04d_%03d.npy' % (i, b)), f[b])
    return np.concatenate(feats)


def ordered_views(opt, device, index, split, rng, epoch=0):
    """The evaluation pass: the clips `split` (dataset indices) in order, batches of --batchSize with the last one ragged, as
    ((G*B, N, 4) views, v_names, labels); views drawn from `rng` (--view_rng numpy) or keyed by (2000, epoch, index) (philox;
    `epoch` > 0: a further test-time draw of facl_amd.predict)."""
    from . import dataset as fds
    vids = [np.asarray(split, dtype=np.int64)[p] for p in fds.ordered_batches(len(split), opt.batchSize)]
    return iter(fds.DiskBatches(index, opt.data_root, opt.branch_choose, vids, opt.view_rng, device, rng=rng, seed=2000,
                                epoch=epoch, prefetch=bool(opt.prefetch), num_crop=opt.num_crop, num_point=opt.SAMPLE_NUM,
                                recipe=view_recipe(opt)))


def extract_split(netR, opt, device, index, split, rng, save_path=''):
    """One split of `run_disk`, drawn by `ordered_views`.  Returns the (clips, (num_crop+1)*512) float32 features as a
    DEVICE tensor; with `save_path` every clip is also written to <save_path>/<v_name>.npy as its batch completes.  The
    caller holds torch.no_grad() and has put `netR` in eval()."""
    feats = []
    for views, names, _ in ordered_views(opt, device, index, split, rng):
        B = len(names)
        clip_major = views.view(opt.num_crop, B, opt.SAMPLE_NUM, 4).permute(1, 0, 2, 3)
        f = extract_batch(netR, clip_major, opt, opt.group_radius)
        feats.append(f)
        if save_path:
            fh = f.cpu().numpy()
            for b, n in enumerate(names):
                np.save(os.path.join(save_path, n + '.npy'), fh[b])
    if not feats:
        return torch.zeros((0, (opt.num_crop + 1) * 512), dtype=torch.float32, device=device)
    return torch.cat(feats)


def run_disk(netR, opt, device):
    """--synthetic 0: extract_motion_feature.py:112-214 -- the train split, then the test split, of the clips listed in
    <data_root>/raw, in order (shuffle=False, drop_last=False: the last batch is ragged); one <v_name>.npy per clip.
    Returns the (clips, (num_crop+1)*512) features in that order.  With --view_rng philox any --num_crop / --SAMPLE_NUM of
    the view kernels' domain (a vector is (num_crop+1)*512 long whatever SAMPLE_NUM is)."""
    from . import dataset as fds
    check_view_flags(opt)
    print(view_recipe(opt).describe())
    index = fds.ClipIndex.from_dir(os.path.join(opt.data_root, fds.EXTRACT_LIST_DIR), opt.dataset)
    rng = np.random.RandomState(2000)
    feats = []
    with torch.no_grad():
        for split in (index.select(opt.split, full_train=bool(opt.full_train)), index.select(opt.split, test=True)):
            if len(split):
                feats.append(extract_split(netR, opt, device, index, split, rng, opt.save_path).cpu().numpy())
    return np.concatenate(feats) if feats else np.zeros((0, (opt.num_crop + 1) * 512), np.float32)
