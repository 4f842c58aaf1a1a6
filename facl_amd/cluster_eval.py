"""Label-free clustering evaluation of extracted features, beside the linear probe (``facl_amd.linear_classify``, the counterpart
of linear_classify/linercls.py) and the weighted kNN (``facl_amd.knn_eval``); the reference has no such entry.  The features of
one split are clustered by spherical k-means on the device (``facl_amd.cluster``) and the clusters are scored against the action
labels, which the clustering never sees: accuracy under the best one-to-one matching of clusters to classes, NMI, ARI, purity."""
import argparse

import numpy as np
import torch

from . import cluster as fcl


def build_parser():
    from . import dataset as fds
    p = argparse.ArgumentParser(description="Clustering evaluation of extracted features")
    p.add_argument('--dataset', type=str, default='ntu120', help='ntu120 | ntu60')
    p.add_argument('--main_gpu', type=int, default=0, help='main GPU id')
    p.add_argument('--data_root', type=str, default='../ntu/3DV_ntu60', help='the dataset root (as the linear probe)')
    p.add_argument('--split', type=str, default='view', choices=fds.SPLIT_MODES, help='view | subject | set')
    p.add_argument('--full_train', type=int, default=1, help='(--split subject): 0 = without the validation performers')
    p.add_argument('--motion_feature_dir', type=str, required=True, help='folder of <v_name>.npy motion features')
    p.add_argument('--appearance_feature_dir', type=str, default=None,
                   help='folder of <v_name>.npy appearance features (optional: one stream alone is accepted)')
    p.add_argument('--subset', type=str, default='test', choices=('test', 'train'), help='the split that is clustered')
    p.add_argument('--clusters', type=int, default=0, help='K (1..1024); 0 = the number of distinct labels in that split')
    p.add_argument('--iters', type=int, default=50, help='centroid updates per restart at most')
    p.add_argument('--restarts', type=int, default=3, help='restarts; the one of largest objective is reported')
    p.add_argument('--seed', type=int, default=0, help='restart r draws its initial rows from RandomState(seed + r)')
    p.add_argument('--columns', type=str, default='all', choices=('all', 'global'),
                   help='all = the whole vector; global = the last 512 columns of each stream (the x_global chunk)')
    return p


def select_columns(features, columns, streams):
    """`all`: the features as they are; `global`: the last 512 columns of each of the `streams` equal-width blocks -- in place
    (a strided view) for one stream, a copy of the blocks' tails for more."""
    if columns == 'all':
        return features
    n, W = features.shape
    if W % streams or (W // streams) < 512:
        raise RuntimeError("--columns global: %d columns are not %d streams of at least 512" % (W, streams))
    w = W // streams
    if streams == 1:
        return features[:, w - 512:]
    return torch.cat([features[:, (s + 1) * w - 512:(s + 1) * w] for s in range(streams)], dim=1)


def main(args=None):
    """Clusters one split; prints and returns dict(acc, nmi, ari, purity, objective, n_iter, restart, sizes)."""
    from .linear_classify import load_splits
    opt = build_parser().parse_args(args)
    print(opt)
    train, test = load_splits(opt)
    f, y = train if opt.subset == 'train' else test
    y = y.cpu().numpy()
    K = opt.clusters if opt.clusters else len(np.unique(y))
    x = select_columns(f, opt.columns, 2 if opt.appearance_feature_dir else 1)
    labels, _, info = fcl.kmeans(x, K, iters=opt.iters, restarts=opt.restarts, seed=opt.seed)
    res = fcl.scores(labels.cpu().numpy(), y)
    print('cluster acc:', res['acc'])
    print('nmi:', res['nmi'])
    print('ari:', res['ari'])
    print('purity:', res['purity'])
    print('objective: %.6f iters: %d restart: %d sizes min/max: %d/%d' % (info['objective'], info['n_iter'], info['restart'],
                                                                         int(info['sizes'].min()), int(info['sizes'].max())))
    res.update(objective=info['objective'], n_iter=info['n_iter'], restart=info['restart'], sizes=info['sizes'])
    return res


if __name__ == '__main__':
    main()
