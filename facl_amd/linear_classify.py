"""Linear-probe consumer of the extracted features -- counterpart of linear_classify/fc_model.py:12-25
(``Final_FC``: L2-normalise + Linear(512*22 -> 120), weight ~ N(0, 0.01), zero bias) and of the training loop of
linear_classify/linercls.py:100-150 (Adam + StepLR(5, 0.7), CrossEntropy, top-1).  The feature format is the one
``facl_amd.extract_common`` writes: per clip [x_view0 .. x_view9, x_global] (11*512) per stream, motion and
appearance concatenated (dataset_of_lin.py:103-105).  The single dense layer runs on the MFMA GEMM of csrc/gemm.hip."""
import argparse
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import tail as _tail
from .train_common import lr_for_epoch


class Final_FC(nn.Module):
    def __init__(self, input_dim=512, gost=11 + 11, num_class=120):
        super().__init__()
        self.fc = nn.Linear(input_dim * gost * 1, num_class)          # parameter holder: same state_dict keys (fc.weight, fc.bias)
        self.fc.weight.data.normal_(mean=0.0, std=0.01)
        self.fc.bias.data.zero_()

    def forward(self, x):
        x = F.normalize(x, p=2, dim=1)
        return _tail.linear(x, self.fc)


def accuracy(output, target, topk=(1,)):
    """linercls.py:158-172."""
    with torch.no_grad():
        maxk = max(topk)
        _, pred = output.topk(maxk, 1, True, True)
        correct = pred.t().eq(target.view(1, -1).expand(maxk, -1))
        return [correct[:k].reshape(-1).float().sum(0, keepdim=True).mul_(100.0 / target.size(0)) for k in topk]


def fit(features, labels, num_class=120, nepoch=20, batch=256, lr=1e-3, shuffle=None, on_epoch=None):
    """Train the probe on (n, 11264) float32 CUDA features; returns (model, last-epoch train top-1).  The layer is sized
    from the feature length (any multiple of 512), so features extracted at another --num_crop G -- (G+1)*512 per stream,
    e.g. 25*512 at G = 24 -- are accepted as they are.  `shuffle`: a
    np.random.RandomState -> every epoch runs over a fresh permutation in full batches only (the reference's loader,
    shuffle=True, drop_last=True); `on_epoch(epoch, model)` is called after every epoch."""
    netR = Final_FC(input_dim=512, gost=features.shape[1] // 512, num_class=num_class).to(features.device)
    optimizer = torch.optim.Adam(netR.parameters(), lr=lr, betas=(0.5, 0.999), eps=1e-06)
    criterion = nn.CrossEntropyLoss()
    top1 = 0.0
    for epoch in range(nepoch):
        for g in optimizer.param_groups:
            g["lr"] = lr_for_epoch(lr, epoch, 5, 0.7)                   # StepLR(5, 0.7) stepped with the epoch
        hit, seen = 0.0, 0
        if shuffle is None:
            chunks = [slice(i, i + batch) for i in range(0, features.shape[0], batch)]
        else:
            perm = torch.from_numpy(shuffle.permutation(features.shape[0])).to(features.device)
            chunks = [perm[i:i + batch] for i in range(0, features.shape[0] - batch + 1, batch)]
        for c in chunks:
            f, y = features[c], labels[c]
            out = netR(f)
            loss = criterion(out, y)
            optimizer.zero_grad()
            loss.backward()
            optimizer.step()
            hit += float(accuracy(out, y)[0]) * f.shape[0] / 100.0
            seen += f.shape[0]
        top1 = 100.0 * hit / max(seen, 1)
        if on_epoch is not None:
            on_epoch(epoch, netR)
    return netR, top1


def evaluate(netR, features, labels, batch=256):
    """Test top-1 (%) over every clip of the split."""
    netR.eval()
    hit = 0.0
    with torch.no_grad():
        for i in range(0, features.shape[0], batch):
            out = netR(features[i:i + batch])
            hit += float(accuracy(out, labels[i:i + batch])[0]) * out.shape[0] / 100.0
    netR.train()
    return 100.0 * hit / max(features.shape[0], 1)


def load_split(index, vids, motion_dir, appearance_dir=None):
    """dataset_of_lin.py:37-110 LIner_NTU: per clip motion || appearance features from <dir>/<v_name>.npy, label from the name.
    One stream alone (either directory None) gives that stream's features as they are."""
    dirs = [d for d in (motion_dir, appearance_dir) if d]
    if not dirs:
        raise ValueError("load_split needs a motion or an appearance feature directory")
    feats, labels = [], []
    for v in vids:
        n = index.v_name(v)
        feats.append(np.concatenate([np.load(os.path.join(d, n + '.npy')) for d in dirs], 0))
        labels.append(index.label(v))
    return np.stack(feats).astype(np.float32), np.asarray(labels, dtype=np.int64)


def load_splits(opt):
    """Makes --main_gpu the current device and returns, on it, ((train features, labels), (test features, labels)) of the
    clips listed in <data_root>/reslution/Resolution60/raw, read from the feature folders of `opt`."""
    from . import dataset as fds
    device = torch.device("cuda", opt.main_gpu)
    torch.cuda.set_device(device)
    index = fds.ClipIndex.from_dir(os.path.join(opt.data_root, fds.PROBE_LIST_DIR), opt.dataset)
    data = []
    for vids in (index.select(opt.split, full_train=bool(opt.full_train)), index.select(opt.split, test=True)):
        f, y = load_split(index, vids, opt.motion_feature_dir, opt.appearance_feature_dir)
        data.append((torch.from_numpy(f).to(device), torch.from_numpy(y).to(device)))
    return data


def main(args=None):
    """linercls.py:27-150: train the probe on the train split, print test top-1 after every epoch from 16 on."""
    from . import dataset as fds
    p = argparse.ArgumentParser(description="Linear probe")
    p.add_argument('--batchSize', type=int, default=64, help='input batch size')
    p.add_argument('--nepoch', type=int, default=50, help='number of epochs to train for')
    p.add_argument('--dataset', type=str, default='ntu120', help='ntu120 | ntu60')
    p.add_argument('--learning_rate', type=float, default=0.005, help='learning rate at t=0')
    p.add_argument('--main_gpu', type=int, default=0, help='main GPU id')
    p.add_argument('--num_class', type=int, default=120, help='NEW: outputs of the probe (literal 120 in fc_model.py)')
    p.add_argument('--data_root', type=str, default='../ntu/3DV_ntu60',
                   help='NEW: the dataset root; the clips listed are <data_root>/reslution/Resolution60/raw (linercls.py:40)')
    p.add_argument('--split', type=str, default='view', choices=fds.SPLIT_MODES, help='NEW: view | subject | set')
    p.add_argument('--full_train', type=int, default=1, help='NEW (--split subject): 0 = without the validation performers')
    p.add_argument('--motion_feature_dir', type=str, required=True, help='NEW: folder of <v_name>.npy motion features')
    p.add_argument('--appearance_feature_dir', type=str, required=True, help='NEW: folder of <v_name>.npy appearance features')
    p.add_argument('--save_fc', type=str, default='',
                   help="NEW: file the probe's state_dict is saved to after the last epoch (facl_amd.predict --head); '' = not saved")
    opt = p.parse_args(args)
    print(opt)
    (ftr, ytr), (fte, yte) = load_splits(opt)
    torch.manual_seed(1)
    if ftr.shape[0] < opt.batchSize:
        raise RuntimeError("the train split has %d clips: fewer than one batch of %d" % (ftr.shape[0], opt.batchSize))
    result = {}

    def on_epoch(epoch, netR):
        if epoch > 15:                                                  # linercls.py:137
            result["top1"] = evaluate(netR, fte, yte, opt.batchSize)
            print('epoch:', epoch, 'test top1:', result["top1"])

    netR, _ = fit(ftr, ytr, num_class=opt.num_class, nepoch=opt.nepoch, batch=opt.batchSize, lr=opt.learning_rate,
                  shuffle=np.random.RandomState(1), on_epoch=on_epoch)
    if opt.save_fc:
        torch.save(netR.state_dict(), opt.save_fc)
    return result.get("top1")


if __name__ == '__main__':
    main()
