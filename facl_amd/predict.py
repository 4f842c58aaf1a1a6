"""Apply a saved classifier: per-clip class probabilities, the k most probable classes, the rank of the label,
top-1 / top-k / mean class accuracy and the confusion matrix of a split -- from a fine-tuned encoder + head
(``facl_amd.finetune``'s finetune_enc_<e>.pth / finetune_fc_<e>.pth) reading the clips on disk, or from a probe head
(``facl_amd.linear_classify --save_fc``) reading extracted feature folders.

    python -m facl_amd.predict --data_root D --dataset ntu60 --encoder ft/finetune_enc_95.pth --head ft/finetune_fc_95.pth \\
        --num_crop 24 --SAMPLE_NUM 2048 --view_rng philox [--subset test|train|all] [--topk 5] [--draws 1] [--out DIR] [--no_labels]
    python -m facl_amd.predict --data_root D --dataset ntu60 --motion_feature_dir feats/motion/ \\
        [--appearance_feature_dir feats/app/] --head probe_fc.pth [...]

The probabilities are the fp64 softmax of the head's logits, averaged over --draws draws of the views (csrc/predict.hip);
they, the top-k lists and the ranks stay on the device until the split is done.  Everything runs on eager launches."""
import io
import os
import zipfile

import numpy as np
import torch

from . import _lib
from . import cls_head
from . import dist as fdist
from .train_flags import build_parser, check_view_flags, view_recipe
from .train_step import group_views

MAX_TOPK = 64              # facl_cls_topk: one list entry per lane


# ---- host side: pure numpy ------------------------------------------------------------------------------------------------------
def confusion(labels, pred, ncls):
    """(int64 (ncls, ncls) matrix with rows = true class and columns = predicted class, clips skipped).  A clip whose label
    or prediction lies outside [0, ncls) (a NaN row predicts -1) is in no cell and counts as skipped."""
    labels, pred = np.asarray(labels).reshape(-1).astype(np.int64), np.asarray(pred).reshape(-1).astype(np.int64)
    if labels.shape != pred.shape:
        raise ValueError("labels and pred differ in length (%d, %d)" % (len(labels), len(pred)))
    ok = (labels >= 0) & (labels < ncls) & (pred >= 0) & (pred < ncls)
    m = np.zeros((ncls, ncls), dtype=np.int64)
    np.add.at(m, (labels[ok], pred[ok]), 1)
    return m, int((~ok).sum())


def metrics(rank, labels, ncls, k):
    """Accuracies (%) from facl_cls_topk's ranks: ``top1`` (rank == 0), ``topk`` (rank < k), ``per_class`` (float64 (ncls,),
    top-1 of the clips of each true class, NaN for a class that does not occur) and ``mean_class`` (the mean of per_class over
    the classes that occur).  A NaN row (rank -1) is a miss.  A clip whose label lies outside [0, ncls) (rank -2) belongs to no
    class: it is left out of every figure and counted in ``skipped``; ``clips`` is the number that remain."""
    rank, labels = np.asarray(rank).reshape(-1).astype(np.int64), np.asarray(labels).reshape(-1).astype(np.int64)
    if rank.shape != labels.shape:
        raise ValueError("rank and labels differ in length (%d, %d)" % (len(rank), len(labels)))
    ok = (labels >= 0) & (labels < ncls) & (rank != -2)
    rank, labels = rank[ok], labels[ok]
    n = len(rank)
    hit1, hitk = rank == 0, (rank >= 0) & (rank < k)
    per_class = np.full(ncls, np.nan)
    count = np.bincount(labels, minlength=ncls)
    hits = np.bincount(labels[hit1], minlength=ncls)
    occurs = count > 0
    per_class[occurs] = 100.0 * hits[occurs] / count[occurs]
    return {"top1": 100.0 * int(hit1.sum()) / n if n else float("nan"),
            "topk": 100.0 * int(hitk.sum()) / n if n else float("nan"),
            "per_class": per_class, "mean_class": float(per_class[occurs].mean()) if n else float("nan"),
            "clips": n, "skipped": int((~ok).sum())}


def save_npz(path, **arrays):
    """np.savez with a fixed member time stamp: the same arrays give the same bytes whenever they are written."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED) as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue())


# ---- sources: the batches of one split, once per draw ---------------------------------------------------------------------------
class ViewSource:
    """The clips `split` of `index` as `facl_amd.finetune.evaluate` reads them.  ``batches(r)`` yields ((G*B, N, 4) views, B) of
    draw r in split order: draw 0 is evaluate's own pass (RandomState(2000), or philox keyed by (2000, 0, index)); philox
    draw r is keyed by epoch r, a NumPy draw r continues the same RandomState, so the draws must be asked for in order."""

    def __init__(self, opt, device, index, split):
        self.opt, self.device, self.index, self.split = opt, device, index, list(split)
        self.n = len(self.split)
        self.names = [index.v_name(int(v)) for v in self.split]
        self.labels = np.asarray([index.label(int(v)) for v in self.split], dtype=np.int64)
        self.rng = np.random.RandomState(2000)

    def batches(self, r):
        from .extract_common import ordered_views
        for views, names, _ in ordered_views(self.opt, self.device, self.index, self.split, self.rng, epoch=r):
            yield views, len(names)


class FeatureSource:
    """Extracted feature vectors (n, W) on the device, in batches of `batch`; one draw only."""

    def __init__(self, feats, labels, names, batch):
        self.feats, self.names, self.batch = feats, list(names), int(batch)
        self.n = feats.shape[0]
        self.labels = np.asarray(labels, dtype=np.int64)

    def batches(self, r):
        if r:
            raise RuntimeError("extracted features hold one draw of the views: draw %d does not exist" % r)
        for i in range(0, self.n, self.batch):
            f = self.feats[i:i + self.batch]
            yield f, f.shape[0]


# ---- the classifier -----------------------------------------------------------------------------------------------------------
class Classifier:
    """A head (state_dict with fc.weight (num_class, W), fc.bias) and, for clips, the encoder in front of it.  With an encoder
    state_dict the head is a ``ClipClassifier`` reading the encoder's stacked output and W = (num_crop + 1) * 512; without one
    it is the probe's ``Final_FC`` on feature vectors of length W.  Construction is host-only; ``to(device)`` moves both and
    puts them into eval()."""

    @staticmethod
    def head_shape(head_sd):
        """(num_class, W) of a head's state_dict."""
        if "fc.weight" not in head_sd or head_sd["fc.weight"].dim() != 2:
            raise RuntimeError("the head is no state_dict of Final_FC / ClipClassifier: it has no 2-D fc.weight (keys %s)"
                               % sorted(head_sd)[:8])
        num_class, width = (int(v) for v in head_sd["fc.weight"].shape)
        if width % cls_head.FEATURE_DIM or width < 2 * cls_head.FEATURE_DIM:
            raise RuntimeError("the head reads vectors of %d floats, which is not (views + 1) * %d" % (width, cls_head.FEATURE_DIM))
        return num_class, width

    def __init__(self, head_sd, opt=None, encoder_sd=None):
        self.num_class, self.width = self.head_shape(head_sd)
        self.views = self.width // cls_head.FEATURE_DIM - 1              # of ONE stream; a two-stream probe head has no encoder
        self.opt, self.device = opt, None
        if encoder_sd is not None:
            from . import cn3d_model_conbag as MM
            if self.views != opt.num_crop:
                raise RuntimeError("the head was built for --num_crop %d (fc.weight is %d x %d), the views asked for are "
                                   "--num_crop %d" % (self.views, self.num_class, self.width, opt.num_crop))
            self.encoder = MM.PointNet_Plus(opt, gost=opt.num_crop)
            self.encoder.load_state_dict(encoder_sd)
            self.encoder.precision = getattr(opt, "precision", "f32")
            self.head = cls_head.ClipClassifier(opt.num_crop, self.num_class)
        else:
            from .linear_classify import Final_FC
            self.encoder = None
            self.head = Final_FC(input_dim=cls_head.FEATURE_DIM, gost=self.width // cls_head.FEATURE_DIM, num_class=self.num_class)
        self.head.load_state_dict(head_sd)

    def to(self, device):
        self.device = torch.device(device)
        if self.encoder is not None:
            self.encoder = self.encoder.to(self.device).eval()
        self.head = self.head.to(self.device).eval()
        return self

    def logits_of_views(self, views, B):
        """(G*B, N, 4) view-major views of B clips -> (B, num_class) logits: group, encoder forward, head."""
        if self.encoder is None:
            raise RuntimeError("this classifier has no encoder: it reads extracted features (logits_of_features)")
        with torch.no_grad():
            xt, yt = group_views(views if views.dtype == torch.float32 else views.float(), self.opt, self.opt.group_radius)
            self.encoder(xt, yt, 1)
            return self.head(self.encoder._stacked, self.views, B)

    def logits_of_features(self, feats):
        """(B, W) extracted feature vectors -> (B, num_class) logits of the probe head."""
        if self.encoder is not None:
            raise RuntimeError("this classifier reads clips through its encoder (logits_of_views)")
        if feats.dim() != 2 or feats.shape[1] != self.width:
            raise RuntimeError("the head reads vectors of %d floats, the features have %s" % (self.width, tuple(feats.shape)))
        with torch.no_grad():
            return self.head(feats)

    def predict(self, source, draws=1, k=5, labels=True):
        """The split of `source` (``n``, ``labels``, ``batches(r)``) -> {"top_p" (n, k) float32, "top_c" (n, k) int32, "rank"
        (n,) int32 or None}: numpy arrays in split order.  The fp64 sums of the probabilities over the draws, the lists and
        the ranks live on the device; they are copied back once, after the last draw."""
        draws, k = int(draws), int(k)
        if draws < 1:
            raise RuntimeError("draws must be >= 1 (got %d)" % draws)
        if not 1 <= k <= min(self.num_class, MAX_TOPK):
            raise RuntimeError("k must be in 1..%d (got %d)" % (min(self.num_class, MAX_TOPK), k))
        n, dev = source.n, self.device
        if n < 1:
            raise RuntimeError("the split has no clips")
        y = torch.as_tensor(np.asarray(source.labels), dtype=torch.int32).to(dev) if labels else None
        acc = _lib.empty((n, self.num_class), dtype=torch.float64, device=dev)
        for r in range(draws):
            i = 0
            for batch, B in source.batches(r):
                lg = self.logits_of_views(batch, B) if self.encoder is not None else self.logits_of_features(batch)
                cls_head.probs_acc(lg, acc[i:i + B], first=(r == 0))
                i += B
            if i != n:
                raise RuntimeError("draw %d gave %d clips, the split has %d" % (r, i, n))
        top_p, top_c, rank = cls_head.topk(acc, draws, k, y)
        return {"top_p": top_p.cpu().numpy(), "top_c": top_c.cpu().numpy(), "rank": None if rank is None else rank.cpu().numpy()}


# ---- the entry ------------------------------------------------------------------------------------------------------------------
def predict_parser():
    p = build_parser('0')
    p.description = "Prediction with a saved classifier"
    p.add_argument('--encoder', type=str, default='', help='NEW: encoder state_dict (finetune_enc_<e>.pth); reads the clips of --data_root')
    p.add_argument('--head', type=str, default='', help='NEW: head state_dict (finetune_fc_<e>.pth, or linear_classify --save_fc)')
    p.add_argument('--motion_feature_dir', type=str, default='', help='NEW: folder of <v_name>.npy motion features (probe path)')
    p.add_argument('--appearance_feature_dir', type=str, default='', help='NEW: folder of <v_name>.npy appearance features (probe path)')
    p.add_argument('--subset', type=str, default='test', choices=('test', 'train', 'all'), help='NEW: the clips predicted; all = train, then test')
    p.add_argument('--topk', type=int, default=5, help='NEW: classes listed per clip, 1..min(num_class, 64)')
    p.add_argument('--draws', type=int, default=1, help='NEW: test-time draws of the views the probabilities are averaged over')
    p.add_argument('--out', type=str, default='', help='NEW: folder for predictions.npz and confusion.npy')
    p.add_argument('--no_labels', action='store_true', help='NEW: no labels, metrics or confusion matrix')
    return p


def check_predict_flags(opt, world=None):
    """Raises before the device is touched (`world` None: the launcher's WORLD_SIZE)."""
    world = fdist.env_world_size() if world is None else world
    if world > 1:
        raise RuntimeError("prediction runs on one rank only (got %d ranks)" % world)
    if opt.draws < 1:
        raise RuntimeError("--draws must be >= 1 (got %d)" % opt.draws)
    folders = bool(opt.motion_feature_dir or opt.appearance_feature_dir)
    if bool(opt.encoder) == folders:
        raise RuntimeError("give either --encoder (clips on disk) or --motion_feature_dir / --appearance_feature_dir (extracted "
                           "features): got %s" % ("both" if folders else "neither"))
    if not opt.head:
        raise RuntimeError("--head is required: the state_dict of the classifier head")
    if folders and opt.draws > 1:
        raise RuntimeError("--draws %d needs --encoder: feature folders hold one draw of the views" % opt.draws)
    if opt.topk < 1 or opt.topk > MAX_TOPK:
        raise RuntimeError("--topk must be in 1..min(num_class, %d) (got %d)" % (MAX_TOPK, opt.topk))
    if opt.encoder:
        opt.synthetic = 0
        check_view_flags(opt)
        print(view_recipe(opt).describe())


def _subset(index, opt):
    train, test = index.select(opt.split, full_train=bool(opt.full_train)), index.select(opt.split, test=True)
    return {"test": test, "train": train, "all": list(train) + list(test)}[opt.subset]


def main(args=None):
    """Returns {"top1", "topk", "mean_class_accuracy", "k", "clips"} (%), or {"clips"} with --no_labels."""
    from . import dataset as fds
    from .finetune import _raise_bad_labels
    opt = predict_parser().parse_args(args)
    print(opt)
    check_predict_flags(opt)
    head_sd = torch.load(opt.head, map_location="cpu", weights_only=True)
    num_class = Classifier.head_shape(head_sd)[0]
    if opt.topk > num_class:
        raise RuntimeError("--topk must be in 1..min(num_class, %d) = 1..%d (got %d)" % (MAX_TOPK, min(num_class, MAX_TOPK), opt.topk))
    enc_sd = torch.load(opt.encoder, map_location="cpu", weights_only=True) if opt.encoder else None
    clf = Classifier(head_sd, opt, enc_sd)
    list_dir = fds.EXTRACT_LIST_DIR if opt.encoder else fds.PROBE_LIST_DIR
    index = fds.ClipIndex.from_dir(os.path.join(opt.data_root, list_dir), opt.dataset)
    split = _subset(index, opt)
    if not len(split):
        raise RuntimeError("--subset %s of %s has no clips" % (opt.subset, opt.data_root))
    labels = np.asarray([index.label(int(v)) for v in split], dtype=np.int64)
    if not opt.no_labels:
        bad = int(((labels < 0) | (labels >= clf.num_class)).sum())
        if bad:
            _raise_bad_labels(bad, clf.num_class, "the %s split" % opt.subset)

    device = torch.device("cuda", opt.main_gpu)
    torch.cuda.set_device(device)
    clf.to(device)
    if opt.encoder:
        source = ViewSource(opt, device, index, split)
    else:
        from .linear_classify import load_splits
        (ftr, _), (fte, _) = load_splits(opt)
        feats = {"test": fte, "train": ftr}[opt.subset] if opt.subset != "all" else torch.cat((ftr, fte))
        if feats.shape[1] != clf.width:
            raise RuntimeError("the head reads vectors of %d floats, the feature folders give %d" % (clf.width, feats.shape[1]))
        source = FeatureSource(feats, labels, [index.v_name(int(v)) for v in split], opt.batchSize)
    res = clf.predict(source, opt.draws, opt.topk, labels=not opt.no_labels)

    out = {"clips": len(split)}
    arrays = {"names": np.asarray(source.names), "top_c": res["top_c"], "top_p": res["top_p"]}
    if not opt.no_labels:
        m = metrics(res["rank"], labels, clf.num_class, opt.topk)
        out.update(top1=m["top1"], topk=m["topk"], mean_class_accuracy=m["mean_class"], k=opt.topk)
        print('top1:', m["top1"])
        if opt.topk > 1:
            print('top%d:' % opt.topk, m["topk"])
        print('mean class accuracy:', m["mean_class"])
        arrays.update(labels=labels, rank=res["rank"])
    if opt.out:
        os.makedirs(opt.out, exist_ok=True)
        save_npz(os.path.join(opt.out, "predictions.npz"), **arrays)
        if not opt.no_labels:
            np.save(os.path.join(opt.out, "confusion.npy"), confusion(labels, res["top_c"][:, 0], clf.num_class)[0])
    return out


if __name__ == '__main__':
    main()
