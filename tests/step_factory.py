"""The model, optimizer and training step of the GPU tests, built in one place: the option namespace the host layer reads,
PointNet_Plus on the formula weights, FusedAdam as the training entries configure it, ContrastiveStep / FineTuneStep, and
the seeded point clouds.  Callers keep their own case dictionaries (B, G, N, D and, where they have it, view_major) and
tolerances.  Tests compare bit for bit against twins and recorded trajectories built from these: the namespace's attributes,
the seeds and the order of the RNG draws are part of the contract."""
from types import SimpleNamespace

import numpy as np
import torch

DEV = "cuda:0"
S = K = 64                                                    # sample_num_level1 / knn_K of every test configuration
ADAM = dict(betas=(0.5, 0.999), eps=1e-6)


def step_opt(D, B, N=512, **flags):
    return SimpleNamespace(temperal_num=3, knn_K=64, ball_radius=0.16, ball_radius2=0.25, sample_num_level1=64,
                           sample_num_level2=64, INPUT_FEATURE_NUM=D, Num_Class=512, batchSize=B,
                           pooling="concatenation", SAMPLE_NUM=N, **flags)


def make_net(D, G, B=4, N=512, neg_gamma=False, opt=None, device=DEV):
    """PointNet_Plus with the formula weights, on `device`, as constructed (training mode)."""
    from facl_amd.cn3d_model_conbag import PointNet_Plus
    from oracle.weights import formula_state_dict
    net = PointNet_Plus(opt or step_opt(D, B, N), gost=G)
    net.load_state_dict({k: torch.as_tensor(v) for k, v in formula_state_dict(D, neg_gamma=neg_gamma).items()})
    return net.to(device)


def make_contrastive_step(c, lr=3e-4, adam=None, **flags):
    """(net, optim, step): the formula model in train() mode, FusedAdam with the entries' betas and eps (`adam`: further
    FusedAdam arguments), ContrastiveStep on the namespace with `flags`."""
    from facl_amd.optim import FusedAdam
    from facl_amd.train_common import ContrastiveStep
    opt = step_opt(c["D"], c["B"], c["N"], **flags)
    net = make_net(c["D"], c["G"], opt=opt).train()
    optim = FusedAdam(net.parameters(), lr=lr, **ADAM, **(adam or {}))
    return net, optim, ContrastiveStep(net, optim, opt, c["G"])


def make_finetune_step(c, ncls, lr=3e-4):
    """(net, optim, step): FineTuneNet with the formula encoder weights and a head drawn from a fixed seed + FusedAdam +
    FineTuneStep."""
    from facl_amd.finetune import FineTuneNet, FineTuneStep
    from facl_amd.optim import FusedAdam
    from oracle.weights import formula_state_dict
    opt = step_opt(c["D"], c["B"], c["N"])
    torch.manual_seed(5)
    net = FineTuneNet(opt, ncls, gost=c["G"])
    net.load_encoder_state_dict({k: torch.as_tensor(v) for k, v in formula_state_dict(c["D"]).items()})
    with torch.no_grad():                                # logits of order one (a head some way into its training), so that the
        net.head.fc.weight.mul_(50.0)                    # loss depends visibly on the labels; a non-zero bias, so that its
        net.head.fc.bias.normal_(0.0, 0.5)               # update is checked against values
    net = net.to(DEV).train()
    optim = FusedAdam(net.parameters(), lr=lr, **ADAM)
    return net, optim, FineTuneStep(net, optim, opt, c["G"])


def points(c, seed, scale=1.0):
    """Uniform clouds in [-0.5, 0.5) * scale from a device generator: (B, G, N, D), or view-major (G*B, N, D) rows where the
    case says view_major."""
    B, G, N, D = c["B"], c["G"], c["N"], c["D"]
    gen = torch.Generator(device=DEV)
    gen.manual_seed(seed)
    shape = (G * B, N, D) if c.get("view_major") else (B, G, N, D)
    return (torch.rand(shape, device=DEV, generator=gen) - 0.5) * scale


def class_labels(c, seed, ncls):
    return torch.from_numpy(np.random.RandomState(seed).randint(0, ncls, c["B"]).astype(np.int32)).to(DEV)


def grouped(c, pts):
    """Grouped rows (P,D) and centres (M*S,3) of `pts` through the grouping the step itself uses (bit-exact to the
    reference: test_gpu_grouping.py), from the view-major rows."""
    from facl_amd.utils_my import group_points_3DV, knn_radius_group
    N, D = c["N"], c["D"]
    vm = pts if c.get("view_major") else pts.permute(1, 0, 2, 3).reshape(-1, N, D)
    if N == 512:
        xt, yt = group_points_3DV(vm.contiguous(), step_opt(D, c["B"], N))
    else:
        xt, yt = knn_radius_group(vm.contiguous(), S, K, 0.16)
    return xt.permute(0, 2, 3, 1).reshape(-1, D), yt.permute(0, 2, 1, 3).reshape(-1, 3)


def dp_step(clip, G, rank, world):
    """Two ContrastiveStep calls with lr = 0 on the (local) `clip`, SyncBN hooks on: (loss, gradients, running buffers)."""
    from facl_amd import dist as fdist
    from facl_amd.train_common import ContrastiveStep
    B, _, N, D = clip.shape
    opt = step_opt(D, B, N)
    net = make_net(D, G, opt=opt, device="cuda").train()    # the rank's current device
    net.bn_reduce_fn = fdist.make_bn_reduce_fn()
    optim = torch.optim.SGD(net.parameters(), lr=0.0)            # keep the parameters: we compare gradients
    step = ContrastiveStep(net, optim, opt, G)
    # two steps (lr = 0): the first gradient sync is synchronous and learns the buckets, the second one overlaps the
    # tail bucket's all-reduce with the set-abstraction backward (facl_amd/dist.py: GradSync)
    step(clip.cuda(), epoch=0, order=np.array([2, 0, 3, 1]))
    loss, _, _ = step(clip.cuda(), epoch=0, order=np.array([2, 0, 3, 1]))
    grads = {k: p.grad.detach().cpu().clone() for k, p in net.named_parameters() if p.grad is not None}
    bufs = {k: v.detach().cpu().clone() for k, v in net.state_dict().items() if "running" in k}
    return float(loss.item()), grads, bufs
