"""Shared pieces of the data-parallel tests (test_ddp_host.py, test_gpu_ddp.py, ddp_worker.py): the generated footage
(the frames tests/test_gpu_data.py generates: 2 videos x 11 frames of 72 x 88), the smallest model the state-dict spec
builds, its optimiser, and the fixed batch of 8 x 12 LR frames decoded to 16 x 24 that every process regenerates from
the same seeds."""
import os

import numpy as np
import torch

FRONT, BACK = 1, 1                       # weights.make_state_dict(front_RBs=1, back_RBs=1): 270 of the 442 keys
KEYS = 442 - 4 * (4 + 39)
COVERED = 434 - 4 * (4 + 39)             # the eight keys of the unused upsampling layers never receive a gradient
TRAIN_OPT = dict(lr_G=1e-4, beta1=0.9, beta2=0.99, lr_scheme="MultiStepLR", lr_steps=[10], lr_gamma=0.5)
SHAPE = (16, 24)
STEPS = 2


def write_footage(root):
    """2 videos x 11 frames of 72 x 88, PNGs written with PIL, and the list file; returns ``root``."""
    from PIL import Image
    rng = np.random.RandomState(21)
    for v in ("clip_a", "clip_b"):
        os.makedirs(os.path.join(root, v))
        for k in range(11):
            Image.fromarray(rng.randint(0, 256, (72, 88, 3)).astype(np.uint8)).save(os.path.join(root, v, f"{k}.png"))
    with open(os.path.join(root, "list.txt"), "w") as f:
        f.write("clip_a\nclip_b\n")
    return root


def make_net(stif, device="cuda"):
    """(net, optimizer, criterion): train.LunaTokis(1, 1) on the seed-0 weights, Adam as the shipped options set it."""
    TR = stif.train
    sd = stif.weights.make_state_dict(seed=0, front_RBs=FRONT, back_RBs=BACK)
    net = TR.LunaTokis(FRONT, BACK)
    net.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in sd.items()}, strict=True)
    net = net.to(device)
    opt, _ = TR.make_optimizer(net, TRAIN_OPT)
    return net, opt, TR.TimesLoss(TR.CharbonnierLoss())


def global_batch(B, device="cuda"):
    """Item b of the batch is a function of b alone: LQs [B, 2, 3, 8, 12], two query times per item, GT
    [B, 2, 3, 16, 24]."""
    lq, gt, t = [], [], []
    for b in range(B):
        g = torch.Generator().manual_seed(1100 + b)
        lq.append(torch.rand(2, 3, 8, 12, generator=g))
        gt.append(torch.rand(2, 3, *SHAPE, generator=g))
        t.append(torch.tensor([0.25 + 0.125 * b, 0.75 - 0.125 * b]))
    t = torch.stack(t)
    return torch.stack(lq).to(device), [t[:, k:k + 1].clone() for k in range(2)], torch.stack(gt).to(device)


def rows(batch, a, b):
    """Items [a, b) of a global_batch as the (inputs, gt) pair of a step."""
    lq, times, gt = batch
    return (lq[a:b], [t[a:b] for t in times], SHAPE), gt[a:b]


def state_of(net, opt):
    """Parameters and Adam moments as CPU tensors, keyed for a bitwise comparison."""
    out = {"p/" + k: p.detach().cpu() for k, p in net.named_parameters()}
    for i, p in enumerate(opt.param_groups[0]["params"]):
        for name, v in opt.state.get(p, {}).items():
            if torch.is_tensor(v):
                out[f"o/{i}/{name}"] = v.detach().cpu()
    return out


def same_bytes(a, b):
    a, b = a.contiguous(), b.contiguous()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == torch.float32:
        return torch.equal(a.view(torch.int32), b.view(torch.int32))
    return torch.equal(a, b)
