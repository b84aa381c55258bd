"""Training-side pieces of the reference's VideoSRBaseModel (training only):
the Charbonnier pixel loss and the two learning-rate schedules its option files select, as drop-ins with
the reference's names, arguments and step semantics.

* ``CharbonnierLoss`` -- loss.py:7-17: sum(sqrt((x - y)^2 + eps)).
* ``CosineAnnealingLR_Restart`` -- lr_scheduler.py:34-64, selected by ``lr_scheme: CosineAnnealingLR_Restart``
  (VideoSR_base_model.py:77-82; train_zsm.yml:57-65): cosine annealing from the group's lr to ``eta_min``
  over ``T_period[k]`` steps, restarted at ``restarts[k]`` to ``initial_lr * weights[k]``.
* ``MultiStepLR_Restart`` -- lr_scheduler.py:8-31 (``lr_scheme: MultiStepLR``, VideoSR_base_model.py:70-76):
  lr x gamma^(multiplicity) at each milestone, restarts as above, optionally clearing the optimizer state.

Both schedules are recurrences on the group's current lr (each step scales the previous lr), exactly as the
reference evaluates them, so a resumed optimizer continues the same sequence; ``tests/test_train.py`` checks
them step for step against sequences recorded from the reference's own classes (tests/golden/make_golden.py
sched).  ``optimize_step`` is VideoSRBaseModel.optimize_parameters (VideoSR_base_model.py:113-134) for a
module and one target.  The whole-model HIP forward (``LunaTokis``) is inference-only.  Two of the model's
operators train on the engine's own kernels: the DCN_sep layers of a torch module through the ``_ext`` drop-in
(integration/_ext.py: stif_dcn_v2_forward / _backward), and the 3x3 / 64 -> 64 convolutions of the residual
trunks through the modules below.

* ``Conv3x3``, ``ResidualBlock_noBN``, ``make_trunk`` -- module_util.py:34-52 with ``nn.Conv2d``'s parameter
  names and shapes (reference checkpoints load), forward and backward on the HIP kernels: the forward and the
  data gradient are stif_conv3x3_wino (the data gradient with the transposed, rotated weight), the weight /
  bias gradient is stif_conv3x3_wgrad, and the weights are re-packed on the device every step
  (stif_pack_conv_weight_dev).  ``mfma="f16x3"`` runs the two Winograd convs on split-fp16 operands; the weight
  gradient always uses exact fp32 products.  The f16x3 operand range is reported through one device status word
  per device: ``module.range_status()`` reads and clears it (one sync).  A step that ends with a non-zero
  status used an operand outside the split range somewhere and must be redone with ``mfma="f32"``.
* ``ConvDown``, ``ConvFirst``, ``FrameFeatures`` -- the per-frame encoder (Sakuya_arch_test.py:282-287, :318-325)
  with the reference's parameter names: the stride-2 pyramid convs (forward stif_conv2d_nhwc with the weight packed
  on the device, backward stif_conv3x3s2_wgrad / stif_conv3x3s2_dgrad) and conv_first (stif_conv_first, backward
  stif_conv_first_wgrad), all fp32, around the trunk and two ``Conv3x3``.  The gradient with respect to the input
  frames is not built.
"""
from __future__ import annotations

import math
from collections import Counter, defaultdict

import torch
from torch import nn
from torch.optim.lr_scheduler import LRScheduler

from . import _lib as L
from . import ops


class CharbonnierLoss(nn.Module):
    """loss.py:7-17 (``pixel_criterion: cb``)"""

    def __init__(self, eps: float = 1e-6):
        super().__init__()
        self.eps = eps

    def forward(self, x, y):
        d = x - y
        return torch.sum(torch.sqrt(d * d + self.eps))


def _restart_lists(restarts, weights):
    r = list(restarts) if restarts else [0]
    w = list(weights) if weights else [1]
    if len(r) != len(w):
        raise ValueError("restarts and their weights do not match")
    return r, w


class CosineAnnealingLR_Restart(LRScheduler):
    """lr_scheduler.py:34-64.  Step e of the current period (k = e - last restart, period T):
    lr_e = eta_min + (lr_{e-1} - eta_min) * (1 + cos(pi k / T)) / (1 + cos(pi (k - 1) / T)); at a restart
    lr = initial_lr * weight and T becomes the next T_period entry; at k = T + 1 (mod 2T) the ratio's
    denominator vanishes and the schedule adds (base_lr - eta_min) (1 - cos(pi / T)) / 2 instead."""

    def __init__(self, optimizer, T_period, restarts=None, weights=None, eta_min=0, last_epoch=-1):
        self.T_period = list(T_period)
        self.T_max = self.T_period[0]
        self.eta_min = eta_min
        self.restarts, self.restart_weights = _restart_lists(restarts, weights)
        self.last_restart = 0
        super().__init__(optimizer, last_epoch)

    def get_lr(self):
        e, groups, eta = self.last_epoch, self.optimizer.param_groups, self.eta_min
        if e == 0:
            return list(self.base_lrs)
        if e in self.restarts:
            i = self.restarts.index(e)
            self.last_restart, self.T_max = e, self.T_period[i + 1]
            return [g["initial_lr"] * self.restart_weights[i] for g in groups]
        T, k = self.T_max, e - self.last_restart
        if (k - 1 - T) % (2 * T) == 0:
            return [g["lr"] + (b - eta) * (1 - math.cos(math.pi / T)) / 2 for b, g in zip(self.base_lrs, groups)]
        ratio = (1 + math.cos(math.pi * k / T)) / (1 + math.cos(math.pi * (k - 1) / T))
        return [ratio * (g["lr"] - eta) + eta for g in groups]


class MultiStepLR_Restart(LRScheduler):
    """lr_scheduler.py:8-31: at step e, a restart sets lr = initial_lr * weight (and, with ``clear_state``,
    drops the optimizer's moments); otherwise lr *= gamma ** (how often e appears in ``milestones``)."""

    def __init__(self, optimizer, milestones, restarts=None, weights=None, gamma=0.1, clear_state=False,
                 last_epoch=-1):
        self.milestones = Counter(milestones)
        self.gamma = gamma
        self.clear_state = clear_state
        self.restarts, self.restart_weights = _restart_lists(restarts, weights)
        super().__init__(optimizer, last_epoch)

    def get_lr(self):
        e, groups = self.last_epoch, self.optimizer.param_groups
        if e in self.restarts:
            if self.clear_state:
                self.optimizer.state = defaultdict(dict)
            w = self.restart_weights[self.restarts.index(e)]
            return [g["initial_lr"] * w for g in groups]
        n = self.milestones.get(e, 0)
        if n == 0:
            return [g["lr"] for g in groups]
        return [g["lr"] * self.gamma ** n for g in groups]


def make_optimizer(net: nn.Module, train_opt: dict):
    """VideoSR_base_model.py:56-83: Adam over the trainable parameters and the configured schedule."""
    wd = train_opt.get("weight_decay_G") or 0
    opt = torch.optim.Adam([p for p in net.parameters() if p.requires_grad], lr=train_opt["lr_G"],
                           weight_decay=wd, betas=(train_opt["beta1"], train_opt["beta2"]))
    scheme = train_opt["lr_scheme"]
    if scheme == "CosineAnnealingLR_Restart":
        sched = CosineAnnealingLR_Restart(opt, train_opt["T_period"], eta_min=train_opt["eta_min"],
                                          restarts=train_opt.get("restarts"), weights=train_opt.get("restart_weights"))
    elif scheme == "MultiStepLR":
        sched = MultiStepLR_Restart(opt, train_opt["lr_steps"], restarts=train_opt.get("restarts"),
                                    weights=train_opt.get("restart_weights"), gamma=train_opt["lr_gamma"],
                                    clear_state=train_opt.get("clear_state", False))
    else:
        raise NotImplementedError(f"lr_scheme {scheme!r}")
    return opt, sched


def update_learning_rate(schedulers, optimizers, cur_iter: int, warmup_iter: int = -1):
    """base_model.py:51-63: step every schedule, then during warm-up (cur_iter < warmup_iter) override each
    group's lr with initial_lr / warmup_iter * cur_iter."""
    for sch in schedulers:
        sch.step()
    if cur_iter < warmup_iter:
        for opt in optimizers:
            for g in opt.param_groups:
                g["lr"] = g["initial_lr"] / warmup_iter * cur_iter


def optimize_step(net: nn.Module, opt, criterion, inputs, gt, weight: float = 1.0) -> float:
    """VideoSR_base_model.py:113-134 for one output: zero_grad, forward, weight * criterion, backward,
    optimizer step; returns the loss (the caller steps the schedule, as train.py does per iteration)."""
    opt.zero_grad()
    loss = weight * criterion(net(*inputs), gt)
    loss.backward()
    opt.step()
    return float(loss.detach())


# ---- the residual trunks' 3x3 convolutions, trainable on the HIP kernels ----

_EPI = {None: L.EPI_NONE, "relu": L.EPI_RELU, "lrelu": L.EPI_LRELU}
_PACK = {"f16x3": L.PACK_WINO | L.PACK_F16X3, "f32": L.PACK_WINO}
_STATUS = {}   # device index -> the int32 status word every module on that device shares


def _status_word(device) -> torch.Tensor:
    idx = device.index if device.index is not None else torch.cuda.current_device()
    s = _STATUS.get(idx)
    if s is None:
        s = _STATUS[idx] = torch.zeros(1, dtype=torch.int32, device=torch.device("cuda", idx))
    return s


def range_status(device=None) -> int:
    """Read and clear the f16x3 range status of ``device`` (default: the current one); one synchronisation.
    Bit 0: a Winograd conv (forward or data gradient) produced a non-finite value -- an activation or gradient
    outside the split-fp16 range; ``STATUS_PACK_RANGE`` (16): a weight outside it (the convs store a plain 1, so a
    later conv's report may replace the packer's bit: test for non-zero).  Non-zero: redo the step with
    ``mfma="f32"``."""
    s = _status_word(torch.device("cuda") if device is None else torch.device(device))
    bits = int(s.item())
    s.zero_()
    return bits


def _nhwc(t: torch.Tensor, what: str) -> torch.Tensor:
    """The NHWC buffer of a logical NCHW tensor: a ``channels_last`` tensor is used in place (its memory is
    NHWC), anything else is converted once."""
    if not t.is_cuda:
        raise RuntimeError(f"{what}: the HIP convolution kernels need a CUDA tensor, got one on {t.device} "
                           "(move the module and its input to the GPU)")
    if t.dtype != torch.float32 or t.dim() != 4 or t.shape[1] != 64:
        raise RuntimeError(f"{what}: expected a float32 [n, 64, H, W] tensor, got {t.dtype} {tuple(t.shape)}")
    v = t.detach().permute(0, 2, 3, 1)
    return v if v.is_contiguous() else v.contiguous()


def _wino(x, weight, bias, mode, epi=L.EPI_NONE, res=None, dgrad=False):
    """stif_conv3x3_wino of NHWC ``x`` with ``weight`` packed on the device for this call (``dgrad``: the data
    gradient's packing, so ``x`` is a grad_output and the result a grad_input); returns a new NHWC tensor."""
    status = _status_word(x.device)
    lay = ops.pack_conv_dev(weight, bias, mode, dgrad=dgrad, status=status)
    out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    ops.conv2d([dict(layer=lay, in0=x, out=out, res=res)], epi=epi, status=status)
    return out


class _Conv3x3Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, act, mode):
        xh = _nhwc(x, "Conv3x3")
        out = _wino(xh, weight, bias, mode, _EPI[act])
        ctx.act, ctx.mode = act, mode
        ctx.save_for_backward(xh, weight, out if act else None)
        return out.permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, grad_out):
        xh, weight, out = ctx.saved_tensors
        g = _nhwc(grad_out, "Conv3x3 backward")
        # the activation's derivative from its output: both activations keep the sign of their argument
        if ctx.act == "relu":
            g = g * (out > 0)
        elif ctx.act == "lrelu":
            g = torch.where(out > 0, g, g * 0.1)
        need_x, need_w, need_b = ctx.needs_input_grad[:3]
        gx = gw = gb = None
        if need_w or need_b:
            gw, gb = ops.conv3x3_wgrad(xh, g)
        if need_x:
            gx = _wino(g, weight, None, ctx.mode, dgrad=True).permute(0, 3, 1, 2)
        return gx, gw if need_w else None, gb if need_b else None, None, None


class _ResBlockFn(torch.autograd.Function):
    """identity + conv2(relu(conv1(x))) as one node: the residual rides in conv2's epilogue, and the identity
    path's gradient in the epilogue of conv1's data gradient."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, mode):
        xh = _nhwc(x, "ResidualBlock_noBN")
        t = _wino(xh, w1, b1, mode, L.EPI_RELU)
        out = _wino(t, w2, b2, mode, L.EPI_RES, res=xh)
        ctx.mode = mode
        ctx.save_for_backward(xh, t, w1, w2)
        return out.permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, grad_out):
        xh, t, w1, w2 = ctx.saved_tensors
        g = _nhwc(grad_out, "ResidualBlock_noBN backward")
        need_x, need_w1, need_b1, need_w2, need_b2 = ctx.needs_input_grad[:5]
        gx = gw1 = gb1 = gw2 = gb2 = None
        if need_w2 or need_b2:
            gw2, gb2 = ops.conv3x3_wgrad(t, g)
        if need_x or need_w1 or need_b1:
            gt = _wino(g, w2, None, ctx.mode, dgrad=True) * (t > 0)
            if need_w1 or need_b1:
                gw1, gb1 = ops.conv3x3_wgrad(xh, gt)
            if need_x:
                gx = _wino(gt, w1, None, ctx.mode, L.EPI_RES, res=g, dgrad=True).permute(0, 3, 1, 2)
        return (gx, gw1 if need_w1 else None, gb1 if need_b1 else None, gw2 if need_w2 else None,
                gb2 if need_b2 else None, None)


def _check_choice(nf, act, mfma):
    if nf != 64:
        raise ValueError(f"the HIP conv backward covers 64 -> 64 channels only, got nf = {nf}")
    if act not in _EPI:
        raise ValueError(f"act must be None, 'relu' or 'lrelu', got {act!r}")
    if mfma not in _PACK:
        raise ValueError(f"mfma must be 'f16x3' or 'f32', got {mfma!r}")


class Conv3x3(nn.Module):
    """nn.Conv2d(64, 64, 3, 1, 1) with an optional fused ReLU / LeakyReLU(0.1), forward and backward on the HIP
    kernels.  ``weight`` [64, 64, 3, 3] and ``bias`` [64] carry nn.Conv2d's names, shapes and default
    initialisation.  Input and output are logical NCHW; the output is ``channels_last``, and a ``channels_last``
    input is read in place."""

    def __init__(self, nf: int = 64, act=None, mfma: str = "f16x3"):
        super().__init__()
        _check_choice(nf, act, mfma)
        self.act, self.mfma = act, mfma
        self.weight = nn.Parameter(torch.empty(nf, nf, 3, 3))
        self.bias = nn.Parameter(torch.empty(nf))
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))
        bound = 1.0 / math.sqrt(nf * 9)
        nn.init.uniform_(self.bias, -bound, bound)

    def forward(self, x):
        return _Conv3x3Fn.apply(x, self.weight, self.bias, self.act, _PACK[self.mfma])

    def range_status(self) -> int:
        return range_status(self.weight.device)

    def extra_repr(self):
        return f"64, 64, kernel_size=(3, 3), padding=1, act={self.act}, mfma={self.mfma}"


class ResidualBlock_noBN(nn.Module):
    """module_util.py:34-52: identity + conv2(relu(conv1(x))), submodules ``conv1`` / ``conv2`` as in the
    reference (kaiming-normal weights scaled by 0.1, zero biases), one autograd node on the HIP kernels."""

    def __init__(self, nf: int = 64, mfma: str = "f16x3"):
        super().__init__()
        _check_choice(nf, None, mfma)
        self.mfma = mfma
        self.conv1 = Conv3x3(nf, "relu", mfma)
        self.conv2 = Conv3x3(nf, None, mfma)
        with torch.no_grad():
            for m in (self.conv1, self.conv2):
                nn.init.kaiming_normal_(m.weight, a=0, mode="fan_in")
                m.weight.mul_(0.1)
                m.bias.zero_()

    def forward(self, x):
        return _ResBlockFn.apply(x, self.conv1.weight, self.conv1.bias, self.conv2.weight, self.conv2.bias,
                                 _PACK[self.mfma])

    def range_status(self) -> int:
        return range_status(self.conv1.weight.device)


def make_trunk(n_blocks: int, nf: int = 64, mfma: str = "f16x3") -> nn.Sequential:
    """module_util.make_layer of ``n_blocks`` ResidualBlock_noBN (keys ``0.conv1.weight``, ...): the
    ``recon_trunk.*`` / ``feature_extraction.*`` slices of a LunaTokis state dict load with ``strict=True``.
    ``trunk[0].range_status()`` (or ``train.range_status()``) reports the f16x3 range for the whole trunk."""
    return nn.Sequential(*[ResidualBlock_noBN(nf, mfma) for _ in range(n_blocks)])


# ---- the per-frame encoder: conv_first, the stride-2 pyramid convs, FrameFeatures ----

_DOWN_EPI = {None: L.EPI_NONE, "lrelu": L.EPI_LRELU}   # the epilogues the stride-2 forward kernel has


class _ConvDownFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, act):
        xh = _nhwc(x, "ConvDown")
        n, H, W, _ = xh.shape
        out = torch.empty(n, (H + 1) // 2, (W + 1) // 2, 64, dtype=torch.float32, device=xh.device)
        ops.conv2d([dict(layer=ops.pack_conv_plain_dev(weight, bias), in0=xh, out=out)], epi=_DOWN_EPI[act], stride=2)
        ctx.act = act
        ctx.save_for_backward(xh, weight, out if act else None)
        return out.permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, grad_out):
        xh, weight, out = ctx.saved_tensors
        g = _nhwc(grad_out, "ConvDown backward")
        if ctx.act == "lrelu":
            g = torch.where(out > 0, g, g * 0.1)
        need_x, need_w, need_b = ctx.needs_input_grad[:3]
        gx = gw = gb = None
        if need_w or need_b:
            gw, gb = ops.conv3x3s2_wgrad(xh, g)
        if need_x:
            gx = ops.conv3x3s2_dgrad(g, weight, xh.shape[1], xh.shape[2]).permute(0, 3, 1, 2)
        return gx, gw if need_w else None, gb if need_b else None, None


class ConvDown(nn.Module):
    """nn.Conv2d(64, 64, 3, 2, 1) with an optional fused LeakyReLU(0.1) (the pyramid's fea_L*_conv1), forward and
    backward on the HIP kernels in fp32: the forward is stif_conv2d_nhwc with the weight packed on the device, the
    backward stif_conv3x3s2_wgrad and stif_conv3x3s2_dgrad.  ``weight`` / ``bias`` as nn.Conv2d's; logical NCHW in
    and out, ``channels_last`` used in place."""

    def __init__(self, nf: int = 64, act="lrelu"):
        super().__init__()
        if nf != 64:
            raise ValueError(f"the HIP conv backward covers 64 -> 64 channels only, got nf = {nf}")
        if act not in _DOWN_EPI:
            raise ValueError(f"act must be None or 'lrelu' (the stride-2 forward kernel's epilogues), got {act!r}")
        self.act = act
        self.weight = nn.Parameter(torch.empty(nf, nf, 3, 3))
        self.bias = nn.Parameter(torch.empty(nf))
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))
        bound = 1.0 / math.sqrt(nf * 9)
        nn.init.uniform_(self.bias, -bound, bound)

    def forward(self, x):
        return _ConvDownFn.apply(x, self.weight, self.bias, self.act)

    def extra_repr(self):
        return f"64, 64, kernel_size=(3, 3), stride=2, padding=1, act={self.act}"


class _ConvFirstFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, frames, weight, bias):
        n, _, H, W = frames.shape
        out = torch.empty(n, H, W, 64, dtype=torch.float32, device=frames.device)
        ops.conv_first(frames, weight.detach().contiguous(), bias.detach().contiguous(), out)
        ctx.save_for_backward(frames, out)
        return out.permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, grad_out):
        frames, out = ctx.saved_tensors
        g = _nhwc(grad_out, "ConvFirst backward")
        g = torch.where(out > 0, g, g * 0.1)
        need_w, need_b = ctx.needs_input_grad[1:3]
        gw = gb = None
        if need_w or need_b:
            gw, gb = ops.conv_first_wgrad(frames, g)
        return None, gw if need_w else None, gb if need_b else None


class ConvFirst(nn.Module):
    """nn.Conv2d(3, 64, 3, 1, 1) + LeakyReLU(0.1) (Sakuya_arch_test.py:282, :318): forward on stif_conv_first,
    weight / bias gradient on stif_conv_first_wgrad.  The gradient with respect to the frames is not built: an
    input that requires grad is refused."""

    def __init__(self):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(64, 3, 3, 3))
        self.bias = nn.Parameter(torch.empty(64))
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))
        bound = 1.0 / math.sqrt(27)
        nn.init.uniform_(self.bias, -bound, bound)

    def forward(self, frames):
        if frames.requires_grad and torch.is_grad_enabled():
            raise NotImplementedError("ConvFirst: the gradient with respect to the input frames is not built "
                                      "(pass frames that do not require grad)")
        if not frames.is_cuda:
            raise RuntimeError(f"ConvFirst: the HIP convolution kernels need a CUDA tensor, got one on {frames.device} "
                               "(move the module and its input to the GPU)")
        if frames.dtype != torch.float32 or frames.dim() != 4 or frames.shape[1] != 3:
            raise RuntimeError(f"ConvFirst: expected a float32 [n, 3, H, W] tensor, got {frames.dtype} "
                               f"{tuple(frames.shape)}")
        return _ConvFirstFn.apply(frames.detach().contiguous(), self.weight, self.bias)

    def extra_repr(self):
        return "3, 64, kernel_size=(3, 3), padding=1, act=lrelu"


class FrameFeatures(nn.Module):
    """The reference's per-frame encoder (Sakuya_arch_test.py:282-287, :318-325) with its parameter names, so the
    ``conv_first.*``, ``feature_extraction.*`` and ``fea_L*_conv*`` slices of a LunaTokis state dict load with
    ``strict=True``: frames [n, 3, H, W] -> (L1, L2, L3), every conv forward and backward on the HIP kernels.
    ``mfma`` selects the operand mode of the Winograd convs; conv_first and the stride-2 convs are fp32."""

    def __init__(self, front_RBs: int = 5, mfma: str = "f16x3"):
        super().__init__()
        _check_choice(64, "lrelu", mfma)
        self.conv_first = ConvFirst()
        self.feature_extraction = make_trunk(front_RBs, 64, mfma)
        self.fea_L2_conv1 = ConvDown(64, "lrelu")
        self.fea_L2_conv2 = Conv3x3(64, "lrelu", mfma)
        self.fea_L3_conv1 = ConvDown(64, "lrelu")
        self.fea_L3_conv2 = Conv3x3(64, "lrelu", mfma)

    def forward(self, frames):
        L1 = self.feature_extraction(self.conv_first(frames))
        L2 = self.fea_L2_conv2(self.fea_L2_conv1(L1))
        L3 = self.fea_L3_conv2(self.fea_L3_conv1(L2))
        return L1, L2, L3

    def range_status(self) -> int:
        return range_status(self.conv_first.weight.device)
