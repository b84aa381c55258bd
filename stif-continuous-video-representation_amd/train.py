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
module and one target.  The inference model (``model.LunaTokis``) stays inference-only; the whole model trains here as
``train.LunaTokis`` (last entry below).  The model's operators train on the engine's own kernels: the DCN_sep layers of a torch module through the ``_ext`` drop-in
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
* ``Upsample2x``, ``Conv3x3Cat``, ``DCN_sep``, ``PCD_Align`` -- the alignment module that consumes the encoder's three
  levels (Sakuya_arch_test.py:20-130, dcn_v2.py:110-140) with the reference's parameter names: the 128 -> 64 convs run
  on their two inputs without a concatenation (stif_conv3x3_wino with two inputs; backward stif_conv3x3_wgrad_cat,
  the weight gradient in 64 x 64 channel blocks, and one 64 -> 64 data-gradient conv per input), the x2 upsample has
  its adjoint kernel (stif_upsample2x_bwd_nhwc), and DCN_sep's 64 -> 216 offset / mask conv trains through the same
  block kernels on a zero-padded 256-channel map (weights packed by stif_pack_conv_block_dev).  The deformable conv
  itself stays in NHWC: stif_dcn_offmask_nhwc, the fused forward stif_dcn_nhwc (fp32) and its backward
  stif_dcn_bwd_nhwc, which writes the offset / mask conv's output gradient in place of any torch assembly.
* ``Conv1x1Cat``, ``ConvLSTMCell``, ``Easy_PCD``, ``DeformableConvLSTM``, ``BiDeformableConvLSTM``, ``GenFeat`` -- the
  rest of LunaTokis.gen_feat (Sakuya_arch_test.py:132-266, :313-362): the 1x1 (64 | 64) -> 64 convs (forward
  stif_conv2d_nhwc on the device pack of stif_pack_conv1x1_dev, backward stif_conv1x1_wgrad and fp32 1x1 data-gradient
  convs), the ConvLSTM cell as one node (the 128 -> 256 Winograd conv writes the pre-activations, stif_lstm_gates_nhwc
  the state; the backward recomputes the gates from them), and the compositions up to ``GenFeat``, which takes an
  optimiser step on everything before the SIREN decoder.
* ``Siren``, ``Decoder``, ``LunaTokis``, ``TimesLoss`` -- the SIREN decoder (SIREN.py:27-79, Sakuya_arch_test.py:304-311,
  :364-459) and the whole model (:1222-1231, ``test=False``), DESIGN.md section 3o.  In training the three MLP input
  matrices are materialised in HBM, one fp32 row per HR pixel (stif_dec_x1_fwd / x2 / x3 and their adjoints; only the
  two warped scatters of stif_dec_x3_bwd use atomics, unless ``set_deterministic`` is on), and each MLP is one autograd node over stif_siren_fwd (which saves
  the sine layers' pre-activations) and stif_siren_bwd (fp32 MFMA, deterministic weight gradients).  ``LunaTokis`` holds
  the reference's 442 keys (the eight of the unused upsampling layers never receive a gradient) and takes an optimiser
  step through ``optimize_step`` with ``TimesLoss(CharbonnierLoss())``.  The decoder is fp32 in both ``mfma`` modes.
"""
from __future__ import annotations

import contextlib
import math
from collections import Counter, defaultdict

import torch
import torch.distributed as dist
from torch import nn
from torch.optim.lr_scheduler import LRScheduler

from . import _lib as L
from . import ops

_DETERMINISTIC = False


def set_deterministic(enabled: bool) -> None:
    """Reproducible backward passes for the whole model: with True, the three order-dependent sums of training -- g_in
    of the deformable conv (``DCN_sep``) and g_hrfeat / g_feat of the decoder's warped gather -- are ordered segment
    sums (ops.dcn_bwd / ops.dec_x3_bwd with ``deterministic=True``) in place of fp32 atomics, so
    that two steps from the same state on the same batch give the same bytes.  Every other kernel adds in a fixed
    order either way.  The backward nodes read the switch when they run.  Off by default, and
    ``torch.use_deterministic_algorithms`` is deliberately not consulted: turning that flag on elsewhere must not
    change what these modules compute or cost."""
    global _DETERMINISTIC
    _DETERMINISTIC = bool(enabled)


def is_deterministic() -> bool:
    return _DETERMINISTIC


@contextlib.contextmanager
def deterministic(enabled: bool = True):
    """``with train.deterministic():`` -- set_deterministic(enabled) for the block (the backward must run inside
    it), then the previous state again; nests."""
    previous = is_deterministic()
    set_deterministic(enabled)
    try:
        yield
    finally:
        set_deterministic(previous)


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
    s = _STATUS.get(device.index)     # a tensor's device carries its index: one lookup per conv
    if s is None:
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


def _need_cuda(who: str, *tensors) -> None:
    """The one refusal of CPU tensors, before any launch."""
    for t in tensors:
        if not t.is_cuda:
            raise RuntimeError(f"{who}: the HIP convolution kernels need a CUDA tensor, got one on {t.device} "
                               "(move the module and its input to the GPU)")


def _nhwc(t: torch.Tensor, what: str, channels=64) -> torch.Tensor:
    """The NHWC buffer of a logical NCHW tensor: a ``channels_last`` tensor is used in place (its memory is
    NHWC), anything else is converted once.  ``channels`` None: any positive multiple of 4."""
    if not t.is_cuda:
        _need_cuda(what, t)
    if channels is None and (t.dtype != torch.float32 or t.dim() != 4 or t.shape[1] % 4 or t.shape[1] < 4):
        raise RuntimeError(f"{what}: expected a float32 [n, 4k, H, W] tensor, got {t.dtype} {tuple(t.shape)}")
    if channels is not None and (t.dtype != torch.float32 or t.dim() != 4 or t.shape[1] != channels):
        raise RuntimeError(f"{what}: expected a float32 [n, 64, H, W] tensor, got {t.dtype} {tuple(t.shape)}")
    v = t.detach().permute(0, 2, 3, 1)
    return v if v.is_contiguous() else v.contiguous()


def _nchw(t):
    """The logical NCHW view of an NHWC buffer (``channels_last`` memory); None stays None."""
    return None if t is None else t.permute(0, 3, 1, 2)


def _same_shape(who: str, first, *others) -> None:
    """The inputs of a node (logical NCHW) must have one shape."""
    for m in others:
        if m.shape != first.shape:
            raise RuntimeError(f"{who}: the inputs differ in shape: "
                               + ", ".join(str(tuple(t.shape)) for t in (first,) + others))


def _act_grad(g, out, act):
    """The gradient before a fused activation from the gradient after it and the activation's saved output: both
    activations keep the sign of their argument."""
    if act == "relu":
        return g * (out > 0)
    if act == "lrelu":
        return torch.where(out > 0, g, g * 0.1)
    return g


def _grads(needs, *values) -> tuple:
    """A backward's result: ``values[i]`` where input i needs a gradient, None where it does not and for every input
    past the values (the options)."""
    out = [None] * len(needs)
    for i, v in enumerate(values):
        if needs[i]:
            out[i] = v
    return tuple(out)


def _wino(x, weight, bias, mode, epi=L.EPI_NONE, res=None):
    """stif_conv3x3_wino of NHWC ``x`` with the 64 -> 64 ``weight`` packed on the device for this call; returns a new
    NHWC tensor."""
    status = _status_word(x.device)
    lay = ops.pack_conv_dev(weight, bias, mode, status=status)
    out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    ops.conv2d([dict(layer=lay, in0=x, out=out, res=res)], epi=epi, status=status)
    return out


def _conv_dgrad(g, weight, mode, *, half=None, res=None, epi=L.EPI_NONE):
    """The data gradient of a stride-1 conv as a conv of NHWC ``g`` (the gradient of its output) with ``weight``
    packed on the device in its data-gradient form; returns a new NHWC [n, H, W, 64] tensor.  The form follows the
    weight: [64, 64, 3, 3] (64 -> 64), [64, 128, 3, 3] ((64 | 64) -> 64), [216, 64, 3, 3] (g the zero-padded 256-channel
    map) and [256, 128, 3, 3] ((64 | 64) -> 256) on stif_conv3x3_wino in ``mode``, [64, 128, 1, 1] as an fp32 1x1 conv
    without a status word (the split-fp16 1x1 kernel takes the (64 | 64) and 200-channel inputs only).  ``half``: which
    input of a two-input conv; ``res`` / ``epi``: the conv's epilogue."""
    if weight.shape[2] == 1:
        status, lay = None, ops.pack_conv1x1_dev(weight, None, L.PACK_PLAIN, dgrad=True, half=half)
    else:
        status = _status_word(g.device)
        if tuple(weight.shape[:2]) == (64, 64):
            lay = ops.pack_conv_dev(weight, None, mode, dgrad=True, status=status)
        else:
            lay = ops.pack_conv_blocks_dev(weight, None, mode, dgrad=True, half=half, status=status)
    gx = torch.empty(tuple(g.shape[:3]) + (64,), dtype=torch.float32, device=g.device)
    ops.conv2d([dict(layer=lay, in0=g, out=gx, res=res)], epi=epi, status=status)
    return gx


def _conv2d_params(cout, cin, ks, init="conv2d"):
    """``weight`` [cout, cin, ks, ks] and ``bias`` [cout] of an nn.Conv2d as parameters, with its default
    initialisation (the weight is drawn first) or, ``init="zeros"``, zeros."""
    if init == "zeros":
        return nn.Parameter(torch.zeros(cout, cin, ks, ks)), nn.Parameter(torch.zeros(cout))
    weight, bias = nn.Parameter(torch.empty(cout, cin, ks, ks)), nn.Parameter(torch.empty(cout))
    nn.init.kaiming_uniform_(weight, a=math.sqrt(5))
    bound = 1.0 / math.sqrt(cin * ks * ks)
    nn.init.uniform_(bias, -bound, bound)
    return weight, bias


class _RangeStatus:
    """``module.range_status()``: ``train.range_status`` of the device of the module's first parameter."""

    def range_status(self) -> int:
        return range_status(next(self.parameters()).device)


class _ConvFn(torch.autograd.Function):
    """The stride-1 conv of one or two 64-channel inputs (``b`` None: one) to 64 channels with an optional fused
    activation.  The kernel size and the packing follow the weight: [64, 64, 3, 3] and [64, 128, 3, 3] run on
    stif_conv3x3_wino, [64, 128, 1, 1] on stif_conv2d_nhwc.  ``who`` names the module in messages."""

    @staticmethod
    def forward(ctx, who, a, b, weight, bias, act, mode):
        ah = _nhwc(a, who)
        status = _status_word(ah.device)
        out = torch.empty(ah.shape, dtype=torch.float32, device=ah.device)
        if b is None:
            lay = ops.pack_conv_dev(weight, bias, mode, status=status)
            ops.conv2d([dict(layer=lay, in0=ah, out=out)], epi=_EPI[act], status=status)
            ctx.save_for_backward(weight, out if act else None, ah)
        else:
            bh = _nhwc(b, who)
            _same_shape(who, a, b)
            pack = ops.pack_conv1x1_dev if weight.shape[2] == 1 else ops.pack_conv_blocks_dev
            lay = pack(weight, bias, mode, status=status)
            ops.conv2d([dict(layer=lay, in0=ah, in1=bh, out=out)], epi=_EPI[act], in1_mode=1, status=status)
            ctx.save_for_backward(weight, out if act else None, ah, bh)
        ctx.who, ctx.act, ctx.mode = who, act, mode
        return out.permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, grad_out):
        weight, out, *xs = ctx.saved_tensors
        g = _act_grad(_nhwc(grad_out, ctx.who + " backward"), out, ctx.act)
        needs = ctx.needs_input_grad
        gw = gb = None
        if needs[3] or needs[4]:
            if weight.shape[2] == 1:
                gw, gb = ops.conv1x1_wgrad(xs, g)
            elif len(xs) == 1:
                gw, gb = ops.conv3x3_wgrad(xs[0], g)
            else:
                gw, gb = ops.conv3x3_wgrad_cat(xs, g, 64)
        two = len(xs) == 2
        ga = _nchw(_conv_dgrad(g, weight, ctx.mode, half=0 if two else None)) if needs[1] else None
        gb2 = _nchw(_conv_dgrad(g, weight, ctx.mode, half=1)) if two and needs[2] else None
        return _grads(needs, None, ga, gb2, gw, gb)


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
        return _nchw(out)

    @staticmethod
    def backward(ctx, grad_out):
        xh, t, w1, w2 = ctx.saved_tensors
        g = _nhwc(grad_out, "ResidualBlock_noBN backward")
        need_x, need_w1, need_b1, need_w2, need_b2 = ctx.needs_input_grad[:5]
        gx = gw1 = gb1 = gw2 = gb2 = None
        if need_w2 or need_b2:
            gw2, gb2 = ops.conv3x3_wgrad(t, g)
        if need_x or need_w1 or need_b1:
            gt = _act_grad(_conv_dgrad(g, w2, ctx.mode), t, "relu")
            if need_w1 or need_b1:
                gw1, gb1 = ops.conv3x3_wgrad(xh, gt)
            if need_x:
                gx = _nchw(_conv_dgrad(gt, w1, ctx.mode, res=g, epi=L.EPI_RES))
        return _grads(ctx.needs_input_grad, gx, gw1, gb1, gw2, gb2)


def _check_choice(nf, act, mfma):
    if nf != 64:
        raise ValueError(f"the HIP conv backward covers 64 -> 64 channels only, got nf = {nf}")
    if act not in _EPI:
        raise ValueError(f"act must be None, 'relu' or 'lrelu', got {act!r}")
    if mfma not in _PACK:
        raise ValueError(f"mfma must be 'f16x3' or 'f32', got {mfma!r}")


class Conv3x3(_RangeStatus, nn.Module):
    """nn.Conv2d(64, 64, 3, 1, 1) with an optional fused ReLU / LeakyReLU(0.1), forward and backward on the HIP
    kernels.  ``weight`` [64, 64, 3, 3] and ``bias`` [64] carry nn.Conv2d's names, shapes and default
    initialisation.  Input and output are logical NCHW; the output is ``channels_last``, and a ``channels_last``
    input is read in place."""

    def __init__(self, nf: int = 64, act=None, mfma: str = "f16x3"):
        super().__init__()
        _check_choice(nf, act, mfma)
        self.act, self.mfma = act, mfma
        self.weight, self.bias = _conv2d_params(nf, nf, 3)

    def forward(self, x):
        return _ConvFn.apply("Conv3x3", x, None, self.weight, self.bias, self.act, _PACK[self.mfma])

    def extra_repr(self):
        return f"64, 64, kernel_size=(3, 3), padding=1, act={self.act}, mfma={self.mfma}"


class ResidualBlock_noBN(_RangeStatus, nn.Module):
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
        return _nchw(out)

    @staticmethod
    def backward(ctx, grad_out):
        xh, weight, out = ctx.saved_tensors
        g = _act_grad(_nhwc(grad_out, "ConvDown backward"), out, ctx.act)
        need_x, need_w, need_b = ctx.needs_input_grad[:3]
        gw, gb = ops.conv3x3s2_wgrad(xh, g) if need_w or need_b else (None, None)
        gx = _nchw(ops.conv3x3s2_dgrad(g, weight, xh.shape[1], xh.shape[2])) if need_x else None
        return _grads(ctx.needs_input_grad, gx, gw, gb)


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
        self.weight, self.bias = _conv2d_params(nf, nf, 3)

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
        return _nchw(out)

    @staticmethod
    def backward(ctx, grad_out):
        frames, out = ctx.saved_tensors
        g = _act_grad(_nhwc(grad_out, "ConvFirst backward"), out, "lrelu")
        need_w, need_b = ctx.needs_input_grad[1:3]
        gw, gb = ops.conv_first_wgrad(frames, g) if need_w or need_b else (None, None)
        return _grads(ctx.needs_input_grad, None, gw, gb)


class ConvFirst(nn.Module):
    """nn.Conv2d(3, 64, 3, 1, 1) + LeakyReLU(0.1) (Sakuya_arch_test.py:282, :318): forward on stif_conv_first,
    weight / bias gradient on stif_conv_first_wgrad.  The gradient with respect to the frames is not built: an
    input that requires grad is refused."""

    def __init__(self):
        super().__init__()
        self.weight, self.bias = _conv2d_params(64, 3, 3)

    def forward(self, frames):
        if frames.requires_grad and torch.is_grad_enabled():
            raise NotImplementedError("ConvFirst: the gradient with respect to the input frames is not built "
                                      "(pass frames that do not require grad)")
        _need_cuda("ConvFirst", frames)
        if frames.dtype != torch.float32 or frames.dim() != 4 or frames.shape[1] != 3:
            raise RuntimeError(f"ConvFirst: expected a float32 [n, 3, H, W] tensor, got {frames.dtype} "
                               f"{tuple(frames.shape)}")
        return _ConvFirstFn.apply(frames.detach().contiguous(), self.weight, self.bias)

    def extra_repr(self):
        return "3, 64, kernel_size=(3, 3), padding=1, act=lrelu"


def _add_pyramid(mod: nn.Module, mfma: str) -> None:
    """Register the reference's four pyramid convs on ``mod`` under their names, in its order."""
    mod.fea_L2_conv1 = ConvDown(64, "lrelu")
    mod.fea_L2_conv2 = Conv3x3(64, "lrelu", mfma)
    mod.fea_L3_conv1 = ConvDown(64, "lrelu")
    mod.fea_L3_conv2 = Conv3x3(64, "lrelu", mfma)


def _pyramid(mod: nn.Module, L1):
    """(L2, L3) of L1 through ``mod``'s pyramid convs."""
    L2 = mod.fea_L2_conv2(mod.fea_L2_conv1(L1))
    return L2, mod.fea_L3_conv2(mod.fea_L3_conv1(L2))


class FrameFeatures(_RangeStatus, nn.Module):
    """The reference's per-frame encoder (Sakuya_arch_test.py:282-287, :318-325) with its parameter names, so the
    ``conv_first.*``, ``feature_extraction.*`` and ``fea_L*_conv*`` slices of a LunaTokis state dict load with
    ``strict=True``: frames [n, 3, H, W] -> (L1, L2, L3), every conv forward and backward on the HIP kernels.
    ``mfma`` selects the operand mode of the Winograd convs; conv_first and the stride-2 convs are fp32."""

    def __init__(self, front_RBs: int = 5, mfma: str = "f16x3"):
        super().__init__()
        _check_choice(64, "lrelu", mfma)
        self.conv_first = ConvFirst()
        self.feature_extraction = make_trunk(front_RBs, 64, mfma)
        _add_pyramid(self, mfma)

    def forward(self, frames):
        L1 = self.feature_extraction(self.conv_first(frames))
        return (L1, *_pyramid(self, L1))


# ---- PCD_Align: the concatenation convs, the x2 upsample, DCN_sep (Sakuya_arch_test.py:20-130, dcn_v2.py:110-140) ----

class _Upsample2xFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, scale):
        xh = _nhwc(x, "Upsample2x", None)
        n, h, w, c = xh.shape
        out = torch.empty(n, 2 * h, 2 * w, c, dtype=torch.float32, device=xh.device)
        ops.upsample2x(xh, out, scale)
        ctx.scale = scale
        return _nchw(out)

    @staticmethod
    def backward(ctx, grad_out):
        return _nchw(ops.upsample2x_bwd(_nhwc(grad_out, "Upsample2x backward", None), ctx.scale)), None


class Upsample2x(nn.Module):
    """``scale`` * F.interpolate(x, scale_factor=2, mode='bilinear', align_corners=False) as one autograd node:
    forward stif_upsample2x_nhwc, backward its adjoint stif_upsample2x_bwd_nhwc.  Logical NCHW in and out
    (``channels_last`` memory), channels a multiple of 4."""

    def __init__(self, scale: float = 1.0):
        super().__init__()
        self.scale = float(scale)

    def forward(self, x):
        return _Upsample2xFn.apply(x, self.scale)

    def extra_repr(self):
        return f"scale={self.scale}"


class Conv3x3Cat(_RangeStatus, nn.Module):
    """nn.Conv2d(128, 64, 3, 1, 1) applied to torch.cat([a, b], 1) with an optional fused ReLU / LeakyReLU(0.1),
    without the concatenation: the forward is one stif_conv3x3_wino launch with two inputs, the backward
    stif_conv3x3_wgrad_cat and one 64 -> 64 Winograd data-gradient conv per input that needs one.  ``weight``
    [64, 128, 3, 3] and ``bias`` [64] as nn.Conv2d's (names, shapes, default initialisation)."""

    def __init__(self, act=None, mfma: str = "f16x3"):
        super().__init__()
        _check_choice(64, act, mfma)
        self.act, self.mfma = act, mfma
        self.weight, self.bias = _conv2d_params(64, 128, 3)

    def forward(self, a, b):
        return _ConvFn.apply("Conv3x3Cat", a, b, self.weight, self.bias, self.act, _PACK[self.mfma])

    def extra_repr(self):
        return f"128, 64, kernel_size=(3, 3), padding=1, act={self.act}, mfma={self.mfma}"


class _DCNSepFn(torch.autograd.Function):
    """DCN_sep as one node that never leaves NHWC.  The offset / mask conv writes the zero-padded 256-channel map om
    (channels 0..143 the reference's cat(o1, o2), 144..215 the mask logits, 216..255 zeros); stif_dcn_offmask_nhwc
    turns it into the offmask the fused deformable conv stif_dcn_nhwc reads; the backward is one stif_dcn_bwd_nhwc
    call, whose g_om is the offset / mask conv's output gradient as it stands."""

    @staticmethod
    def forward(ctx, inp, fea, weight, bias, om_weight, om_bias, act, mode):
        feah, xh = _nhwc(fea, "DCN_sep"), _nhwc(inp, "DCN_sep")
        _same_shape("DCN_sep", inp, fea)
        status = _status_word(feah.device)
        n, H, W, _ = feah.shape
        om = torch.empty(n, H, W, 256, dtype=torch.float32, device=feah.device)
        ops.conv2d([dict(layer=ops.pack_conv_blocks_dev(om_weight, om_bias, mode, status=status), in0=feah, out=om)],
                   status=status)
        offmask = ops.dcn_offmask(om)
        out = torch.empty(n, H, W, 64, dtype=torch.float32, device=feah.device)
        ops.dcn([dict(layer=ops.pack_conv_plain_dev(weight, bias), inp=xh, offmask=offmask, out=out)], epi=_EPI[act])
        ctx.act, ctx.mode = act, mode
        ctx.save_for_backward(xh, offmask, feah, weight, om_weight, out if act else None)
        return _nchw(out)

    @staticmethod
    def backward(ctx, grad_out):
        xh, offmask, feah, weight, om_weight, out = ctx.saved_tensors
        g = _nhwc(grad_out, "DCN_sep backward")
        need_in, need_fea, need_w, need_b, need_omw, need_omb = ctx.needs_input_grad[:6]
        need = (need_in, need_fea or need_omw or need_omb, need_w or need_b)
        g_in = g_om = g_w = g_b = None
        if any(need):
            g_in, g_om, g_w, g_b = ops.dcn_bwd(xh, offmask, weight, g, out=out, epi=_EPI[ctx.act], need=need,
                                               deterministic=_DETERMINISTIC)
        g_omw, g_omb = ops.conv3x3_wgrad_cat([feah], g_om, 216) if need_omw or need_omb else (None, None)
        g_fea = _conv_dgrad(g_om, om_weight, ctx.mode) if need_fea else None
        return _grads(ctx.needs_input_grad, _nchw(g_in), _nchw(g_fea), g_w, g_b, g_omw, g_omb)


class _ConvParams(nn.Module):
    """The parameters of an nn.Conv2d(cin, cout, 3) (``weight``, ``bias``) under its names, with no forward of its own;
    ``init`` as _conv2d_params."""

    def __init__(self, cout, cin, init="conv2d"):
        super().__init__()
        self.weight, self.bias = _conv2d_params(cout, cin, 3, init)


class DCN_sep(_RangeStatus, nn.Module):
    """dcn_v2.py:110-140 for 64 -> 64 channels, 3x3, 8 deformable groups, trainable on the engine: ``forward(input,
    fea)`` = the modulated deformable conv of ``input`` with offsets and masks from ``conv_offset_mask(fea)``,
    optionally followed by LeakyReLU(0.1).  Parameters under the reference's names -- ``weight``, ``bias``,
    ``conv_offset_mask.weight`` [216, 64, 3, 3], ``conv_offset_mask.bias`` -- with its initialisation (uniform
    weight, zero bias, zeroed offset conv).  The offset / mask conv and its data gradient are stif_conv3x3_wino, its
    weight gradient stif_conv3x3_wgrad_cat, the deformable conv stif_dcn_nhwc (fp32, after stif_dcn_offmask_nhwc) with
    the backward stif_dcn_bwd_nhwc; gradients that are not needed are not computed."""

    def __init__(self, act=None, mfma: str = "f16x3"):
        super().__init__()
        if act not in (None, "lrelu"):
            raise ValueError(f"act must be None or 'lrelu', got {act!r}")
        _check_choice(64, None, mfma)
        self.act, self.mfma = act, mfma
        self.weight = nn.Parameter(torch.empty(64, 64, 3, 3))
        self.bias = nn.Parameter(torch.zeros(64))
        stdv = 1.0 / math.sqrt(64 * 9)
        nn.init.uniform_(self.weight, -stdv, stdv)
        self.conv_offset_mask = _ConvParams(216, 64, "zeros")

    def forward(self, input, fea):
        return _DCNSepFn.apply(input, fea, self.weight, self.bias, self.conv_offset_mask.weight,
                               self.conv_offset_mask.bias, self.act, _PACK[self.mfma])

    def extra_repr(self):
        return f"64, 64, kernel_size=(3, 3), padding=1, deformable_groups=8, act={self.act}, mfma={self.mfma}"


class PCD_Align(_RangeStatus, nn.Module):
    """Sakuya_arch_test.py:20-130 with the reference's submodule names and registration order, so the ``pcd_align.*``
    slice of a LunaTokis state dict (and ``ConvBLSTM.forward_net.pcd_h.pcd_align.*`` / ``...pcd_c.pcd_align.*``) loads
    with ``strict=True``: ``forward(fea1, fea2)`` takes two lists [L1, L2, L3] of logical-NCHW 64-channel maps and
    returns [B, 128, H, W], every conv, upsample and deformable conv forward and backward on the HIP kernels."""

    def __init__(self, mfma: str = "f16x3"):
        super().__init__()
        _check_choice(64, None, mfma)
        for s in ("_1", "_2"):
            self.add_module("L3_offset_conv1" + s, Conv3x3Cat("lrelu", mfma))
            self.add_module("L3_offset_conv2" + s, Conv3x3(64, "lrelu", mfma))
            self.add_module("L3_dcnpack" + s, DCN_sep("lrelu", mfma))
            for lv in ("L2", "L1"):
                self.add_module(f"{lv}_offset_conv1" + s, Conv3x3Cat("lrelu", mfma))
                self.add_module(f"{lv}_offset_conv2" + s, Conv3x3Cat("lrelu", mfma))
                self.add_module(f"{lv}_offset_conv3" + s, Conv3x3(64, "lrelu", mfma))
                self.add_module(f"{lv}_dcnpack" + s, DCN_sep(None, mfma))
                self.add_module(f"{lv}_fea_conv" + s, Conv3x3Cat("lrelu" if lv == "L2" else None, mfma))
        self.up_offset = Upsample2x(2.0)     # F.interpolate(offset) * 2
        self.up_fea = Upsample2x(1.0)

    def _branch(self, s, fa, fb):
        m = lambda name: getattr(self, name + s)
        L3_off = m("L3_offset_conv2")(m("L3_offset_conv1")(fa[2], fb[2]))
        L3_fea = m("L3_dcnpack")(fa[2], L3_off)
        L2_off = m("L2_offset_conv1")(fa[1], fb[1])
        L2_off = m("L2_offset_conv3")(m("L2_offset_conv2")(L2_off, self.up_offset(L3_off)))
        L2_fea = m("L2_fea_conv")(m("L2_dcnpack")(fa[1], L2_off), self.up_fea(L3_fea))
        L1_off = m("L1_offset_conv1")(fa[0], fb[0])
        L1_off = m("L1_offset_conv3")(m("L1_offset_conv2")(L1_off, self.up_offset(L2_off)))
        return m("L1_fea_conv")(m("L1_dcnpack")(fa[0], L1_off), self.up_fea(L2_fea))

    def branches(self, fea1, fea2):
        """The two 64-channel halves of ``forward``'s result (the inputs checked as there): what a consumer that takes
        its two inputs apart (``Conv1x1Cat``) reads without the concatenation."""
        fea1, fea2 = list(fea1), list(fea2)
        if len(fea1) != 3 or len(fea2) != 3:
            raise ValueError("PCD_Align: fea1 and fea2 are lists [L1, L2, L3]")
        if fea1[0].dim() != 4:
            raise ValueError(f"PCD_Align: expected [B, 64, H, W] maps, got {tuple(fea1[0].shape)}")
        B, _, H, W = fea1[0].shape
        if H % 4 or W % 4:
            raise ValueError(f"PCD_Align: H and W must be multiples of 4 (three pyramid levels), got {H} x {W}")
        for lv in range(3):
            want = (B, 64, H >> lv, W >> lv)
            if tuple(fea1[lv].shape) != want or tuple(fea2[lv].shape) != want:
                raise ValueError(f"PCD_Align: level L{lv + 1} must be {want}, got {tuple(fea1[lv].shape)} and "
                                 f"{tuple(fea2[lv].shape)}")
        _need_cuda("PCD_Align", *fea1, *fea2)     # a CPU tensor is refused before any launch
        return self._branch("_1", fea1, fea2), self._branch("_2", fea2, fea1)

    def forward(self, fea1, fea2):
        return torch.cat(self.branches(fea1, fea2), dim=1)


# ---- Easy_PCD, the ConvLSTM cell, BiDeformableConvLSTM, gen_feat (Sakuya_arch_test.py:132-266, :313-362) ----

_PACK1 = {"f16x3": L.PACK_PLAIN | L.PACK_F16X3, "f32": L.PACK_PLAIN}   # the 1x1 layers' packings


class Conv1x1Cat(_RangeStatus, nn.Module):
    """nn.Conv2d(128, 64, 1) applied to torch.cat([a, b], 1) without the concatenation (``fusion``,
    ``Easy_PCD.fusion``, ``ConvBLSTM.conv_1x1``): the forward is stif_conv2d_nhwc with two inputs on the weight packed
    by stif_pack_conv1x1_dev, the backward stif_conv1x1_wgrad and one fp32 1x1 64 -> 64 conv per input that needs a
    gradient.  ``weight`` [64, 128, 1, 1] and ``bias`` [64] as nn.Conv2d's (names, shapes, default initialisation)."""

    def __init__(self, mfma: str = "f16x3"):
        super().__init__()
        _check_choice(64, None, mfma)
        self.mfma = mfma
        self.weight, self.bias = _conv2d_params(64, 128, 1)

    def forward(self, a, b):
        return _ConvFn.apply("Conv1x1Cat", a, b, self.weight, self.bias, None, _PACK1[self.mfma])

    def extra_repr(self):
        return f"128, 64, kernel_size=(1, 1), mfma={self.mfma}"


class _ConvLSTMCellFn(torch.autograd.Function):
    """The whole cell as one node: the two-input Winograd conv writes the 256 pre-activations in the reference's row
    order, stif_lstm_gates_nhwc the new state.  Saved: the three inputs and the pre-activations; the backward
    recomputes the gates (stif_lstm_gates_bwd_nhwc)."""

    @staticmethod
    def forward(ctx, x, h, c, weight, bias, mode):
        xh, hh, ch = (_nhwc(t, "ConvLSTMCell") for t in (x, h, c))
        _same_shape("ConvLSTMCell", x, h, c)
        status = _status_word(xh.device)
        n, H, W, _ = xh.shape
        pre = torch.empty(n, H, W, 256, dtype=torch.float32, device=xh.device)
        ops.conv2d([dict(layer=ops.pack_conv_blocks_dev(weight, bias, mode, status=status), in0=xh, in1=hh, out=pre)],
                   in1_mode=1, status=status)
        h_next, c_next = ops.lstm_gates(pre, ch)
        ctx.mode = mode
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(xh, hh, ch, pre, weight)
        return _nchw(h_next), _nchw(c_next)

    @staticmethod
    def backward(ctx, g_h, g_c):
        xh, hh, ch, pre, weight = ctx.saved_tensors
        if g_h is None and g_c is None:
            return (None,) * 6
        g_h = None if g_h is None else _nhwc(g_h, "ConvLSTMCell backward")
        g_c = None if g_c is None else _nhwc(g_c, "ConvLSTMCell backward")
        need_x, need_h, need_c, need_w, need_b = ctx.needs_input_grad[:5]
        g_pre, g_cc = ops.lstm_gates_bwd(pre, ch, g_h, g_c, need_c=need_c)
        gw, gb = ops.conv3x3_wgrad_cat([xh, hh], g_pre, 256) if need_w or need_b else (None, None)
        gin = [_nchw(_conv_dgrad(g_pre, weight, ctx.mode, half=half)) if need else None
               for half, need in enumerate((need_x, need_h))]
        return _grads(ctx.needs_input_grad, gin[0], gin[1], _nchw(g_cc), gw, gb)


class ConvLSTMCell(_RangeStatus, nn.Module):
    """convlstm.py:8-58 for 64 input and 64 hidden channels, 3x3: ``forward(x, (h, c)) -> (h_next, c_next)`` with
    ``conv.weight`` [256, 128, 3, 3] / ``conv.bias`` [256] under the reference's names (rows: gates i, f, o, g of 64
    hidden channels each).  One autograd node: forward stif_conv3x3_wino on (x | h) and stif_lstm_gates_nhwc; backward
    stif_lstm_gates_bwd_nhwc, stif_conv3x3_wgrad_cat in eight 64 x 64 blocks and one 256 -> 64 Winograd data-gradient
    conv per input that needs one."""

    def __init__(self, mfma: str = "f16x3"):
        super().__init__()
        _check_choice(64, None, mfma)
        self.mfma = mfma
        self.conv = _ConvParams(256, 128)

    def forward(self, x, state):
        h, c = state
        return _ConvLSTMCellFn.apply(x, h, c, self.conv.weight, self.conv.bias, _PACK[self.mfma])


def _check_maps(who, maps, what="[B, 64, H, W]"):
    """CPU tensors, wrong shapes and sizes that the three pyramid levels cannot halve are refused before any launch."""
    first = maps[0]
    for t in maps:
        if t.dim() != 4 or t.shape[1] != 64 or t.shape != first.shape:
            raise ValueError(f"{who}: expected {what} maps of one shape, got {[tuple(m.shape) for m in maps]}")
    if first.shape[2] % 4 or first.shape[3] % 4:
        raise ValueError(f"{who}: H and W must be multiples of 4 (three pyramid levels), got "
                         f"{first.shape[2]} x {first.shape[3]}")
    _need_cuda(who, *maps)


class Easy_PCD(_RangeStatus, nn.Module):
    """Sakuya_arch_test.py:132-166 with the reference's submodule names and registration order: the two-level pyramid
    of both inputs (one pass over the 2B stacked items), ``pcd_align`` and the 1x1 ``fusion`` on its two halves.
    ``forward(f1, f2)``: [B, 64, H, W] each -> [B, 64, H, W], H and W multiples of 4."""

    def __init__(self, mfma: str = "f16x3"):
        super().__init__()
        _check_choice(64, None, mfma)
        _add_pyramid(self, mfma)
        self.pcd_align = PCD_Align(mfma)
        self.fusion = Conv1x1Cat(mfma)

    def forward(self, f1, f2):
        _check_maps("Easy_PCD", [f1, f2])
        B = f1.shape[0]
        L2, L3 = _pyramid(self, torch.cat([f1, f2], dim=0))     # the reference stacks on dim 1; the convs are per item
        a, b = self.pcd_align.branches([f1, L2[:B], L3[:B]], [f2, L2[B:], L3[B:]])
        return self.fusion(a, b)


class DeformableConvLSTM(nn.Module):
    """Sakuya_arch_test.py:168-245 for one layer of 64 channels with the reference's submodule names and registration
    order (``cell_list.0``, ``pcd_h``, ``pcd_c``): ``forward(x)``, x [B, T, 64, H, W] -> the hidden states
    [B, T, 64, H, W], from a zero initial state on x's device."""

    def __init__(self, mfma: str = "f16x3"):
        super().__init__()
        _check_choice(64, None, mfma)
        self.cell_list = nn.ModuleList([ConvLSTMCell(mfma)])
        self.pcd_h = Easy_PCD(mfma)
        self.pcd_c = Easy_PCD(mfma)

    def forward(self, x):
        if x.dim() != 5:
            raise ValueError(f"DeformableConvLSTM: expected [B, T, 64, H, W], got {tuple(x.shape)}")
        _check_maps("DeformableConvLSTM", [x[:, 0]], "[B, T, 64, H, W]")
        h = c = torch.zeros_like(x[:, 0])
        outs = []
        for t in range(x.shape[1]):
            xt = x[:, t]
            h, c = self.cell_list[0](xt, (self.pcd_h(xt, h), self.pcd_c(xt, c)))
            outs.append(h)
        return torch.stack(outs, dim=1)


class BiDeformableConvLSTM(_RangeStatus, nn.Module):
    """Sakuya_arch_test.py:247-266: ``forward_net`` over the sequence and over its reverse (the same weights),
    ``conv_1x1`` on (out_fwd[t] | out_rev[T - 1 - t]).  [B, T, 64, H, W] -> [B, T, 64, H, W], H and W multiples of 4;
    the ``ConvBLSTM.*`` slice of a LunaTokis state dict loads with ``strict=True``."""

    def __init__(self, mfma: str = "f16x3"):
        super().__init__()
        _check_choice(64, None, mfma)
        self.forward_net = DeformableConvLSTM(mfma)
        self.conv_1x1 = Conv1x1Cat(mfma)

    def forward(self, x):
        if x.dim() != 5:
            raise ValueError(f"BiDeformableConvLSTM: expected [B, T, 64, H, W], got {tuple(x.shape)}")
        _check_maps("BiDeformableConvLSTM", [x[:, 0]], "[B, T, 64, H, W]")
        B, T, C, H, W = x.shape
        fwd = self.forward_net(x)
        rev = self.forward_net(x.flip(1)).flip(1)
        out = self.conv_1x1(fwd.reshape(B * T, C, H, W), rev.reshape(B * T, C, H, W))
        return out.reshape(B, T, C, H, W)


_NOT_GEN_FEAT = ("feat_imnet.", "flow_imnet.", "encode_imnet.", "upconv1.", "upconv2.", "HRconv.", "conv_last.")


def gen_feat_state_dict(sd) -> dict:
    """The slice of a LunaTokis state dict that ``GenFeat`` loads with ``strict=True``: everything but the decoder
    and the unused upsampling layers; numpy arrays become tensors."""
    return {k: torch.as_tensor(v) for k, v in sd.items() if not k.startswith(_NOT_GEN_FEAT)}


class GenFeat(_RangeStatus, nn.Module):
    """LunaTokis.gen_feat (Sakuya_arch_test.py:313-362), everything before the decoder, trainable on the engine with
    the parameters under the reference's top-level names: frames [B, N, 3, H, W] -> features [B, 2N - 1, 64, H, W],
    H and W multiples of 4.  ``gen_feat_state_dict(sd)`` loads with ``strict=True``."""

    def __init__(self, front_RBs: int = 5, back_RBs: int = 40, mfma: str = "f16x3"):
        super().__init__()
        _check_choice(64, None, mfma)
        self.conv_first = ConvFirst()
        self.feature_extraction = make_trunk(front_RBs, 64, mfma)
        _add_pyramid(self, mfma)
        self.pcd_align = PCD_Align(mfma)
        self.fusion = Conv1x1Cat(mfma)
        self.ConvBLSTM = BiDeformableConvLSTM(mfma)
        self.recon_trunk = make_trunk(back_RBs, 64, mfma)

    def forward(self, x):
        if x.dim() != 5 or x.shape[2] != 3 or x.shape[1] < 2:
            raise ValueError(f"GenFeat: expected frames [B, N >= 2, 3, H, W], got {tuple(x.shape)}")
        B, N, _, H, W = x.shape
        if H % 4 or W % 4:
            raise ValueError(f"GenFeat: H and W must be multiples of 4 (three pyramid levels), got {H} x {W}")
        L1 = self.feature_extraction(self.conv_first(x.reshape(B * N, 3, H, W)))
        lv = [t.reshape(B, N, 64, t.shape[2], t.shape[3]) for t in (L1, *_pyramid(self, L1))]
        seq = [lv[0][:, 0]]
        for i in range(N - 1):
            a, b = self.pcd_align.branches([t[:, i] for t in lv], [t[:, i + 1] for t in lv])
            seq += [self.fusion(a, b), lv[0][:, i + 1]]
        feats = self.ConvBLSTM(torch.stack(seq, dim=1))
        T = feats.shape[1]
        return self.recon_trunk(feats.reshape(B * T, 64, H, W)).reshape(B, T, 64, H, W)


# ---- the SIREN decoder and the whole model (SIREN.py:27-79, Sakuya_arch_test.py:304-311, :364-459, :1222-1231) ----

class _SirenFn(torch.autograd.Function):
    """A whole SIREN MLP as one node over stif_siren_fwd / stif_siren_bwd.  Saved: the input matrix, the sine
    layers' pre-activations and the parameters; the backward recomputes sin and cos."""

    @staticmethod
    def forward(ctx, x, *params):
        nl = len(params) // 2
        xd = x.detach()
        y, z = ops.siren_fwd(xd, [p.detach() for p in params[:nl]], [p.detach() for p in params[nl:]])
        ctx.save_for_backward(xd, z, *params)
        return y

    @staticmethod
    def backward(ctx, g_y):
        x, z, *params = ctx.saved_tensors
        nl = len(params) // 2
        if not g_y.is_cuda:
            raise RuntimeError("Siren backward: the HIP kernels need a CUDA tensor")
        g_x, g_ws, g_bs = ops.siren_bwd(x, z, [p.detach() for p in params[:nl]], [p.detach() for p in params[nl:]],
                                        g_y.contiguous(), need_x=ctx.needs_input_grad[0])
        grads = [g if need else None for g, need in zip(g_ws + g_bs, ctx.needs_input_grad[1:])]
        return (g_x, *grads)


class _SineLayer(nn.Module):
    """SIREN.py:27-53: the parameters of one sine layer under the name ``linear``, with the reference's weight
    initialisation (first layer U(+-1 / in), others U(+-sqrt(6 / in) / 30)) and nn.Linear's default bias."""

    def __init__(self, in_features, out_features, is_first):
        super().__init__()
        self.linear = nn.Linear(in_features, out_features)
        bound = 1.0 / in_features if is_first else math.sqrt(6.0 / in_features) / 30.0
        with torch.no_grad():
            self.linear.weight.uniform_(-bound, bound)


class Siren(nn.Module):
    """SIREN.py:57-79 with ``outermost_linear=True`` and omega_0 = 30: ``hidden_features`` (64, 64, 256) or
    (64, 64, 256, 256) sine layers sin(30 (x W^T + b)) and a final nn.Linear to ``out_features`` in {64, 4, 3}, the
    parameters under the reference's names (``net.{i}.linear.weight / bias``, ``net.{last}.weight / bias``) and
    initialisation.  One autograd node on the HIP kernels (stif_siren_fwd / stif_siren_bwd, fp32 MFMA).  ``forward(x)``:
    x [..., in_features], or [..., in_features rounded up to 8] with zero pad columns as the decoder's input builders
    write it (no copy) -> [..., out_features]."""

    def __init__(self, in_features: int, hidden_features, out_features: int):
        super().__init__()
        hidden = tuple(int(h) for h in hidden_features)
        if hidden not in ops.SIREN_WIDTHS.values():
            raise ValueError(f"Siren: hidden_features must be (64, 64, 256) or (64, 64, 256, 256), got {hidden}")
        if out_features not in (64, 4, 3):
            raise ValueError(f"Siren: out_features must be 64, 4 or 3, got {out_features}")
        if not 1 <= in_features <= 528:
            raise ValueError(f"Siren: in_features must be in [1, 528], got {in_features}")
        self.in_features, self.hidden_features, self.out_features = int(in_features), hidden, int(out_features)
        dims = (self.in_features,) + hidden
        layers = [_SineLayer(dims[i], dims[i + 1], i == 0) for i in range(len(hidden))]
        last = nn.Linear(hidden[-1], out_features)
        bound = math.sqrt(6.0 / hidden[-1]) / 30.0
        with torch.no_grad():
            last.weight.uniform_(-bound, bound)
        self.net = nn.Sequential(*layers, last)

    def _params(self):
        mods = [m.linear for m in self.net[:-1]] + [self.net[-1]]
        return [m.weight for m in mods] + [m.bias for m in mods]

    def forward(self, x):
        kp = (self.in_features + 7) // 8 * 8
        if not x.is_cuda:
            raise RuntimeError(f"Siren: the HIP kernels need a CUDA tensor, got one on {x.device} "
                               "(move the module and its input to the GPU)")
        if x.dtype != torch.float32 or x.dim() < 1 or x.shape[-1] not in (self.in_features, kp) or x.numel() == 0:
            raise RuntimeError(f"Siren: expected a float32 [..., {self.in_features}] tensor (or [..., {kp}] with zero pad "
                               f"columns), got {x.dtype} {tuple(x.shape)}")
        lead = x.shape[:-1]
        x2 = x.reshape(-1, x.shape[-1])
        if x2.shape[1] != kp:
            x2 = nn.functional.pad(x2, (0, kp - x2.shape[1]))
        if x2.stride(1) != 1 or x2.stride(0) % 8 or x2.stride(0) < kp or x2.data_ptr() % 16:
            x2 = x2.contiguous()
        return _SirenFn.apply(x2, *self._params()).reshape(*lead, self.out_features)

    def extra_repr(self):
        return f"{self.in_features} -> {self.hidden_features} -> {self.out_features}, omega_0=30"


class _DecX1Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, lat, geom):
        ctx.geom = geom
        return ops.dec_x1_fwd(geom)

    @staticmethod
    def backward(ctx, g_x1):
        return ops.dec_x1_bwd(ctx.geom, g_x1.contiguous()) if ctx.needs_input_grad[0] else None, None


class _DecX2Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, hrfeat, lat, geom):
        ctx.geom = geom
        return ops.dec_x2_fwd(geom, hrfeat.detach().contiguous())

    @staticmethod
    def backward(ctx, g_x2):
        g_hr, g_lat = ops.dec_x2_bwd(ctx.geom, g_x2.contiguous())
        return g_hr if ctx.needs_input_grad[0] else None, g_lat if ctx.needs_input_grad[1] else None, None


class _DecX3Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, hrfeat, flow, lat, geom):
        hr, fl = hrfeat.detach().contiguous(), flow.detach().contiguous()
        ctx.geom = geom
        ctx.save_for_backward(hr, fl)
        return ops.dec_x3_fwd(geom, hr, fl)

    @staticmethod
    def backward(ctx, g_x3):
        hr, fl = ctx.saved_tensors
        g_flow, g_hr, g_lat = ops.dec_x3_bwd(ctx.geom, hr, fl, g_x3.contiguous(), deterministic=_DETERMINISTIC)
        need = ctx.needs_input_grad
        return g_hr if need[0] else None, g_flow if need[1] else None, g_lat if need[2] else None, None


def _hr_size(H, W, scale):
    """(HH, WW) of the decode: ``scale`` None -> x4 (Sakuya_arch_test.py:368-371); otherwise its two entries, each an
    int or a tensor as the reference's collated batches carry it (its first element is taken)."""
    if scale is None:
        return 4 * H, 4 * W
    if isinstance(scale, torch.Tensor):
        scale = scale.reshape(-1).tolist()
    if len(scale) != 2:
        raise ValueError(f"scale must be None or (HH, WW), got {scale!r}")
    return tuple(int(s.reshape(-1)[0]) if isinstance(s, torch.Tensor) else int(s) for s in scale)


def _item_times(t, B, device):
    """One entry of ``times`` -- a float, or a tensor of 1 or B elements such as the reference's [B, 1] -- as a
    float32 [B] tensor on ``device`` without a gradient."""
    if isinstance(t, torch.Tensor):
        t = t.detach().reshape(-1)
        if t.numel() not in (1, B):
            raise ValueError(f"a time query must hold 1 or {B} values, got {t.numel()}")
        return t.to(device=device, dtype=torch.float32).expand(B).contiguous()
    return torch.full((B,), float(t), dtype=torch.float32, device=device)


def _decode(who, feat_imnet, flow_imnet, encode_imnet, feat, inp, times, scale):
    """LunaTokis.decoding (Sakuya_arch_test.py:364-459): per time, X1 -> feat_imnet -> HRfeat, X2 -> flow_imnet -> flow,
    X3 -> encode_imnet -> the frame, every matrix in HBM.  Everything is refused before the first
    launch: CPU tensors, wrong shapes, HH or WW < 2."""
    if feat.dim() != 5 or feat.shape[1] != 3 or feat.shape[2] != 64:
        raise ValueError(f"{who}: expected features [B, 3, 64, H, W], got {tuple(feat.shape)}")
    B, _, _, H, W = feat.shape
    if tuple(inp.shape) != (B, 2, 3, H, W):
        raise ValueError(f"{who}: expected frames [{B}, 2, 3, {H}, {W}], got {tuple(inp.shape)}")
    HH, WW = _hr_size(H, W, scale)
    if HH < 2 or WW < 2:
        raise ValueError(f"{who}: the output must be at least 2 x 2 (the warp grid divides by n - 1), got {HH} x {WW}")
    if times is None or len(times) == 0:
        raise ValueError(f"{who}: times is a non-empty list")
    for t in (feat, inp):
        if not t.is_cuda:
            raise RuntimeError(f"{who}: the HIP kernels need a CUDA tensor, got one on {t.device} "
                               "(move the module and its input to the GPU)")
        if t.dtype != torch.float32:
            raise RuntimeError(f"{who}: expected float32 tensors, got {t.dtype}")
    tbs = [_item_times(t, B, feat.device) for t in times]
    lat = feat.reshape(B, 192, H, W).permute(0, 2, 3, 1).contiguous()      # cat(feat[:, 0..2]) (:365), NHWC
    frames = inp.detach().reshape(B, 6, H, W).contiguous()
    outs = []
    for tb in tbs:
        geom = ops.DecTrainGeom(lat.detach(), frames, tb, HH, WW)
        hrfeat = feat_imnet(_DecX1Fn.apply(lat, geom))
        flow = flow_imnet(_DecX2Fn.apply(hrfeat, lat, geom))
        pred = encode_imnet(_DecX3Fn.apply(hrfeat, flow, lat, geom))
        outs.append(pred.reshape(B, HH, WW, 3).permute(0, 3, 1, 2))
    return outs


def _make_imnets(mod):
    mod.feat_imnet = Siren(201, (64, 64, 256), 64)
    mod.flow_imnet = Siren(65 + 192 + 6, (64, 64, 256), 4)
    mod.encode_imnet = Siren(141 + 192 * 2, (64, 64, 256, 256), 3)


class Decoder(nn.Module):
    """LunaTokis.decoding (Sakuya_arch_test.py:364-459) with the three SIREN MLPs under the reference's names
    (``feat_imnet``, ``flow_imnet``, ``encode_imnet``: 26 keys), trainable on the engine.  ``forward(feat, inp, times,
    scale=None)``: feat [B, 3, 64, H, W] (gen_feat's output), inp [B, 2, 3, H, W] the LR frames, ``times`` a list of
    floats or [B, 1] tensors, ``scale`` None (x4), (HH, WW) or a pair of tensors -> a list of [B, 3, HH, WW].  One set
    of autograd nodes per time; gradients reach ``feat`` and the parameters, never ``inp`` or ``times``.  The local
    ensemble, windows, tiles, points and time fields of the inference decoder are not part of training."""

    def __init__(self):
        super().__init__()
        _make_imnets(self)

    def forward(self, feat, inp, times, scale=None):
        return _decode("Decoder", self.feat_imnet, self.flow_imnet, self.encode_imnet, feat, inp, times, scale)


class LunaTokis(GenFeat):
    """The whole model (Sakuya_arch_test.py:268-311, :1222-1231 with ``test=False``) trainable on the engine:
    ``GenFeat``'s parameters, the decoder's three SIREN MLPs and the eight keys of the reference's unused upsampling
    layers (``upconv1``, ``upconv2``, ``HRconv``, ``conv_last``), which take part in nothing and never receive a
    gradient -- 442 keys, a reference state dict loads with ``strict=True``.  ``forward(x, times, scale=None)``: frames
    x [B, 2, 3, H, W], H and W multiples of 4 -> a list of [B, 3, HH, WW], one per time."""

    def __init__(self, front_RBs: int = 5, back_RBs: int = 40, mfma: str = "f16x3"):
        super().__init__(front_RBs, back_RBs, mfma)
        self.upconv1 = _ConvParams(256, 64)
        self.upconv2 = _ConvParams(256, 64)
        self.HRconv = _ConvParams(64, 64)
        self.conv_last = _ConvParams(3, 64)
        _make_imnets(self)

    def forward(self, x, times, scale=None):
        if x.dim() != 5 or x.shape[1] != 2 or x.shape[2] != 3:
            raise ValueError(f"LunaTokis: expected frames [B, 2, 3, H, W], got {tuple(x.shape)}")
        if x.shape[3] % 4 or x.shape[4] % 4:
            raise ValueError(f"LunaTokis: H and W must be multiples of 4 (three pyramid levels), got "
                             f"{x.shape[3]} x {x.shape[4]}")
        HH, WW = _hr_size(x.shape[3], x.shape[4], scale)
        if HH < 2 or WW < 2:
            raise ValueError(f"LunaTokis: the output must be at least 2 x 2, got {HH} x {WW}")
        if times is None or len(times) == 0:
            raise ValueError("LunaTokis: times is a non-empty list")
        if not x.is_cuda:
            raise RuntimeError(f"LunaTokis: the HIP kernels need a CUDA tensor, got one on {x.device} "
                               "(move the module and its input to the GPU)")
        feat = GenFeat.forward(self, x)
        return _decode("LunaTokis", self.feat_imnet, self.flow_imnet, self.encode_imnet, feat, x, times, scale)


class TimesLoss(nn.Module):
    """VideoSR_base_model.py:126-128: the pixel criterion summed over the query times, output ``idx`` against
    ``gt[:, idx]`` -- what ``optimize_step`` needs as its criterion for a model that returns a list of frames."""

    def __init__(self, criterion):
        super().__init__()
        self.criterion = criterion

    def forward(self, outs, gt):
        return sum(self.criterion(o, gt[:, i]) for i, o in enumerate(outs))


# ---- data-parallel training: the gradient arena, the rank-ordered sum, DataParallel ----

def _named(params):
    """[(name, parameter)] of a module, of ``named_parameters()``-style pairs, or of bare parameters."""
    if isinstance(params, nn.Module):
        return list(params.named_parameters())
    out = []
    for i, p in enumerate(params):
        out.append(tuple(p) if isinstance(p, (tuple, list)) else (str(i), p))
    if not out:
        raise ValueError("GradArena: no parameters")
    return out


class GradArena:
    """One contiguous fp32 buffer for the gradients of ``params`` (a module, ``named_parameters()`` pairs or
    parameters), in that order: parameter i lives at ``offsets[i]``, the previous end rounded up to 4 floats, and
    ``total`` is the sum of the rounded sizes.  The layout is fixed here.  ``pack()`` gathers the ``.grad`` tensors into
    the arena (or into ``out``, a row of a slab) with one stif_grad_pack launch, gaps written as +0.0; ``views()`` are
    per-parameter views of the arena and ``assign()`` makes them the ``.grad``s, so that the optimiser steps on the
    reduced arena and nothing is copied back."""

    def __init__(self, params):
        named = _named(params)
        self.names, self.params = [k for k, _ in named], [p for _, p in named]
        dev = self.params[0].device
        for k, p in named:
            if p.dtype != torch.float32 or p.device != dev:
                raise ValueError(f"GradArena: {k} is {p.dtype} on {p.device}; float32 parameters on one device only")
        self.table = ops.GradTable([p.numel() for p in self.params], dev)
        self.sizes, self.offsets, self.total = list(self.table.sizes), list(self.table.offsets), self.table.floats
        self.arena = torch.zeros(max(self.total, 4), dtype=torch.float32, device=dev)
        self._views = None

    def grads(self):
        missing = [k for k, p in zip(self.names, self.params) if p.grad is None]
        if missing:
            raise RuntimeError(f"{len(missing)} covered parameter(s) received no gradient in this backward: "
                               + ", ".join(missing[:8]) + (" ..." if len(missing) > 8 else ""))
        return [p.grad for p in self.params]

    def pack(self, out: torch.Tensor = None) -> torch.Tensor:
        out = self.arena if out is None else out
        self.table = ops.grad_pack(self.grads(), out, self.table)
        return out

    def views(self):
        """Per-parameter views of the arena, made once: the same tensors are handed out every step."""
        if self._views is None:
            self._views = [self.arena[o:o + n].view_as(p) for o, n, p in zip(self.offsets, self.sizes, self.params)]
        return self._views

    def assign(self):
        for p, v in zip(self.params, self.views()):
            p.grad = v


def _covered(net: nn.Module):
    """The parameters that received a gradient in the backward just run, as named_parameters() pairs."""
    return [(k, p) for k, p in net.named_parameters() if p.grad is not None]


def _staged(group) -> bool:
    """parallel.halo_exchange's backend rule: gloo moves CPU tensors, so device buffers are staged through (pinned)
    host memory -- which is what lets several ranks share one GPU; nccl takes the device buffers as they are."""
    return dist.get_backend(group) == "gloo"


def _small_gather(values, group, device) -> torch.Tensor:
    """One small collective: every rank's int64 ``values`` as a CPU [world, len(values)] tensor."""
    world = dist.get_world_size(group)
    dev = "cpu" if _staged(group) else device
    mine = torch.tensor(list(values), dtype=torch.int64, device=dev)
    rows = [torch.empty_like(mine) for _ in range(world)]
    dist.all_gather(rows, mine, group=group)
    return torch.stack(rows).cpu()


def _names_hash(names) -> int:
    import hashlib
    return int.from_bytes(hashlib.sha256("\n".join(names).encode()).digest()[:8], "little", signed=True)


def check_covered_set(covered, every, group=None, device="cpu") -> None:
    """The first step's agreement on which parameters the arena covers: one small collective compares a hash of the
    covered names over the ranks.  On a mismatch -- seen by every rank alike, so all of them leave together instead of
    hanging in an exchange of different sizes -- the ranks trade the names they leave out and RuntimeError lists
    them."""
    hashes = _small_gather([_names_hash(covered)], group, device)[:, 0].tolist()
    if len(set(hashes)) == 1:
        return
    left_out = sorted(set(every) - set(covered))
    per_rank = [None] * dist.get_world_size(group)
    dist.all_gather_object(per_rank, left_out, group=group)
    common = set.intersection(*[set(x) for x in per_rank])
    odd = [f"rank {r}: " + (", ".join(k for k in x if k not in common) or "-") for r, x in enumerate(per_rank)]
    raise RuntimeError("DataParallel: the ranks disagree on which parameters received a gradient in the first "
                       "backward; without a gradient only on " + "; ".join(odd))


class DataParallel:
    """Data-parallel optimiser steps with sum semantics: every rank runs forward and backward
    on its own items of the global batch, the gradients are summed over ranks -- never averaged, the reference's loss is
    a sum -- and every rank takes the optimiser step one process would take on the whole batch, up to fp32
    reassociation.  The gradients cross as one arena in one collective:

    * ``reduce="sum"``: one ``dist.all_reduce(SUM)`` on the arena (the backend's order of addition);
    * ``reduce="ordered"``: ``all_gather`` into a [world, N] slab, then stif_rank_sum, ((g0 + g1) + g2) + ... by rank
      on every rank: replicas stay bitwise identical, a run is the same under gloo and RCCL, and ``emulate_ranks``
      reproduces it in one process;
    * ``reduce=None`` (default): "ordered" while ``is_deterministic()``, "sum" otherwise, read at every step.

    At construction rank 0's parameters and buffers are broadcast.  The arena covers exactly the parameters that
    received a gradient in the first backward (434 of LunaTokis' 442); the ranks compare a hash of that set once
    (``check_covered_set``), and a covered parameter without a gradient on a later step raises.  With the gloo backend
    the arena is staged through pinned host memory; with nccl the device buffers go unstaged and
    ``parallel.warm_group`` runs first.  ``world == 1`` needs no process group.  ``step`` forces no host
    synchronisation of its own (gloo's staging waits for the copy); ``global_loss()`` and ``range_status()`` are the
    reads, for ``print_freq``."""

    def __init__(self, net: nn.Module, optimizer, group=None, reduce=None):
        if reduce not in (None, "sum", "ordered"):
            raise ValueError(f"reduce must be 'sum', 'ordered' or None, got {reduce!r}")
        self.net, self.optimizer, self.group, self.reduce = net, optimizer, group, reduce
        self.distributed = dist.is_available() and dist.is_initialized()
        self.world = dist.get_world_size(group) if self.distributed else 1
        self.rank = dist.get_rank(group) if self.distributed else 0
        self.arena = self._slab = self._host = self._host_slab = self._loss = None
        if self.world > 1:
            if self.world > L.RANK_SUM_MAX_RANKS:
                raise ValueError(f"DataParallel: at most {L.RANK_SUM_MAX_RANKS} ranks, got {self.world}")
            if not _staged(group):
                from . import parallel
                parallel.warm_group(group)
            self._broadcast()

    def _broadcast(self):
        stage = _staged(self.group)
        src = dist.get_global_rank(self.group, 0) if self.group is not None else 0
        with torch.no_grad():
            for t in list(self.net.parameters()) + list(self.net.buffers()):
                buf = t.detach().cpu() if stage else t.detach()
                dist.broadcast(buf, src, group=self.group)
                if stage and self.rank != 0:
                    t.copy_(buf)

    def _first_backward(self):
        named = _covered(self.net)
        if not named:
            raise RuntimeError("DataParallel: no parameter received a gradient")
        if self.world > 1:
            check_covered_set([k for k, _ in named], [k for k, _ in self.net.named_parameters()], self.group,
                              named[0][1].device)
        self.arena = GradArena(named)
        covered = {id(p) for p in self.arena.params}
        self._outside = [(k, p) for k, p in self.net.named_parameters() if id(p) not in covered]

    def _mode(self):
        return self.reduce or ("ordered" if is_deterministic() else "sum")

    def _reduce(self):
        a, N = self.arena.arena, self.arena.arena.numel()
        stage, mode = _staged(self.group), self._mode()
        if stage and self._host is None:
            self._host = torch.empty(N, dtype=torch.float32, pin_memory=a.is_cuda)
        if mode == "sum":
            if not stage:
                dist.all_reduce(a, op=dist.ReduceOp.SUM, group=self.group)
                return
            self._host.copy_(a, non_blocking=True)
            _wait(a)
            dist.all_reduce(self._host, op=dist.ReduceOp.SUM, group=self.group)
            a.copy_(self._host, non_blocking=True)
            return
        if self._slab is None:
            self._slab = torch.empty(self.world, N, dtype=torch.float32, device=a.device)
        if not stage:
            dist.all_gather_into_tensor(self._slab, a, group=self.group)
        else:
            if self._host_slab is None:
                self._host_slab = torch.empty(self.world, N, dtype=torch.float32, pin_memory=a.is_cuda)
            self._host.copy_(a, non_blocking=True)
            _wait(a)
            dist.all_gather(list(self._host_slab.unbind(0)), self._host, group=self.group)
            self._slab.copy_(self._host_slab, non_blocking=True)
        ops.rank_sum(self._slab, a)

    def step(self, criterion, inputs, gt, weight: float = 1.0) -> torch.Tensor:
        """optimize_step for this rank's items of the global batch: zero_grad(set_to_none=True), forward,
        ``weight * criterion``, backward, pack, reduce over the ranks, the arena's views as ``.grad``,
        ``optimizer.step()``.  Returns this rank's loss as a device tensor."""
        self.optimizer.zero_grad(set_to_none=True)
        loss = weight * criterion(self.net(*inputs), gt)
        loss.backward()
        if self.arena is None:
            self._first_backward()
        else:
            late = [k for k, p in self._outside if p.grad is not None]
            if late:
                raise RuntimeError("DataParallel: parameter(s) outside the arena received a gradient (the covered set "
                                   "is fixed by the first backward): " + ", ".join(late[:8]))
        self.arena.pack()
        if self.world > 1:
            self._reduce()
        self.arena.assign()
        self.optimizer.step()
        self._loss = loss.detach()
        return self._loss

    def global_loss(self) -> float:
        """The last step's loss summed over the ranks in rank order (fp32); one synchronisation and, with several
        ranks, one small collective."""
        if self._loss is None:
            raise RuntimeError("DataParallel.global_loss: no step taken yet")
        mine = self._loss.reshape(1).to(torch.float32)
        if self.world == 1:
            return float(mine)
        dev = "cpu" if _staged(self.group) else mine.device
        rows = [torch.empty(1, dtype=torch.float32, device=dev) for _ in range(self.world)]
        dist.all_gather(rows, mine.to(dev), group=self.group)
        total = rows[0].cpu()
        for r in rows[1:]:
            total = total + r.cpu()
        return float(total)

    def range_status(self) -> int:
        """``train.range_status`` of this rank's device, ORed over the ranks."""
        dev = next(self.net.parameters()).device
        bits = range_status(dev)
        if self.world > 1:
            for b in _small_gather([bits], self.group, dev)[:, 0].tolist():
                bits |= int(b)
        return bits

    def replicas_agree(self) -> bool:
        """One small collective: an exact integer checksum of every parameter's bits, compared over the ranks."""
        if self.world == 1:
            return True
        dev = next(self.net.parameters()).device
        total = torch.zeros((), dtype=torch.int64, device=dev)
        for i, p in enumerate(self.net.parameters()):
            total += p.detach().reshape(-1).view(torch.int32).to(torch.int64).sum() * (2 * i + 1)
        sums = _small_gather([int(total)], self.group, dev)[:, 0].tolist()
        return len(set(sums)) == 1


def _wait(t: torch.Tensor) -> None:
    """A host collective reads the staging buffer next: wait for the copies queued on ``t``'s stream."""
    if t.is_cuda:
        torch.cuda.current_stream(t.device).synchronize()


def emulate_ranks(net: nn.Module, optimizer, criterion, per_rank_batches, weight: float = 1.0) -> torch.Tensor:
    """The definition ``DataParallel`` with the ordered sum is held to, in one process: from the same state, each
    ``(inputs, gt)`` of ``per_rank_batches`` in turn takes rank r's forward and backward and is packed into row r of a
    slab; stif_rank_sum adds the rows in rank order, the arena's views become the ``.grad``s and the optimiser takes
    one step.  Also "accumulate over micro-batches" on one GPU.  Returns the losses summed in rank order (a device
    tensor, fp32).  The arena and the slab are kept on the optimiser (``optimizer.emulated_arena``, a ``GradArena``)
    for the next call with as many batches."""
    batches = list(per_rank_batches)
    R = len(batches)
    if not 1 <= R <= L.RANK_SUM_MAX_RANKS:
        raise ValueError(f"emulate_ranks: 1 .. {L.RANK_SUM_MAX_RANKS} batches, got {R}")
    total = arena = slab = None
    for r, (inputs, gt) in enumerate(batches):
        optimizer.zero_grad(set_to_none=True)
        loss = weight * criterion(net(*inputs), gt)
        loss.backward()
        if r == 0:
            named = _covered(net)
            arena, slab = getattr(optimizer, "emulated_arena", None), getattr(optimizer, "emulated_slab", None)
            if arena is None or arena.names != [k for k, _ in named] or slab.shape[0] != R:
                arena = optimizer.emulated_arena = GradArena(named)
                slab = optimizer.emulated_slab = torch.empty(R, arena.arena.numel(), dtype=torch.float32,
                                                             device=arena.arena.device)
        arena.pack(slab[r])
        total = loss.detach() if total is None else total + loss.detach()
    ops.rank_sum(slab, arena.arena)
    arena.assign()
    optimizer.step()
    return total
