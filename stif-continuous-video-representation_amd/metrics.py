"""PSNR / SSIM of decoded frames against ground truth, computed on the device.

The reference scores on the host (myutils.test_metric_adobe_liif4x, myutils.py:1151-1174): every output frame is
quantised by ``utils.util.tensor2img`` (``round(clamp(o, 0, 1) * 255)`` in fp32, half to even), reduced to the Y
channel by ``data.util.bgr2ycbcr`` and compared by ``utils.util.calculate_psnr`` / ``ssim`` (util.py:140-174:
11 x 11 Gaussian, sigma 1.5, fp64, windows inside the image only).  ``psnr_ssim`` is that computation in one
streaming pass of ``stif_metric_psnr_ssim`` over frames already in HBM; ``channels="rgb"`` is the reference's
three-channel alternative and ``psnr_float`` is ``myutils.calc_psnr`` (:269-271).  ``eval_metrics`` is the float
protocol of ``myutils.eval_metrics`` (:234-241) through ``stif_metric_float``: ``calc_psnr`` beside
``ssim_matlab`` (:105-158), the volumetric SSIM of the clamped RGB frame, defined here with the fp64 window (the
reference's is fp32; the recorded gap is in DESIGN.md section 3f).

One difference from the reference, on purpose: the reference turns the ground truth into ``uint8 / 255`` in fp32
and casts its luma back to fp32, so its GT carries fp32 rounding noise.  Here the metric is defined on the
ground truth's exact integers; the two agree to ~3e-7 dB and ~4e-9 SSIM.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L


def window() -> np.ndarray:
    """The normalised 11-tap window the kernel uses (cv2.getGaussianKernel(11, 1.5)); no GPU needed."""
    k = (C.c_double * 11)()
    L.check(L.lib().stif_metric_window(k), "stif_metric_window")
    return np.array(k, dtype=np.float64)


def finish(out4, float_mode: bool = False):
    """Host arithmetic on the kernel's sums: out4 [n, 4] = (sse, npix, ssim_sum, nwin) per item ->
    (psnr [n], ssim [n]) float64.  Quantised modes: 20 log10(255 / sqrt(mse)), inf at zero MSE
    (calculate_psnr); float mode: -10 log10(mse + 1e-8) (calc_psnr).  SSIM is NaN where no window fits
    (nwin == 0: H < 11 or W < 11, or SSIM not requested), as numpy's mean of an empty map."""
    o = np.asarray(out4, dtype=np.float64).reshape(-1, 4)
    mse = o[:, 0] / o[:, 1]
    with np.errstate(divide="ignore", invalid="ignore"):
        if float_mode:
            psnr = -10.0 * np.log10(mse + 1e-8)
        else:
            psnr = np.where(mse == 0, np.inf, 20.0 * np.log10(255.0 / np.sqrt(mse)))
        ssim = np.where(o[:, 3] > 0, o[:, 2] / o[:, 3], np.nan)
    return psnr, ssim


def _shape4(t, what):
    """[n, 3, H, W] (or [3, H, W]) float32 view with a contiguous last dimension, on any device"""
    import torch
    if t.dim() == 3:
        t = t[None]
    if t.dim() != 4 or t.shape[1] != 3:
        raise ValueError(f"{what} must be [n, 3, H, W]")
    if t.dtype != torch.float32:
        t = t.float()
    if t.shape[-1] > 1 and t.stride(-1) != 1:
        raise ValueError(f"{what}: the last dimension must be contiguous")
    return t


def _planes(t, what):
    """[n, 3, H, W] float32 device view with a contiguous last dimension -> the tensor (no copy for fp32)."""
    t = _shape4(t, what)
    if not t.is_cuda:
        raise ValueError(f"{what} must be on the GPU")
    return t


def sums(pred, gt, flags: int):
    """One stif_metric_psnr_ssim call: the raw [n, 4] float64 sums as a device tensor (no synchronisation).
    pred: [n, 3, H, W] float on the device, any strided view whose rows are contiguous (strides are passed
    through, nothing is copied).  gt: [n, H, W, 3] uint8 BGR (torch or numpy), or with L.METRIC_FLOAT a float
    [n, 3, H, W]; moved to pred's device."""
    import torch
    p = _planes(pred, "pred")
    n, _, H, W = p.shape
    a = L.MetricArgs()
    a.pred = p.data_ptr()
    a.pred_item, a.pred_plane, a.pred_pitch = p.stride(0), p.stride(1), p.stride(2)
    if n == 1:
        a.pred_item = 3 * max(p.stride(1), 1)     # one item: its stride is never used
    if flags & L.METRIC_FLOAT:
        g = _planes(torch.as_tensor(gt).to(p.device), "ref")
        if tuple(g.shape) != tuple(p.shape):
            raise ValueError(f"ref {tuple(g.shape)} does not match pred {tuple(p.shape)}")
        a.gt_f32 = g.data_ptr()
        a.gtf_item, a.gtf_plane, a.gtf_pitch = g.stride(0), g.stride(1), g.stride(2)
        if n == 1:
            a.gtf_item = 3 * max(g.stride(1), 1)
    else:
        g = torch.as_tensor(gt)
        if g.dim() == 3:
            g = g[None]
        if g.dtype != torch.uint8 or tuple(g.shape) != (n, H, W, 3):
            raise ValueError(f"gt must be uint8 [n, H, W, 3] = {(n, H, W, 3)} (BGR, as cv2.imread); got "
                             f"{g.dtype} {tuple(g.shape)}")
        g = g.to(p.device).contiguous()
        a.gt_u8 = g.data_ptr()
    a.n, a.H, a.W, a.flags = n, H, W, flags
    lib = L.lib()
    nbytes = lib.stif_metric_workspace_size(n, H, W, flags)
    ws = torch.empty(max(nbytes, 8) // 8, device=p.device, dtype=torch.float64)
    out = torch.empty(n, 4, device=p.device, dtype=torch.float64)
    with torch.cuda.device(p.device):
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        L.check(lib.stif_metric_psnr_ssim(C.byref(a), out.data_ptr(), ws.data_ptr(), nbytes, st),
                "stif_metric_psnr_ssim")
    return out


def mode_flags(channels: str = "y", ssim: bool = True) -> int:
    if channels not in ("y", "rgb"):
        raise ValueError('channels must be "y" or "rgb"')
    return (L.METRIC_Y if channels == "y" else 0) | (L.METRIC_SSIM if ssim else 0)


def psnr_ssim(pred, gt, channels: str = "y", ssim: bool = True):
    """(psnr [n], ssim [n]) float64 numpy of pred [n, 3, H, W] (device float, RGB, unclamped) against
    gt [n, H, W, 3] uint8 BGR: one launch pair and a read-back of 4 n doubles.  ssim=False: PSNR only (SSIM NaN)."""
    return finish(sums(pred, gt, mode_flags(channels, ssim)).cpu().numpy())


def psnr_float(pred, ref):
    """myutils.calc_psnr per item: -10 log10(mean((pred - ref)^2) + 1e-8) of unquantised floats [n, 3, H, W]."""
    return finish(sums(pred, ref, L.METRIC_FLOAT).cpu().numpy(), float_mode=True)[0]


def sums_float(pred, ref, volume: bool = True):
    """One stif_metric_float call: the raw [n, 4] float64 sums (sse, 3HW, ssim_sum, 3HW) as a device tensor (no
    synchronisation).  pred, ref: [n, 3, H, W] float RGB, unclamped; pred on the device, ref moved to it; strided
    views with contiguous rows are passed through without a copy.  volume=True: myutils.ssim_matlab's 11 x 11 x 11
    window over (channel, row, column); False: myutils.ssim's 11 x 11 window per channel."""
    import torch
    p, g = _shape4(pred, "pred"), _shape4(torch.as_tensor(ref), "ref")
    if tuple(g.shape) != tuple(p.shape):
        raise ValueError(f"ref {tuple(g.shape)} does not match pred {tuple(p.shape)}")
    n, _, H, W = p.shape
    if H < 11 or W < 11:
        raise ValueError(f"{H}x{W} is smaller than the 11 x 11 window: the reference's shrinking window for "
                         "small images is not reproduced")
    if not p.is_cuda:
        raise ValueError("pred must be on the GPU")
    g = g.to(p.device)
    a = L.MetricArgs()
    a.pred, a.gt_f32 = p.data_ptr(), g.data_ptr()
    a.pred_item, a.pred_plane, a.pred_pitch = p.stride(0), p.stride(1), p.stride(2)
    a.gtf_item, a.gtf_plane, a.gtf_pitch = g.stride(0), g.stride(1), g.stride(2)
    if n == 1:                                    # one item: its stride is never used
        a.pred_item, a.gtf_item = 3 * max(p.stride(1), 1), 3 * max(g.stride(1), 1)
    a.n, a.H, a.W, a.flags = n, H, W, L.METRIC_FLOAT
    mode = L.FSSIM_VOLUME if volume else L.FSSIM_PLANAR
    lib = L.lib()
    nbytes = lib.stif_metric_float_workspace_size(n, H, W, mode)
    ws = torch.empty(max(nbytes, 8) // 8, device=p.device, dtype=torch.float64)
    out = torch.empty(n, 4, device=p.device, dtype=torch.float64)
    with torch.cuda.device(p.device):
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        L.check(lib.stif_metric_float(C.byref(a), mode, out.data_ptr(), ws.data_ptr(), nbytes, st),
                "stif_metric_float")
    return out


def eval_metrics(pred, ref, volume: bool = True):
    """myutils.eval_metrics per item (:234-241), (psnr [n], ssim [n]) float64 numpy: calc_psnr of the unclamped
    floats beside ssim_matlab of the frames clamped to [0, 1] (volume=False: myutils.ssim instead), in one launch
    pair and a read-back of 4 n doubles."""
    return finish(sums_float(pred, ref, volume).cpu().numpy(), float_mode=True)


def ssim_float(pred, ref, volume: bool = True):
    """The SSIM half of eval_metrics: ssim [n]."""
    return eval_metrics(pred, ref, volume)[1]
