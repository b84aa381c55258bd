"""Time the on-device PSNR / SSIM metric (stif_metric_psnr_ssim, Y + SSIM) per 2160x3840 frame for n = 1 and
n = 8, against the same metric composed from torch ops on the same GPU (quantise, luma, float64 F.conv2d with the
11-tap window as a 1x11 then an 11x1 kernel -- and, for n = 1, the reference's literal 11x11 form), alternating
the arms.  HIP events around warmed-up loops; prints microseconds per frame, achieved bytes/s against the
algorithmic 15 B per pixel (12 B of prediction + 3 B of ground truth) and the two floors.

  python tools/bench_metrics.py [--iters 20] [--small]      (--small: 270x480, a rehearsal size)

--float times the float protocol instead (stif_metric_float, volume mode: calc_psnr + ssim_matlab) against the
same sums composed from torch float64 F.pad + F.conv3d, with the Y + SSIM call beside it as the per-plane yardstick.

  python tools/bench_metrics.py --float [--literal] [--iters 20] [--small]
"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import stif_pkg  # noqa: E402

HBM_MEASURED, HBM_SPEC = 6.29e12, 8.0e12     # B/s (float4 copy / datasheet)
FP64_VECTOR = 157.3e12 / 2                   # FLOP/s: the fp64 vector rate is half the fp32 vector rate (datasheet 78.6 TF)
# fp64 FMAs per pixel the separable algorithm needs with no halo recomputation: horizontal pass 2 x 11 (a, b)
# + 3 x 11 (a^2, b^2, ab) + 3 products, vertical pass 5 x 11
FMA_PER_PIXEL = 2 * 11 + 3 * 11 + 3 + 5 * 11


def timed(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters      # us per call


def torch_metric(pred, gt, k, separable=True):
    """the same sums from torch ops: (sse, ssim_sum) per item, float64"""
    q = torch.round(pred.clamp(0, 1) * 255.0).double()
    g = gt.double()
    a = ((24.966 * q[:, 2] + 128.553 * q[:, 1] + 65.481 * q[:, 0]) / 255.0 + 16.0)[:, None]
    b = ((24.966 * g[..., 0] + 128.553 * g[..., 1] + 65.481 * g[..., 2]) / 255.0 + 16.0)[:, None]
    sse = ((a - b) ** 2).sum((1, 2, 3))
    x = torch.cat([a, b, a * a, b * b, a * b], 0)
    if separable:
        f = F.conv2d(F.conv2d(x, k.view(1, 1, 1, 11)), k.view(1, 1, 11, 1))
    else:
        f = F.conv2d(x, torch.outer(k, k).view(1, 1, 11, 11))
    mu1, mu2, eaa, ebb, eab = f.chunk(5, 0)
    s1, s2, s12 = eaa - mu1 * mu1, ebb - mu2 * mu2, eab - mu1 * mu2
    m = ((2 * mu1 * mu2 + 6.5025) * (2 * s12 + 58.5225)) / ((mu1 * mu1 + mu2 * mu2 + 6.5025) * (s1 + s2 + 58.5225))
    return sse, m.sum((1, 2, 3))


def torch_float_metric(pred, ref, k, literal=False):
    """stif_metric_float's volume-mode sums from torch ops, one item at a time (the padded float64 volumes of
    eight 2160x3840 frames at once are tens of GB): (sse, ssim_sum) per item.  F.pad replicates 5 on all three
    axes; the window is three 11-tap F.conv3d passes, or with `literal` the reference's one 11x11x11 kernel."""
    sse, ssum = [], []
    for p, r in zip(pred, ref):
        d = p.double() - r.double()
        sse.append((d * d).sum())
        a, b = p.clamp(0, 1).double(), r.clamp(0, 1).double()
        x = F.pad(torch.stack([a, b, a * a, b * b, a * b])[:, None], (5,) * 6, mode="replicate")
        if literal:
            f = F.conv3d(x, torch.einsum("i,j,l->ijl", k, k, k).view(1, 1, 11, 11, 11))
        else:
            f = F.conv3d(F.conv3d(F.conv3d(x, k.view(1, 1, 11, 1, 1)), k.view(1, 1, 1, 11, 1)), k.view(1, 1, 1, 1, 11))
        mu1, mu2, eaa, ebb, eab = f.unbind(0)
        s1, s2, s12 = eaa - mu1 * mu1, ebb - mu2 * mu2, eab - mu1 * mu2
        m = ((2 * mu1 * mu2 + 1e-4) * (2 * s12 + 9e-4)) / ((mu1 * mu1 + mu2 * mu2 + 1e-4) * (s1 + s2 + 9e-4))
        ssum.append(m.sum())
    return torch.stack(sse), torch.stack(ssum)


def float_rows(opt, stif, H, W):
    """--float: stif_metric_float (volume mode) per frame for n = 1 and n = 8 against torch_float_metric and, as
    the per-plane yardstick, the Y + SSIM call of stif_metric_psnr_ssim on frames of the same size (one scored
    plane per frame there, three here), alternating the arms."""
    M, L, lib = stif.metrics, stif._lib, stif._lib.lib()
    k = torch.from_numpy(M.window()).cuda()
    px = H * W
    fma = 3 * (FMA_PER_PIXEL + 5 * 3)          # per pixel of a frame: three channels, each with the 3 x 3 mix of five fields
    print(f"frame {H}x{W}, float protocol (calc_psnr + ssim_matlab); floors per frame: HBM "
          f"{24 * px / HBM_MEASURED * 1e6:.1f} us at the measured {HBM_MEASURED / 1e12:.2f} TB/s for the algorithmic "
          f"24 B per pixel, fp64 {2 * fma * px / FP64_VECTOR * 1e6:.1f} us ({fma} FMA per pixel at "
          f"{FP64_VECTOR / 1e12:.1f} TFLOP/s)")
    gen = torch.Generator(device="cuda").manual_seed(0)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for n in (1, 8):
        pred = torch.rand(n, 3, H, W, device="cuda", generator=gen) * 1.2 - 0.1
        ref = torch.rand(n, 3, H, W, device="cuda", generator=gen) * 1.2 - 0.1
        gt = torch.randint(0, 256, (n, H, W, 3), device="cuda", dtype=torch.uint8, generator=gen)
        out = M.sums_float(pred, ref)
        a = L.MetricArgs()
        a.pred, a.gt_f32, a.gt_u8, a.n, a.H, a.W = pred.data_ptr(), ref.data_ptr(), gt.data_ptr(), n, H, W
        nbytes = lib.stif_metric_float_workspace_size(n, H, W, L.FSSIM_VOLUME)
        ws = torch.empty(nbytes // 8, device="cuda", dtype=torch.float64)
        out2 = torch.empty(n, 4, device="cuda", dtype=torch.float64)
        ay = L.MetricArgs()
        ay.pred, ay.gt_u8, ay.n, ay.H, ay.W, ay.flags = pred.data_ptr(), gt.data_ptr(), n, H, W, M.mode_flags("y", True)
        nbytes_y = lib.stif_metric_workspace_size(n, H, W, ay.flags)
        ws_y = torch.empty(nbytes_y // 8, device="cuda", dtype=torch.float64)
        out_y = torch.empty(n, 4, device="cuda", dtype=torch.float64)

        def call():
            L.check(lib.stif_metric_float(ctypes.byref(a), L.FSSIM_VOLUME, out2.data_ptr(), ws.data_ptr(), nbytes, st),
                    "metric_float")

        def call_y():
            L.check(lib.stif_metric_psnr_ssim(ctypes.byref(ay), out_y.data_ptr(), ws_y.data_ptr(), nbytes_y, st), "metric")

        call()
        assert out2.cpu().numpy().tobytes() == out.cpu().numpy().tobytes()
        us_k = timed(call, opt.iters)
        us_y = timed(call_y, opt.iters)
        us_k2 = timed(call, opt.iters)
        us_y2 = timed(call_y, opt.iters)
        best, best_y = min(us_k, us_k2), min(us_y, us_y2)
        print(f"n={n}: stif_metric_float {us_k / n:9.1f} / {us_k2 / n:9.1f} us per frame ({best / n / 3:8.1f} us per scored "
              f"plane, {24 * px * n / best / 1e3:7.1f} GB/s of the algorithmic bytes)   Y + SSIM {us_y / n:9.1f} / "
              f"{us_y2 / n:9.1f} us per frame = per scored plane   per-plane ratio {best / 3 / best_y:5.2f}x")
        for literal in (False, True):
            if literal and not (opt.literal and n == 1):
                continue
            name = "torch F.pad + F.conv3d 11x11x11" if literal else "torch F.pad + three 11-tap F.conv3d"
            try:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                sse, ssum = torch_float_metric(pred, ref, k, literal)
                o = out.cpu().numpy()
                err = max(float(np.abs(sse.cpu().numpy() / o[:, 0] - 1).max()),
                          float(np.abs(ssum.cpu().numpy() / o[:, 2] - 1).max()))
                first = time.perf_counter() - t0       # the read-back synchronises; bounds the timed window to ~20 s
                us_t = timed(lambda: torch_float_metric(pred, ref, k, literal),
                             max(1, min(opt.iters // 4, int(20.0 / first))), warmup=1)
                us_k3 = timed(call, opt.iters)
                print(f"n={n}: {name}: {us_t / n:11.1f} us per frame   kernel again {us_k3 / n:9.1f}   ratio "
                      f"{us_t / min(best, us_k3):7.1f}x   max relative difference of the sums {err:.1e}")
            except RuntimeError as e:      # e.g. no float64 convolution in this build
                print(f"n={n}: {name} not available: {str(e).splitlines()[0]}")
        del pred, ref, gt
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--float", action="store_true", help="the float protocol (stif_metric_float, volume mode) instead")
    ap.add_argument("--literal", action="store_true", help="with --float: also time the 11x11x11 F.conv3d for n = 1")
    opt = ap.parse_args()
    assert torch.cuda.is_available(), "bench_metrics needs the GPU"
    stif = stif_pkg.load()
    M = stif.metrics
    H, W = (270, 480) if opt.small else (2160, 3840)
    if opt.float:
        return float_rows(opt, stif, H, W)
    flags = M.mode_flags("y", True)
    k = torch.from_numpy(M.window()).cuda()
    px = H * W
    print(f"frame {H}x{W}, Y + SSIM; floors per frame: HBM {15 * px / HBM_MEASURED * 1e6:.1f} us at the measured "
          f"{HBM_MEASURED / 1e12:.2f} TB/s ({15 * px / HBM_SPEC * 1e6:.1f} us at the {HBM_SPEC / 1e12:.1f} TB/s spec), "
          f"fp64 {2 * FMA_PER_PIXEL * px / FP64_VECTOR * 1e6:.1f} us ({FMA_PER_PIXEL} FMA per pixel at "
          f"{FP64_VECTOR / 1e12:.1f} TFLOP/s)")
    gen = torch.Generator(device="cuda").manual_seed(0)
    for n in (1, 8):
        pred = torch.rand(n, 3, H, W, device="cuda", generator=gen) * 1.2 - 0.1
        gt = torch.randint(0, 256, (n, H, W, 3), device="cuda", dtype=torch.uint8, generator=gen)
        out = M.sums(pred, gt, flags)
        # the timed arm is the C-ABI call alone (arguments, workspace and output set up once)
        L, lib = stif._lib, stif._lib.lib()
        a = L.MetricArgs()
        a.pred, a.gt_u8, a.n, a.H, a.W, a.flags = pred.data_ptr(), gt.data_ptr(), n, H, W, flags
        nbytes = lib.stif_metric_workspace_size(n, H, W, flags)
        ws = torch.empty(nbytes // 8, device="cuda", dtype=torch.float64)
        out2 = torch.empty(n, 4, device="cuda", dtype=torch.float64)
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

        def call():
            L.check(lib.stif_metric_psnr_ssim(ctypes.byref(a), out2.data_ptr(), ws.data_ptr(), nbytes, st), "metric")

        call()
        assert out2.cpu().numpy().tobytes() == out.cpu().numpy().tobytes()
        for sep in (True, False):
            if not sep and n > 1:
                continue
            name = "torch separable 1x11, 11x1" if sep else "torch 11x11"
            try:
                sse, ssum = torch_metric(pred, gt, k, sep)
                o = out.cpu().numpy()
                err = max(float(np.abs(sse.cpu().numpy() / o[:, 0] - 1).max()),
                          float(np.abs(ssum.cpu().numpy() / o[:, 2] - 1).max()))
                us_k = timed(call, opt.iters)
                us_t = timed(lambda: torch_metric(pred, gt, k, sep), max(2, opt.iters // 4), warmup=1)
                us_k2 = timed(call, opt.iters)
                print(f"n={n}: kernel {us_k / n:9.1f} / {us_k2 / n:9.1f} us per frame "
                      f"({15 * px * n / min(us_k, us_k2) / 1e3:7.1f} GB/s of the algorithmic bytes)   {name}: {us_t / n:11.1f} us "
                      f"per frame   ratio {us_t / min(us_k, us_k2):7.1f}x   max relative difference of the sums {err:.1e}")
            except RuntimeError as e:      # e.g. no float64 convolution in this build
                print(f"n={n}: {name} not available: {str(e).splitlines()[0]}")
        del pred, gt
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
