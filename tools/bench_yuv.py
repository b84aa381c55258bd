"""Time the two video I/O kernels and the streaming renderer.

Kernels: stif_yuv_to_rgb and stif_rgb_to_yuv at 1920x1080 4:2:0, 8-bit and 10-bit, n = 8 frames, HIP events around
warmed-up loops, the median of repeated loops; achieved GB/s against the algorithmic bytes (every sample and
every fp32 value moved once: 12 B/px of fp32 + 1.5 samples/px).  stif_frames_to_u8 on the same pixel count, in the
same run, stands beside rgb_to_yuv: both read 12 B/px of fp32; a zero fill of the fp32 frames stands beside
yuv_to_rgb, which writes the same 12 B/px.

Streaming: ms per output frame of video.render_stream(chunk_pairs=6) against video.run_sequence on the 7 x 128 x
128 window, x4 size, x8 frame rate (the streamed run renders the window's 48 frames plus the closing t = 1 frame).

  python tools/bench_yuv.py [--iters 20] [--reps 7] [--small] [--no-stream]     (--small: 480x270, a rehearsal size)
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import stif_pkg  # noqa: E402

HBM_MEASURED = 6.29e12     # B/s, float4 copy (tools/bench_metrics.py)


def timed(fn, iters, reps, warmup=3):
    """median over `reps` loops of `iters` calls: microseconds per call"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / iters)
    return statistics.median(out), min(out), max(out)


def bench_kernels(stif, W, H, n, iters, reps):
    L, lib, ops = stif._lib, stif._lib.lib(), stif.ops
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    gen = torch.Generator(device="cuda").manual_seed(0)
    px = W * H * n
    rgb = torch.rand(n, 3, H, W, device="cuda", generator=gen) * 1.2 - 0.1
    u8 = torch.empty(n, H, W, 3, device="cuda", dtype=torch.uint8)

    def to_u8():
        L.check(lib.stif_frames_to_u8(rgb.data_ptr(), u8.data_ptr(), n, H, W, st), "stif_frames_to_u8")

    print(f"{n} frames of {W}x{H}, 4:2:0; a pass over the algorithmic bytes at the measured "
          f"{HBM_MEASURED / 1e12:.2f} TB/s: {(12 + 1.5) * px / HBM_MEASURED * 1e6:.1f} us (8-bit)")
    for depth in (8, 10):
        fmt = stif.y4m.YuvFormat(W, H, "420jpeg", depth, "bt709", False)
        nbytes = px * 12 + n * fmt.frame_bytes
        yuv = torch.randint(0, 256 if depth == 8 else 4, (n, fmt.frame_bytes), device="cuda", dtype=torch.uint8,
                            generator=gen)
        out = torch.empty(n, 3, H, W, device="cuda")
        f, y, u, v, _ = ops._yuv_planes(yuv, fmt)
        dense = (3 * H * W, H * W, W)

        def to_rgb():
            L.check(lib.stif_yuv_to_rgb(ctypes.byref(f), y, u, v, n, out.data_ptr(), *dense, st), "stif_yuv_to_rgb")

        def to_yuv():
            L.check(lib.stif_rgb_to_yuv(ctypes.byref(f), rgb.data_ptr(), *dense, n, y, u, v, st), "stif_rgb_to_yuv")

        for name, fn in (("yuv_to_rgb", to_rgb), ("rgb_to_yuv", to_yuv)):
            med, lo, hi = timed(fn, iters, reps)
            print(f"  {depth:2d}-bit {name}: {med:8.1f} us per call (min {lo:.1f}, max {hi:.1f}), "
                  f"{med / n:7.1f} us per frame, {nbytes / med / 1e3:7.1f} GB/s of {nbytes / 1e6:.1f} MB")
    out = torch.empty(n, 3, H, W, device="cuda")
    med, lo, hi = timed(out.zero_, iters, reps)
    print(f"  zero fill of the fp32 frames (12 B/px out, what yuv_to_rgb writes): {med:8.1f} us per call "
          f"(min {lo:.1f}, max {hi:.1f}), {px * 12 / med / 1e3:7.1f} GB/s")
    med, lo, hi = timed(to_u8, iters, reps)
    nbytes = px * 15
    print(f"  frames_to_u8 (12 B/px in, 3 B/px out): {med:8.1f} us per call (min {lo:.1f}, max {hi:.1f}), "
          f"{med / n:7.1f} us per frame, {nbytes / med / 1e3:7.1f} GB/s of {nbytes / 1e6:.1f} MB")


def bench_stream(stif, reps):
    V = stif.video
    model = stif.LunaTokis(64, 6, 8, 5, 40)
    model.load_state_dict(stif.weights.make_state_dict(seed=0), strict=True)
    frames = torch.rand(7, 3, 128, 128, generator=torch.Generator().manual_seed(1)).cuda()

    def window():
        outs = V.run_sequence(model, frames)
        return sum(len(r) for r in outs)

    def stream():
        n = 0
        for o in V.render_stream(model, iter(frames), 25, 200, scale=4, chunk_pairs=6):
            n += 1
        return n

    res = {"run_sequence": [], "render_stream": []}
    counts = {}
    for fn in (window, stream):
        fn()                                            # warm-up: tables, constant maps, code objects
    for _ in range(reps):                               # alternate the arms
        for name, fn in (("run_sequence", window), ("render_stream", stream)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            counts[name] = fn()
            torch.cuda.synchronize()
            res[name].append((time.perf_counter() - t0) * 1e3)
    print("7 x 128 x 128 window, x4 size, x8 frame rate:")
    for name, ts in res.items():
        med = statistics.median(ts)
        print(f"  {name:14s}: {med:8.2f} ms per call (min {min(ts):.2f}, max {max(ts):.2f}), {counts[name]} frames, "
              f"{med / counts[name]:.3f} ms per output frame")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--no-stream", action="store_true")
    opt = ap.parse_args()
    assert torch.cuda.is_available(), "bench_yuv needs the GPU"
    stif = stif_pkg.load()
    W, H = (480, 270) if opt.small else (1920, 1080)
    bench_kernels(stif, W, H, 8, opt.iters, opt.reps)
    if not opt.no_stream:
        bench_stream(stif, opt.reps)


if __name__ == "__main__":
    main()
