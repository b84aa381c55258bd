"""Time the scene-cut kernel beside a one-pass yardstick.

stif_scene_sad on n = 9 frames of 1920x1080 fp32 RGB (the 8 pairs of a default chunk: one walk, every frame read
once), on both of its load paths: the vector path (16-byte loads; a dense, aligned buffer) and the scalar path (the
same frames in a view whose base pointer is off by one float).  stif_yuv_to_rgb (8-bit 4:2:0 -> the same fp32
frames, its vector path) runs in the same process as the yardstick for a one-pass bandwidth-bound kernel: it writes
the 12 B/px that scene_sad reads.  HIP events around warmed-up loops, the arms alternated, the median of repeated
loops; achieved GB/s against the algorithmic bytes (scene_sad: 12 B/px read once; yuv_to_rgb: 12 B/px written +
1.5 samples/px read).  No pass / fail time.

  python tools/bench_scene.py [--iters 20] [--reps 7] [--small]     (--small: 480x270, a rehearsal size)
"""
import argparse
import ctypes
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import stif_pkg  # noqa: E402

HBM_MEASURED = 6.29e12     # B/s, float4 copy (tools/bench_metrics.py)


def loop_us(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--small", action="store_true")
    opt = ap.parse_args()
    assert torch.cuda.is_available(), "bench_scene needs the GPU"
    stif = stif_pkg.load()
    L, lib, ops = stif._lib, stif._lib.lib(), stif.ops
    W, H = (480, 270) if opt.small else (1920, 1080)
    n = 9
    px = n * H * W
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    gen = torch.Generator(device="cuda").manual_seed(0)

    fmt = stif.y4m.YuvFormat(W, H, "420jpeg", 8, "bt709", False)
    yuv = torch.randint(0, 256, (n, fmt.frame_bytes), device="cuda", dtype=torch.uint8, generator=gen)
    rgb = torch.empty(n, 3, H, W, device="cuda")        # 16-byte aligned: the vector path
    off = torch.empty(px * 3 + 4, device="cuda")[1:px * 3 + 1].view(n, 3, H, W)   # a float off: the scalar path
    assert rgb.data_ptr() % 16 == 0 and off.data_ptr() % 16 == 4
    f, y, u, v, _ = ops._yuv_planes(yuv, fmt)
    dense = (3 * H * W, H * W, W)
    sad = torch.empty(n - 1, device="cuda", dtype=torch.int64)
    need = lib.stif_scene_workspace_size(n, H, W)
    ws = torch.empty(need // 8, device="cuda", dtype=torch.int64)

    def to_rgb():
        L.check(lib.stif_yuv_to_rgb(ctypes.byref(f), y, u, v, n, rgb.data_ptr(), *dense, st), "stif_yuv_to_rgb")

    def scene(t):
        def fn():
            L.check(lib.stif_scene_sad(t.data_ptr(), *dense, n, H, W, sad.data_ptr(), ws.data_ptr(), need, st),
                    "stif_scene_sad")
        return fn

    to_rgb()
    want = ops.scene_sad(rgb)
    off.copy_(rgb)
    assert torch.equal(ops.scene_sad(off), want)        # the two paths agree before they are timed
    arms = {"scene_sad, vector loads": (scene(rgb), px * 12),
            "scene_sad, scalar loads": (scene(off), px * 12),
            "yuv_to_rgb (8-bit 4:2:0, vector)": (to_rgb, px * 12 + n * fmt.frame_bytes)}
    for fn, _ in arms.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in arms}
    for _ in range(opt.reps):                           # alternate the arms
        for k, (fn, _) in arms.items():
            times[k].append(loop_us(fn, opt.iters))
    print(f"{n} frames of {W}x{H}; a pass over 12 B/px at the measured {HBM_MEASURED / 1e12:.2f} TB/s: "
          f"{px * 12 / HBM_MEASURED * 1e6:.1f} us")
    for k, (_, nbytes) in arms.items():
        med = statistics.median(times[k])
        print(f"  {k:34s}: {med:8.1f} us per call (min {min(times[k]):.1f}, max {max(times[k]):.1f}), "
              f"{med / n:6.1f} us per frame, {nbytes / med / 1e3:7.1f} GB/s of {nbytes / 1e6:.1f} MB")
    print(f"  workspace {need} B; sums of the random frames: {want.tolist()}")


if __name__ == "__main__":
    main()
