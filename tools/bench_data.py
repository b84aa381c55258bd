"""Time the training-batch builder alone (data.build_batch, stif_build_batch).

Shape: B = 18, d = 3 -> G = 192, LQ 32 x 32, GT 96 x 96, every flag on, from 720 x 1280 uint8 frames resident on the
device (5 per item).  Two arms, interleaved in one process on one GPU, HIP events around warmed-up loops, the median
of repeated loops:

  builder  data.build_batch on the whole frames (one stacked device tensor): two launches of k_build_batch that read
           the crops in place, plus one asynchronous upload of its tables, offsets and times;
  parent   what the parent commit offers for the same batch: video.resize_frames on the packed crops (already on the
           device: its most favourable start) at 1 / (2 d) and at 1 / 2, then torch flip, transpose and contiguous,
           and the reshape into [B, 2 | 3, 3, o, o]: 2 k_resize_in launches + 2 flips + 2 copies = 6 kernels.
  Printed as well: the builder on a nested list of the 5 B frames and on the packed crops (the parent arm's start),
  the two launches alone (everything already on the device), and for every arm the host time to issue one batch.

  python tools/bench_data.py [--batch 18] [--d 3.0] [--iters 20] [--reps 9]
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import stif_pkg  # noqa: E402


def timed_interleaved(arms, iters, reps, warmup=3):
    """arms {name: fn} -> {name: (median, min, max)} microseconds per call; the arms alternate within every rep"""
    for fn in arms.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in arms}
    for _ in range(reps):
        for name, fn in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            out[name].append(e0.elapsed_time(e1) * 1e3 / iters)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=18)
    ap.add_argument("--d", type=float, default=3.0)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=9)
    opt = ap.parse_args()
    assert torch.cuda.is_available(), "bench_data needs the GPU"
    stif = stif_pkg.load()
    D, V = stif.data, stif.video
    B = opt.batch
    geo = D.resize_geometry(64, opt.d)
    G = geo.G
    p = D.CollateParams(opt.d, G, 264, 544, True, True, True)
    gen = torch.Generator(device="cuda").manual_seed(0)
    stacked = torch.randint(0, 256, (B, 5, 720, 1280, 3), device="cuda", dtype=torch.uint8, generator=gen)
    frames = [[stacked[b, k] for k in range(5)] for b in range(B)]
    times = np.tile(np.array([[0.125, 0.5, 0.875]]), (B, 1))
    r, c = p.crop_origin(720, 1280)
    crops = torch.stack([torch.stack([f[r:r + G, c:c + G] for f in item]) for item in frames]).contiguous()
    lq_in = crops[:, :2].reshape(2 * B, G, G, 3).contiguous()
    gt_in = crops[:, 2:].reshape(3 * B, G, G, 3).contiguous()

    def builder():
        return D.build_batch(stacked, p, "cuda", times)

    def builder_list():
        return D.build_batch(frames, p, "cuda", times)

    def builder_packed():
        return D.build_batch(crops, p, "cuda", times)

    # the two launches alone, everything already on the device
    L, lib = stif._lib, stif._lib.lib()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    tabs = []
    for o, scale in ((geo.lq, geo.lq_scale), (geo.gt, geo.gt_scale)):
        w, idx, s0 = V.resize_tables(G, o, scale)
        tabs.append((o, torch.from_numpy(w).cuda(), torch.from_numpy(idx).cuda(), w.shape[1], s0))
    k_off = [torch.arange(2 * B, dtype=torch.int64, device="cuda") * (G * G * 3),
             torch.arange(3 * B, dtype=torch.int64, device="cuda") * (G * G * 3)]
    k_str = torch.full((3 * B,), 3 * G, dtype=torch.int64, device="cuda")
    k_out = [torch.empty(2 * B, 3, geo.lq, geo.lq, device="cuda"), torch.empty(3 * B, 3, geo.gt, geo.gt, device="cuda")]
    k_src = [lq_in, gt_in]

    def kernels():
        for g, (o, w, idx, P, s0) in enumerate(tabs):
            L.check(lib.stif_build_batch(k_src[g].data_ptr(), k_off[g].data_ptr(), k_str.data_ptr(),
                                         k_out[g].data_ptr(), k_out[g].shape[0], G, o, w.data_ptr(), idx.data_ptr(), P,
                                         s0, 7, st), "stif_build_batch")

    def parent():
        lq = V.resize_frames(lq_in, geo.lq_scale).flip(-1, -2).transpose(-1, -2).contiguous()
        gt = V.resize_frames(gt_in, geo.gt_scale).flip(-1, -2).transpose(-1, -2).contiguous()
        return lq.view(B, 2, 3, geo.lq, geo.lq), gt.view(B, 3, 3, geo.gt, geo.gt)

    (lq, gt), outs = parent(), [builder(), builder_list(), builder_packed()]
    kernels()
    same = all(torch.equal(a["LQs"], lq) and torch.equal(a["GT"], gt) for a in outs)
    same = same and torch.equal(k_out[0].view_as(lq), lq) and torch.equal(k_out[1].view_as(gt), gt)
    print(f"B = {B}, d = {opt.d}: G = {G}, LQ {geo.lq} x {geo.lq}, GT {geo.gt} x {geo.gt}, flags 7; "
          f"builder == parent route bit for bit: {same}")
    assert same
    arms = {"builder (frames in place)": builder, "parent route (packed crops)": parent,
            "builder (list of 5 B frames)": builder_list, "builder (packed crops)": builder_packed,
            "the two launches alone": kernels}
    res = timed_interleaved(arms, opt.iters, opt.reps)
    launches = {"parent route (packed crops)": "6 kernels", "the two launches alone": "2 kernels"}
    for name, (med, lo, hi) in res.items():
        # the host's share: the same loop without a device wait
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(opt.iters):
            arms[name]()
        host = (time.perf_counter() - t0) * 1e6 / opt.iters
        torch.cuda.synchronize()
        print(f"  {name:30s}: {med:9.1f} us per batch (min {lo:.1f}, max {hi:.1f}), host {host:7.1f} us to issue; "
              f"{launches.get(name, '2 kernels + 1 upload')}")
    ratio = res["parent route (packed crops)"][0] / res["builder (frames in place)"][0]
    print(f"  parent / builder = {ratio:.2f}")
    assert ratio >= 1.0, "the builder must not be slower than the parent commit's route"


if __name__ == "__main__":
    main()
