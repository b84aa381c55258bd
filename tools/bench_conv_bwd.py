"""Time the 3x3 conv backward on the trunk shapes of tools/bench_conv.py: C1 (18 x 256 x 256 x 64) and C0
(18 x 128 x 128 x 64).  Device events around each call, warm-up rounds first, the contenders of a section alternated
in one process, median and min..max over the rounds.

  (a) stif_conv3x3_wgrad: time per call and the fraction of the fp32 MFMA peak (157.3 TFLOP/s).  The reduction
      kernel's share needs per-kernel times: run `rocprofv3 --kernel-trace --stats -d DIR -- python
      tools/bench_conv_bwd.py --only wgrad` in a run of its own and compare k_wgrad_reduce with k_wgrad.
  (b) the device packer per call, against host pack_conv + upload (host clock around a synchronise).
  (c) one forward + backward of train.ResidualBlock_noBN in both mfma modes, against the same block built from
      nn.Conv2d on the same GPU (channels_last and contiguous, both reported), and the torch elementwise ReLU mask
      of the block's backward timed alone for its share.
  (d) the frame encoder's kernels at the frame shapes of the trunks' benchmark (14 x 128 x 128 and 14 x 256 x 256 at
      L1, and the 14 x 64 x 64 L2 input of the second stride-2 conv): stif_conv3x3s2_wgrad and stif_conv3x3s2_dgrad
      in TFLOP/s of the nine-tap count and their share of the fp32 MFMA peak, stif_conv_first_wgrad in bytes/s of gy
      against the HBM roof (8 TB/s), the PLAIN device packer beside k_pack_wino.  Reported, not gated.
  (e) one forward + backward of train.FrameFeatures(5) against the same module built from nn.Conv2d on the same GPU,
      channels_last and contiguous.  Gate: the engine's median is not above torch channels_last's at both shapes
      (the exit status says so); ConvFirst and ConvDown alone against their nn.Conv2d forms give the split.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import stif_pkg  # noqa: E402

stif = stif_pkg.load()
L, ops, T = stif._lib, stif.ops, stif.train
SHAPES = {"C1": (18, 256, 256), "C0": (18, 128, 128)}
PEAK_F32_MFMA = 157.3e12


def timed(fns, rounds, warmup):
    """Per-call device times in us of each callable, the callables alternated round by round."""
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(rounds):
        for k, f in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            out[k].append(e0.elapsed_time(e1) * 1e3)
    return out


def show(name, us, extra=""):
    print(f"{name:44s} median {statistics.median(us):9.1f} us  min..max {min(us):9.1f} .. {max(us):9.1f}  {extra}",
          flush=True)
    return statistics.median(us)


class TorchBlock(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv2d(64, 64, 3, 1, 1)
        self.conv2 = nn.Conv2d(64, 64, 3, 1, 1)

    def forward(self, x):
        return x + self.conv2(torch.relu(self.conv1(x)))


class TorchEncoder(nn.Module):
    """train.FrameFeatures from nn.Conv2d: what a user has without the engine's backward kernels"""

    def __init__(self, front_RBs=5):
        super().__init__()
        self.conv_first = nn.Conv2d(3, 64, 3, 1, 1)
        self.feature_extraction = nn.Sequential(*[TorchBlock() for _ in range(front_RBs)])
        self.fea_L2_conv1 = nn.Conv2d(64, 64, 3, 2, 1)
        self.fea_L2_conv2 = nn.Conv2d(64, 64, 3, 1, 1)
        self.fea_L3_conv1 = nn.Conv2d(64, 64, 3, 2, 1)
        self.fea_L3_conv2 = nn.Conv2d(64, 64, 3, 1, 1)

    def forward(self, x):
        act = lambda t: nn.functional.leaky_relu(t, 0.1)
        L1 = self.feature_extraction(act(self.conv_first(x)))
        L2 = act(self.fea_L2_conv2(act(self.fea_L2_conv1(L1))))
        L3 = act(self.fea_L3_conv2(act(self.fea_L3_conv1(L2))))
        return L1, L2, L3


FRAME_SHAPES = {"14x128x128": (14, 128, 128), "14x256x256": (14, 256, 256)}
HBM_ROOF = 8.0e12


def bench_frame_kernels(a, w, b):
    """(d)"""
    wd, bd = torch.from_numpy(w).cuda(), torch.from_numpy(b).cuda()
    r = timed({"plain": lambda: ops.pack_conv_plain_dev(wd, bd), "wino": lambda: ops.pack_conv_dev(wd, bd, L.PACK_WINO)},
              a.rounds, a.warmup)
    show("(d) pack_conv_plain_dev", r["plain"])
    show("(d) pack_conv_dev f32 (k_pack_wino), alternated", r["wino"])
    for sname, (n, H, W) in dict(FRAME_SHAPES, **{"14x64x64 (L2 of 128)": (14, 64, 64)}).items():
        Ho, Wo = (H + 1) // 2, (W + 1) // 2
        x = torch.randn(n, H, W, 64, device="cuda")
        gy = torch.randn(n, Ho, Wo, 64, device="cuda")
        flop = 2.0 * 64 * 64 * 9 * n * Ho * Wo
        r = timed({"wgrad": lambda: ops.conv3x3s2_wgrad(x, gy), "dgrad": lambda: ops.conv3x3s2_dgrad(gy, wd, H, W)},
                  a.rounds, a.warmup)
        for k, what in (("wgrad", "stif_conv3x3s2_wgrad (both kernels)"), ("dgrad", "stif_conv3x3s2_dgrad")):
            med = statistics.median(r[k])
            show(f"(d) {sname} {what}", r[k], f"{flop / med / 1e6:6.1f} TFLOP/s = "
                 f"{100 * flop / med / 1e-6 / PEAK_F32_MFMA:4.1f} % of the fp32 MFMA peak")
        if sname in FRAME_SHAPES:
            frames = torch.rand(n, 3, H, W, device="cuda")
            g1 = torch.randn(n, H, W, 64, device="cuda")
            r = timed({"cf": lambda: ops.conv_first_wgrad(frames, g1)}, a.rounds, a.warmup)
            med = statistics.median(r["cf"])
            bps = 256.0 * n * H * W / (med * 1e-6)
            show(f"(d) {sname} stif_conv_first_wgrad (both kernels)", r["cf"],
                 f"{bps / 1e12:5.2f} TB/s of gy = {100 * bps / HBM_ROOF:4.1f} % of the HBM roof")


def bench_encoder(a):
    """(e); returns whether the gate holds"""
    ok = True
    for sname, (n, H, W) in FRAME_SHAPES.items():
        frames = torch.rand(n, 3, H, W, device="cuda")
        r3 = [torch.randn(n, 64, H >> k, W >> k, device="cuda").contiguous(memory_format=torch.channels_last)
              for k in range(3)]
        r3c = [t.contiguous() for t in r3]

        def step(net, gs):
            def f():
                net.zero_grad(set_to_none=True)
                torch.autograd.backward(net(frames), gs)
            return f

        fns = {f"stif {m}": step(T.FrameFeatures(5, mfma=m).cuda(), r3) for m in ("f16x3", "f32")}
        fns["torch nn.Conv2d channels_last"] = step(TorchEncoder().cuda().to(memory_format=torch.channels_last), r3)
        fns["torch nn.Conv2d contiguous"] = step(TorchEncoder().cuda(), r3c)
        r = timed(fns, a.rounds, a.warmup)
        med = {k: show(f"(e) {sname} FrameFeatures(5) fwd+bwd: {k}", v) for k, v in r.items()}
        ratio = med["stif f16x3"] / med["torch nn.Conv2d channels_last"]
        good = ratio <= 1.0
        ok &= good
        print(f"    {sname} gate (stif f16x3 <= torch channels_last): {ratio:5.2f} x  {'PASS' if good else 'FAIL'}; "
              f"range status {T.range_status()}", flush=True)

        # the split: the three convs this module adds, each alone against its nn.Conv2d form
        x1 = torch.randn(n, 64, H, W, device="cuda").contiguous(memory_format=torch.channels_last).requires_grad_(True)
        g2 = r3[1]

        def mstep(net, inp, g, post=None):
            def f():
                net.zero_grad(set_to_none=True)
                inp.grad = None
                o = net(inp)
                (post(o) if post else o).backward(g)
            return f

        act = lambda t: nn.functional.leaky_relu(t, 0.1)
        fns = {"stif ConvDown": mstep(T.ConvDown().cuda(), x1, g2),
               "torch Conv2d s2 + lrelu channels_last": mstep(
                   nn.Conv2d(64, 64, 3, 2, 1).cuda().to(memory_format=torch.channels_last), x1, g2, act),
               "stif ConvFirst": mstep(T.ConvFirst().cuda(), frames, r3[0]),
               "torch Conv2d 3->64 + lrelu channels_last": mstep(
                   nn.Conv2d(3, 64, 3, 1, 1).cuda().to(memory_format=torch.channels_last), frames, r3[0], act)}
        r = timed(fns, a.rounds, a.warmup)
        for k, v in r.items():
            show(f"(e) {sname} split: {k}", v)
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["wgrad", "pack", "block", "frame", "encoder"])
    ap.add_argument("--shapes", default="C1,C0")
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    torch.manual_seed(0)
    rng = np.random.default_rng(0)
    w = (rng.standard_normal((64, 64, 3, 3)) * 0.05).astype(np.float32)
    b = rng.standard_normal(64).astype(np.float32)

    if a.only in (None, "pack"):
        wd, bd = torch.from_numpy(w).cuda(), torch.from_numpy(b).cuda()
        status = torch.zeros(1, dtype=torch.int32, device="cuda")
        for name, mode in (("f32", L.PACK_WINO), ("f16x3", L.PACK_WINO | L.PACK_F16X3)):
            r = timed({"dev": lambda: ops.pack_conv_dev(wd, bd, mode, status=status)}, a.rounds, a.warmup)
            show(f"(b) pack_conv_dev {name}", r["dev"])
            host = []
            for _ in range(a.rounds):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ops.pack_conv(w, b, mode)
                torch.cuda.synchronize()
                host.append((time.perf_counter() - t0) * 1e6)
            show(f"(b) host pack_conv + upload {name} (host clock)", host)

    for sname in a.shapes.split(",") if a.only not in ("frame", "encoder") else ():
        n, H, W = SHAPES[sname]
        x = torch.randn(n, H, W, 64, device="cuda")
        gy = torch.randn(n, H, W, 64, device="cuda")
        flop = 2.0 * 64 * 64 * 9 * n * H * W
        if a.only in (None, "wgrad"):
            r = timed({"wgrad": lambda: ops.conv3x3_wgrad(x, gy)}, a.rounds, a.warmup)
            med = statistics.median(r["wgrad"])
            show(f"(a) {sname} stif_conv3x3_wgrad (both kernels)", r["wgrad"],
                 f"{flop / med / 1e6:6.1f} TFLOP/s = {100 * flop / med / 1e-6 / PEAK_F32_MFMA:4.1f} % of the fp32 MFMA peak")
        if a.only in (None, "block"):
            xn = x.permute(0, 3, 1, 2)                              # logical NCHW, channels_last memory
            go = torch.randn_like(xn)
            blocks = {f"stif {m}": T.ResidualBlock_noBN(mfma=m).cuda() for m in ("f32", "f16x3")}
            ref = TorchBlock().cuda()
            ref_cl = TorchBlock().cuda().to(memory_format=torch.channels_last)
            xc, goc = xn.contiguous(), go.contiguous()

            def step(net, inp, g):
                def f():
                    net.zero_grad(set_to_none=True)
                    inp.grad = None
                    net(inp).backward(g)
                return f

            xs = xn.detach().requires_grad_(True)
            xcs = xc.detach().requires_grad_(True)
            fns = {k: step(m, xs, go) for k, m in blocks.items()}
            fns["torch nn.Conv2d channels_last"] = step(ref_cl, xs, go)
            fns["torch nn.Conv2d contiguous"] = step(ref, xcs, goc)
            tt = x.clone()
            fns["relu mask alone (gt * (t > 0))"] = lambda: gy * (tt > 0)
            r = timed(fns, a.rounds, a.warmup)
            med = {k: show(f"(c) {sname} block fwd+bwd: {k}", v) for k, v in r.items()}
            best = min(med["torch nn.Conv2d channels_last"], med["torch nn.Conv2d contiguous"])
            for k in blocks:
                print(f"    {sname} {k}: {med[k] / best:5.2f} x the faster torch block; mask share "
                      f"{100 * med['relu mask alone (gt * (t > 0))'] / med[k]:4.1f} %", flush=True)
            print(f"    range status after the timed steps: {T.range_status()}", flush=True)

    if a.only in (None, "frame"):
        bench_frame_kernels(a, w, b)
    if a.only in (None, "encoder") and not bench_encoder(a):
        sys.exit("gate (e) failed: FrameFeatures on the engine is slower than torch channels_last")


if __name__ == "__main__":
    main()
