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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["wgrad", "pack", "block"])
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

    for sname in a.shapes.split(","):
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


if __name__ == "__main__":
    main()
