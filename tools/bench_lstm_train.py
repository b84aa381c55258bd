"""Time the training kernels of the ConvLSTM part and one forward + backward of train.BiDeformableConvLSTM at the C0
latent shape: 6 sequences x 3 steps x 64 channels x 128 x 128.  Device events around each call, warm-up rounds first,
the contenders of a section alternated in one process, median and min..max over the rounds.  Nothing here is a gate.

  (a) stif_lstm_gates_nhwc and stif_lstm_gates_bwd_nhwc on 6 x 128 x 128 pixels: the achieved bytes/s against the bytes
      they must move (forward: pre and c_cur read, h_next and c_next written, 1792 B per pixel; backward with every
      gradient: pre, c_cur, g_h, g_c_next read, g_pre, g_c_cur written, 3072 B per pixel), beside the same arithmetic
      in torch ops on the same NHWC buffers.
  (b) stif_conv1x1_wgrad, one and two inputs, on 18 x 128 x 128 pixels (conv_1x1 sees every step at once): bytes/s of
      the 256 (1 + nx) B per pixel it must read, beside torch's einsum on the same buffers; and the (2, 256, 256) block
      weight gradient of the cell's conv with its share of the fp32 MFMA peak.
  (c) one forward + backward of train.BiDeformableConvLSTM in both mfma modes, and its split by ops.TRACE label (device
      events around every library call of one traced step, median over the rounds): the share of each new kernel, and
      the untraced rest -- the torch ops between the calls.
"""
import argparse
import os
import statistics
import sys
from collections import defaultdict

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import stif_pkg  # noqa: E402

stif = stif_pkg.load()
L, ops, T = stif._lib, stif.ops, stif.train
B, STEPS, H, W = 6, 3, 128, 128
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
    print(f"{name:56s} median {statistics.median(us):9.1f} us  min..max {min(us):9.1f} .. {max(us):9.1f}  {extra}",
          flush=True)
    return statistics.median(us)


def rate(nbytes, med_us):
    return f"{nbytes / (med_us * 1e-6) / 1e12:5.2f} TB/s of the {nbytes / 1e6:.1f} MB it must move"


def bench_gates(a):
    """(a)"""
    px = B * H * W
    pre, gpre = torch.randn(B, H, W, 256, device="cuda"), torch.empty(B, H, W, 256, device="cuda")
    c, gh, gc = (torch.randn(B, H, W, 64, device="cuda") for _ in range(3))
    h, cn, gcc = (torch.empty(B, H, W, 64, device="cuda") for _ in range(3))

    def torch_fwd():
        i, f, o, g = torch.split(pre, 64, dim=3)
        c2 = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
        return torch.sigmoid(o) * torch.tanh(c2), c2

    r = timed({"fwd": lambda: ops.lstm_gates(pre, c, h, cn), "torch": torch_fwd,
               "bwd": lambda: ops.lstm_gates_bwd(pre, c, gh, gc, g_pre=gpre, g_c_cur=gcc),
               "bwd_h": lambda: ops.lstm_gates_bwd(pre, c, gh, None, need_c=False, g_pre=gpre)}, a.rounds, a.warmup)
    m = show("(a) lstm_gates 6x128x128", r["fwd"])
    print(" " * 60 + rate(4.0 * (256 + 3 * 64) * px, m))
    show("(a) the same arithmetic in torch ops", r["torch"])
    m = show("(a) lstm_gates_bwd, every gradient", r["bwd"])
    print(" " * 60 + rate(4.0 * (2 * 256 + 4 * 64) * px, m))
    m = show("(a) lstm_gates_bwd, g_h only, no g_c_cur (last step)", r["bwd_h"])
    print(" " * 60 + rate(4.0 * (2 * 256 + 2 * 64) * px, m))


def bench_wgrad(a):
    """(b)"""
    n = B * STEPS
    px = n * H * W
    x0, x1, gy = (torch.randn(n, H, W, 64, device="cuda") for _ in range(3))
    r = timed({"two": lambda: ops.conv1x1_wgrad([x0, x1], gy), "one": lambda: ops.conv1x1_wgrad([x0], gy),
               "torch": lambda: (torch.einsum("nhwo,nhwi->oi", gy, x0), torch.einsum("nhwo,nhwi->oi", gy, x1),
                                 gy.sum((0, 1, 2)))}, a.rounds, a.warmup)
    m = show("(b) conv1x1_wgrad (64 | 64) -> 64, 18x128x128", r["two"])
    print(" " * 60 + rate(4.0 * 64 * 3 * px, m))
    m = show("(b) conv1x1_wgrad 64 -> 64", r["one"])
    print(" " * 60 + rate(4.0 * 64 * 2 * px, m))
    show("(b) two torch einsums and a sum", r["torch"])
    px = B * H * W
    xa, xb, g256 = (torch.randn(B, H, W, c, device="cuda") for c in (64, 64, 256))
    r = timed({"cell": lambda: ops.conv3x3_wgrad_cat([xa, xb], g256, 256)}, a.rounds, a.warmup)
    m = show("(b) wgrad_cat (2, 256, 256), 6x128x128", r["cell"])
    flop = 2.0 * 256 * 128 * 9 * px
    print(" " * 60 + f"{flop / m / 1e6:6.1f} TFLOP/s = {100 * flop / (m * 1e-6) / PEAK_F32_MFMA:4.1f} % of the fp32 "
          "MFMA peak")


class Tracer:
    """ops.TRACE: device events around every library call, summed per label."""

    def __init__(self):
        self.ev = []

    def begin(self, kind, flops, nbytes=0.0):
        e0 = torch.cuda.Event(enable_timing=True)
        e0.record()
        self.ev.append([kind, e0, None])

    def end(self):
        e1 = torch.cuda.Event(enable_timing=True)
        e1.record()
        self.ev[-1][2] = e1

    def totals(self):
        torch.cuda.synchronize()
        tot = defaultdict(float)
        for kind, e0, e1 in self.ev:
            tot[kind] += e0.elapsed_time(e1) * 1e3
        return tot


def label(kind):
    if kind[0] == "wino":
        return f"stif_conv3x3_wino cout {kind[5]}" + (" two inputs" if kind[4] else "")
    if kind[0] == "conv":
        return f"stif_conv2d_nhwc ks {kind[1]} stride {kind[2]}" + (" two inputs" if kind[4] else "")
    if kind[0] == "wgrad_cat":
        return f"stif_conv3x3_wgrad_cat {kind[1:]}"
    if kind[0] == "wgrad_1x1":
        return f"stif_conv1x1_wgrad nx {kind[1]}"
    return {"wgrad": "stif_conv3x3_wgrad", "wgrad_s2": "stif_conv3x3s2_wgrad", "dgrad_s2": "stif_conv3x3s2_dgrad",
            "up2": "stif_upsample2x_nhwc", "up2_bwd": "stif_upsample2x_bwd_nhwc", "dcn": "stif_dcn_nhwc",
            "dcn_bwd": "stif_dcn_bwd_nhwc", "dcn_offmask": "stif_dcn_offmask_nhwc",
            "lstm_gates": "stif_lstm_gates_nhwc", "lstm_gates_bwd": "stif_lstm_gates_bwd_nhwc",
            "dcn_bwd_contrib": "stif_dcn_bwd_contrib", "segsum": "stif_segsum"}.get(kind[0], kind[0])


def bench_step(a):
    """(c)"""
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, STEPS, 64, H, W, generator=g).cuda().requires_grad_(True)
    gout = torch.randn(B, STEPS, 64, H, W, generator=g).cuda()
    nets = {}
    for mfma in ("f16x3", "f32"):
        torch.manual_seed(1)
        net = T.BiDeformableConvLSTM(mfma).cuda()
        with torch.no_grad():
            for m in net.modules():
                if isinstance(m, T.DCN_sep):
                    m.conv_offset_mask.weight.normal_(0, 0.01)
        nets[mfma] = net

    def step(net):
        for p in net.parameters():
            p.grad = None
        x.grad = None
        net(x).backward(gout)

    def det_step(net):
        with T.deterministic():
            step(net)

    fns = {k: (lambda net=net: step(net)) for k, net in nets.items()}
    if a.deterministic:   # the same nets under train.deterministic(), alternated with the atomic lines
        fns.update({k + " deterministic": (lambda net=net: det_step(net)) for k, net in nets.items()})
    r = timed(fns, a.rounds, a.warmup)
    for k in fns:
        show(f"(c) BiDeformableConvLSTM {k} forward + backward, 6x3x128x128", r[k])
    assert nets["f16x3"].range_status() == 0
    per = defaultdict(list)
    whole = []
    for _ in range(a.rounds):
        tr = Tracer()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ops.TRACE = tr
        try:
            e0.record()
            (det_step if a.deterministic else step)(nets["f16x3"])
            e1.record()
        finally:
            ops.TRACE = None
        tot = tr.totals()
        whole.append(e0.elapsed_time(e1) * 1e3)
        by = defaultdict(float)
        for kind, us in tot.items():
            by[label(kind)] += us
        by["untraced: torch ops between the calls"] = whole[-1] - sum(tot.values())
        for k, us in by.items():
            per[k].append(us)
    wm = statistics.median(whole)
    print(f"(c) split of one traced f16x3 {'deterministic ' if a.deterministic else ''}step (events around every call): {wm:9.1f} us", flush=True)
    for k, us in sorted(per.items(), key=lambda kv: -statistics.median(kv[1])):
        m = statistics.median(us)
        print(f"      {k:56s} {m:9.1f} us  {100 * m / wm:5.1f} %", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", choices=["gates", "wgrad", "step"])
    ap.add_argument("--deterministic", action="store_true",
                    help="add the steps under train.deterministic() beside the atomic ones in (c); the traced step is "
                         "then the deterministic one")
    a = ap.parse_args()
    print(f"device: {torch.cuda.get_device_name(0)}, rounds {a.rounds}, warm-up {a.warmup}")
    for name, fn in (("gates", bench_gates), ("wgrad", bench_wgrad), ("step", bench_step)):
        if a.only in (None, name):
            fn(a)
