"""Time the training kernels of PCD_Align and one forward + backward of train.PCD_Align at the C0 pyramid shapes:
6 pairs x 128 x 128 (L1) and its halves 64 x 64 (L2), 32 x 32 (L3).  Device events around each call, warm-up rounds
first, the contenders of a section alternated in one process, median and min..max over the rounds.  Nothing here is
a gate.

  (a) stif_conv3x3_wgrad_cat, 216 form, against four stif_conv3x3_wgrad calls on contiguous 64-channel copies of gy
      (copies included); the cat form against two such calls (no copies: its gy is 64 channels already).  TFLOP/s of
      the nine-tap count and the share of the fp32 MFMA peak (157.3 TFLOP/s); the 64 -> 64 kernel alone beside them.
  (b) stif_upsample2x_bwd_nhwc against torch's autograd of F.interpolate on channels_last, 64 channels, scale 2.
  (c) one forward + backward of train.PCD_Align in both mfma modes, and its split by ops.TRACE label (device events
      around every library call of one traced step, median over the rounds): in particular the share of the deformable
      conv's backward, and the untraced rest -- the torch ops between the calls: the activation masks, torch.cat of
      the two branches and the allocations.
  (d) ops.dcn_offmask + ops.dcn_bwd (stif_dcn_bwd_nhwc: g_in, g_om, g_w, g_b) against what they replace, at the three
      pyramid shapes: ops.dcn_v2_backward with the NHWC -> NCHW copies of the input and the output gradient, the
      offset / mask split with its sigmoid, and the g_om assembly the DCN_sep node made with torch ops; both entry
      points alone beside them, and the new one without the weight kernel and without the data kernel.
"""
import argparse
import os
import statistics
import sys
from collections import defaultdict

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import stif_pkg  # noqa: E402

stif = stif_pkg.load()
L, ops, T = stif._lib, stif.ops, stif.train
LEVELS = {"L1 6x128x128": (6, 128, 128), "L2 6x64x64": (6, 64, 64), "L3 6x32x32": (6, 32, 32)}
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
    print(f"{name:52s} median {statistics.median(us):9.1f} us  min..max {min(us):9.1f} .. {max(us):9.1f}  {extra}",
          flush=True)
    return statistics.median(us)


def peak(flop, med_us):
    share = 100 * flop / (med_us * 1e-6) / PEAK_F32_MFMA
    return f"{flop / med_us / 1e6:6.1f} TFLOP/s = {share:4.1f} % of the fp32 MFMA peak"


def bench_wgrad(a):
    """(a)"""
    for name, (n, H, W) in LEVELS.items():
        x0, x1 = torch.randn(n, H, W, 64, device="cuda"), torch.randn(n, H, W, 64, device="cuda")
        g64, g256 = torch.randn(n, H, W, 64, device="cuda"), torch.randn(n, H, W, 256, device="cuda")
        g256[..., 216:] = 0

        def four_calls():
            for s in range(4):
                gs = g256[..., 64 * s:64 * s + 64].contiguous() if s < 3 else F.pad(g256[..., 192:216], (0, 40))
                ops.conv3x3_wgrad(x0, gs)

        r = timed({"om": lambda: ops.conv3x3_wgrad_cat([x0], g256, 216), "four": four_calls,
                   "cat": lambda: ops.conv3x3_wgrad_cat([x0, x1], g64, 64),
                   "two": lambda: (ops.conv3x3_wgrad(x0, g64), ops.conv3x3_wgrad(x1, g64)),
                   "one": lambda: ops.conv3x3_wgrad(x0, g64)}, a.rounds, a.warmup)
        px = n * H * W
        m = show(f"(a) {name} wgrad_cat 216 form", r["om"])
        print(" " * 56 + peak(2.0 * 216 * 64 * 9 * px, m) + "; of the 256 padded rows "
              + peak(2.0 * 256 * 64 * 9 * px, m))
        show(f"(a) {name} 4 x conv3x3_wgrad + gy copies", r["four"])
        m = show(f"(a) {name} wgrad_cat cat form", r["cat"])
        print(" " * 56 + peak(2.0 * 64 * 128 * 9 * px, m))
        show(f"(a) {name} 2 x conv3x3_wgrad", r["two"])
        m = show(f"(a) {name} conv3x3_wgrad (64 -> 64)", r["one"])
        print(" " * 56 + peak(2.0 * 64 * 64 * 9 * px, m))


def bench_upsample(a):
    """(b)"""
    for name, (n, H, W) in list(LEVELS.items())[:2]:
        gy = torch.randn(n, H, W, 64, device="cuda")
        x = torch.randn(n, 64, H // 2, W // 2, device="cuda").contiguous(memory_format=torch.channels_last)
        x.requires_grad_(True)
        up = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False) * 2
        g_nchw = gy.permute(0, 3, 1, 2)
        r = timed({"hip": lambda: ops.upsample2x_bwd(gy, 2.0),
                   "torch": lambda: torch.autograd.grad(up, x, g_nchw, retain_graph=True)}, a.rounds, a.warmup)
        nbytes = 4.0 * 64 * n * H * W * 1.25
        m = show(f"(b) {name} -> half: upsample2x_bwd", r["hip"])
        print(" " * 56 + f"{nbytes / (m * 1e-6) / 1e12:5.2f} TB/s of gy read + gx written")
        show(f"(b) {name} -> half: torch autograd of F.interpolate", r["torch"])


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
    if kind[0] == "wgrad_cat":
        return f"stif_conv3x3_wgrad_cat {kind[1:]}"
    return {"wgrad": "stif_conv3x3_wgrad", "up2": "stif_upsample2x_nhwc", "up2_bwd": "stif_upsample2x_bwd_nhwc",
            "dcn_v2_fwd": "stif_dcn_v2_forward", "dcn_v2_bwd": "stif_dcn_v2_backward", "dcn": "stif_dcn_nhwc",
            "dcn_bwd": "stif_dcn_bwd_nhwc", "dcn_offmask": "stif_dcn_offmask_nhwc",
            "dcn_bwd_contrib": "stif_dcn_bwd_contrib", "segsum": "stif_segsum"}.get(kind[0], kind[0])


DCN_GEOM = (3, 3, 1, 1, 1, 1, 1, 1, 8)


def bench_dcn(a):
    """(d)"""
    for name, (n, H, W) in LEVELS.items():
        g = torch.Generator().manual_seed(H)
        rnd = lambda *s: torch.randn(*s, generator=g).cuda()
        xh, gh, w, b = rnd(n, H, W, 64), rnd(n, H, W, 64), rnd(64, 64, 3, 3) / 24, rnd(64)
        om = rnd(n, H, W, 256)           # offsets ~ N(0, 1): a trained module's range
        om[..., 216:] = 0

        def old_path():
            x = xh.permute(0, 3, 1, 2).contiguous()
            offset = om[..., :144].permute(0, 3, 1, 2).contiguous()
            mask = torch.sigmoid(om[..., 144:216]).permute(0, 3, 1, 2).contiguous()
            go = gh.permute(0, 3, 1, 2).contiguous()
            g_in, g_off, g_mask, g_w, g_b = ops.dcn_v2_backward(x, w, b, offset, mask, go, *DCN_GEOM)
            g_om = torch.zeros(n, H, W, 256, dtype=torch.float32, device=xh.device)
            g_om[..., :144] = g_off.permute(0, 2, 3, 1)
            g_om[..., 144:216] = (g_mask * mask * (1.0 - mask)).permute(0, 2, 3, 1)
            return g_in, g_om, g_w, g_b

        offmask = ops.dcn_offmask(om)
        x, go = xh.permute(0, 3, 1, 2).contiguous(), gh.permute(0, 3, 1, 2).contiguous()
        offset = om[..., :144].permute(0, 3, 1, 2).contiguous()
        mask = torch.sigmoid(om[..., 144:216]).permute(0, 3, 1, 2).contiguous()
        r = {"new": lambda: ops.dcn_bwd(xh, ops.dcn_offmask(om), w, gh), "old": old_path,
             "bwd": lambda: ops.dcn_bwd(xh, offmask, w, gh),
             "v2": lambda: ops.dcn_v2_backward(x, w, b, offset, mask, go, *DCN_GEOM),
             "data": lambda: ops.dcn_bwd(xh, offmask, w, gh, need=(True, True, False)),
             "weight": lambda: ops.dcn_bwd(xh, offmask, w, gh, need=(False, False, True)),
             "offmask": lambda: ops.dcn_offmask(om)}
        if a.deterministic:   # the ordered g_in, alternated with the atomic lines above
            r["det"] = lambda: ops.dcn_bwd(xh, offmask, w, gh, deterministic=True)
            r["det-data"] = lambda: ops.dcn_bwd(xh, offmask, w, gh, need=(True, True, False), deterministic=True)
        r = timed(r, a.rounds, a.warmup)
        flop = 2.0 * 64 * 576 * n * H * W
        show(f"(d) {name} dcn_offmask + dcn_bwd", r["new"])
        show(f"(d) {name} dcn_v2_backward + copies, sigmoid, g_om", r["old"])
        m = show(f"(d) {name} dcn_bwd alone", r["bwd"])
        print(" " * 56 + peak(2 * flop, m) + " (column-gradient + weight-gradient GEMMs)")
        show(f"(d) {name} dcn_v2_backward alone", r["v2"])
        m = show(f"(d) {name} dcn_bwd, g_in + g_om only", r["data"])
        print(" " * 56 + peak(flop, m))
        m = show(f"(d) {name} dcn_bwd, g_w + g_b only", r["weight"])
        print(" " * 56 + peak(flop, m))
        show(f"(d) {name} dcn_offmask", r["offmask"])
        if a.deterministic:
            md = show(f"(d) {name} dcn_bwd alone, deterministic", r["det"])
            mdd = show(f"(d) {name} dcn_bwd, g_in + g_om only, deterministic", r["det-data"])
            print(f"      deterministic / atomic medians: dcn_bwd {md / statistics.median(r['bwd']):.2f}x, "
                  f"g_in + g_om only {mdd / statistics.median(r['data']):.2f}x", flush=True)
        ok = min(r["old"]) > max(r["new"])
        print(f"      ranges {'do not overlap: new max < old min' if ok else 'OVERLAP'}; "
              f"old / new medians = {statistics.median(r['old']) / statistics.median(r['new']):.1f}x", flush=True)


def bench_step(a):
    """(c)"""
    n, H, W = LEVELS["L1 6x128x128"]
    g = torch.Generator().manual_seed(0)
    mk = lambda: [torch.randn(n, 64, H >> l, W >> l, generator=g).cuda().contiguous(memory_format=torch.channels_last)
                  .requires_grad_(True) for l in range(3)]
    fea1, fea2 = mk(), mk()
    gout = torch.randn(n, 128, H, W, generator=g).cuda()
    nets = {}
    for mfma in ("f16x3", "f32"):
        torch.manual_seed(1)
        net = T.PCD_Align(mfma).cuda()
        with torch.no_grad():
            for m in net.modules():
                if isinstance(m, T.DCN_sep):
                    m.conv_offset_mask.weight.normal_(0, 0.01)
        nets[mfma] = net

    def step(net):
        for p in net.parameters():
            p.grad = None
        for t in fea1 + fea2:
            t.grad = None
        net(fea1, fea2).backward(gout)

    def det_step(net):
        with T.deterministic():
            step(net)

    fns = {k: (lambda net=net: step(net)) for k, net in nets.items()}
    if a.deterministic:   # the same nets under train.deterministic(), alternated with the atomic lines
        fns.update({k + " deterministic": (lambda net=net: det_step(net)) for k, net in nets.items()})
    r = timed(fns, a.rounds, a.warmup)
    for k in fns:
        show(f"(c) PCD_Align {k} forward + backward, 6 x 128 x 128", r[k])
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
    ap.add_argument("--only", choices=["wgrad", "upsample", "step", "dcn"])
    ap.add_argument("--deterministic", action="store_true",
                    help="add the ordered-sum paths (train.deterministic(), ops.dcn_bwd(deterministic=True)) beside "
                         "the atomic ones in (c) and (d); the traced step of (c) is then the deterministic one")
    a = ap.parse_args()
    print(f"device: {torch.cuda.get_device_name(0)}, rounds {a.rounds}, warm-up {a.warmup}")
    for name, fn in (("wgrad", bench_wgrad), ("upsample", bench_upsample), ("step", bench_step), ("dcn", bench_dcn)):
        if a.only in (None, name):
            fn(a)
