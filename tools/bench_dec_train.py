"""Time the training kernels of the SIREN decoder, one forward + backward of train.Decoder beside the same decoder
done by torch autograd on the same GPU (F.grid_sample + F.linear + torch.sin, fp32), and one whole train.LunaTokis
step, at the C0 training shape of tools/bench_lstm_train.py: 6 items of 128 x 128 LR pixels, decoded at --scale (x2 by
default: N = 6 x 256 x 256 rows).  Device events around each call, warm-up rounds first, the contenders of a section
alternated in one process, median and min..max over the rounds.  Nothing here is a gate.

  (a) the builders and adjoints (stif_dec_x{1,2,3}_fwd / _bwd) with the bytes they must move, and stif_siren_fwd /
      stif_siren_bwd of the three nets with their share of the fp32 MFMA peak (2 MACs forward; backward 4 MACs, the
      data and the weight pass);
  (b) train.Decoder forward + backward for one time, against torch autograd of the same arithmetic;
  (c) one train.LunaTokis step (forward, Charbonnier loss, backward; f16x3 convs, fp32 decoder) and its split by
      ops.TRACE label.
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
B, H, W = 6, 128, 128
PEAK_F32_MFMA = 157.3e12
NETS = {"feat_imnet": (201, (64, 64, 256), 64), "flow_imnet": (263, (64, 64, 256), 4),
        "encode_imnet": (525, (64, 64, 256, 256), 3)}


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


def mfma_share(flop, med_us):
    return f"{flop / med_us / 1e6:6.1f} TFLOP/s = {100 * flop / (med_us * 1e-6) / PEAK_F32_MFMA:4.1f} % of the fp32 MFMA peak"


def inputs(a):
    g = torch.Generator().manual_seed(0)
    feat = (torch.randn(B, 3, 64, H, W, generator=g) * 0.5).cuda()
    inp = torch.rand(B, 2, 3, H, W, generator=g).cuda()
    return feat, inp, a.scale * H, a.scale * W


def bench_kernels(a):
    """(a)"""
    feat, inp, HH, WW = inputs(a)
    lat = feat.reshape(B, 192, H, W).permute(0, 2, 3, 1).contiguous()
    geom = ops.DecTrainGeom(lat, inp.reshape(B, 6, H, W).contiguous(), torch.full((B,), 0.5, device="cuda"), HH, WW)
    N = geom.N
    print(f"(a) N = {B} x {HH} x {WW} = {N} rows")
    hr, flow = torch.randn(N, 64, device="cuda") * 0.1, torch.randn(N, 4, device="cuda")
    x = {k: torch.empty(N, w, device="cuda") for k, w in (("x1", 208), ("x2", 264), ("x3", 528))}
    gx = {k: torch.randn(N, w, device="cuda") for k, w in (("x1", 208), ("x2", 264), ("x3", 528))}
    r = {"x1_fwd": lambda: ops.dec_x1_fwd(geom, x["x1"]), "x1_bwd": lambda: ops.dec_x1_bwd(geom, gx["x1"]),
         "x2_fwd": lambda: ops.dec_x2_fwd(geom, hr, x["x2"]), "x2_bwd": lambda: ops.dec_x2_bwd(geom, gx["x2"]),
         "x3_fwd": lambda: ops.dec_x3_fwd(geom, hr, flow, x["x3"]),
         "x3_bwd": lambda: ops.dec_x3_bwd(geom, hr, flow, gx["x3"])}
    if a.deterministic:   # the ordered adjoint, alternated with the atomic one
        r["x3_bwd deterministic"] = lambda: ops.dec_x3_bwd(geom, hr, flow, gx["x3"], deterministic=True)
    r = timed(r, a.rounds, a.warmup)
    lr = lat.numel()
    for k, nbytes in (("x1_fwd", 4.0 * (N * 208 + lr)), ("x1_bwd", 4.0 * (N * 192 + lr)),
                      ("x2_fwd", 4.0 * (N * (264 + 64) + lr)), ("x2_bwd", 4.0 * (N * (256 + 64) + lr)),
                      ("x3_fwd", 4.0 * (N * (528 + 64 + 4) + lr)), ("x3_bwd", 4.0 * (N * (528 + 2 * 64 + 8) + 2 * lr))):
        m = show(f"(a) dec_{k}", r[k])
        print(" " * 60 + rate(nbytes, m) + " (unique bytes; gathers re-read through the caches)")
    if a.deterministic:
        m = show("(a) dec_x3_bwd deterministic (contrib, 2 sorts, 2 segsums)", r["x3_bwd deterministic"])
        print(" " * 60 + f"deterministic / atomic medians = {m / statistics.median(r['x3_bwd']):.2f}x")
    for net, (cin, hidden, cout) in NETS.items():
        mod = T.Siren(cin, hidden, cout).cuda()
        ps = [p.detach() for p in mod._params()]
        nl = len(ps) // 2
        xin = x["x1" if cin == 201 else "x2" if cin == 263 else "x3"]
        xin.normal_()
        xin[:, cin:] = 0
        y, z = ops.siren_fwd(xin, ps[:nl], ps[nl:])
        gy = torch.randn_like(y)
        gxb = torch.empty_like(xin)
        ws = torch.empty(L.lib().stif_siren_bwd_workspace_size(N, len(hidden)) // 4, device="cuda")
        r = timed({"fwd": lambda: ops.siren_fwd(xin, ps[:nl], ps[nl:], y, z),
                   "bwd": lambda: ops.siren_bwd(xin, z, ps[:nl], ps[nl:], gy, g_x=gxb, workspace=ws)}, a.rounds, a.warmup)
        macs = sum(p.numel() for p in ps[:nl])
        m = show(f"(a) siren_fwd {net}", r["fwd"])
        print(" " * 60 + mfma_share(2.0 * macs * N, m))
        m = show(f"(a) siren_bwd {net}, g_x and every weight gradient", r["bwd"])
        print(" " * 60 + mfma_share(4.0 * macs * N, m))


def torch_decoder(P, feat, inp, t, HH, WW):
    """The decoder in torch ops (fp32): what autograd differentiates in section (b)."""
    def siren(x, p, n):
        for i in range(n):
            x = torch.sin(30.0 * F.linear(x, P[f"{p}.net.{i}.linear.weight"], P[f"{p}.net.{i}.linear.bias"]))
        return F.linear(x, P[f"{p}.net.{n}.weight"], P[f"{p}.net.{n}.bias"])

    def sample(img, grid, mode):
        return F.grid_sample(img, grid.unsqueeze(1), mode=mode, align_corners=False)[:, :, 0, :].permute(0, 2, 1)

    lo, hi = -1 + 1e-6, 1 - 1e-6
    featc, inpc = feat.reshape(B, 192, H, W), inp.reshape(B, 6, H, W)
    ys = ((torch.arange(HH, device="cuda").float() * 2 + 1) / HH - 1).clamp(lo, hi)
    xs = ((torch.arange(WW, device="cuda").float() * 2 + 1) / WW - 1).clamp(lo, hi)
    grid = torch.stack([xs[None, :].expand(HH, WW), ys[:, None].expand(HH, WW)], -1).reshape(1, -1, 2).expand(B, -1, 2)
    ly = (torch.arange(H, device="cuda").float() * 2 + 1) / H - 1
    lx = (torch.arange(W, device="cuda").float() * 2 + 1) / W - 1
    coord = torch.stack([ly[:, None].expand(H, W), lx[None, :].expand(H, W)], 0)[None].expand(B, 2, H, W)
    rel = grid.flip(-1) - sample(coord, grid, "nearest")
    rel = rel * torch.tensor([H, W], device="cuda", dtype=torch.float32)
    pe = torch.full((B, HH * WW, 1), t, device="cuda")
    hrfeat = siren(torch.cat([sample(featc, grid, "nearest"), sample(inpc, grid, "nearest"), rel, pe], -1), "feat_imnet", 3)
    flow = siren(torch.cat([hrfeat, sample(featc, grid, "bilinear"), sample(inpc, grid, "bilinear"), pe], -1),
                 "flow_imnet", 3)
    hr_img = hrfeat.permute(0, 2, 1).reshape(B, 64, HH, WW)
    bx = torch.linspace(-1, 1, WW, device="cuda")[None, :].expand(HH, WW).reshape(1, -1)
    by = torch.linspace(-1, 1, HH, device="cuda")[:, None].expand(HH, WW).reshape(1, -1)
    grids = [torch.stack([bx + flow[..., 2 * k] / ((WW - 1.0) / 2.0), by + flow[..., 2 * k + 1] / ((HH - 1.0) / 2.0)],
                         -1).clamp(lo, hi) for k in range(2)]
    x3 = torch.cat([sample(hr_img, g, "bilinear") for g in grids] + [sample(featc, g, "bilinear") for g in grids]
                   + [sample(inpc, g, "bilinear") for g in grids] + [pe], -1)
    return siren(x3, "encode_imnet", 4).permute(0, 2, 1).reshape(B, 3, HH, WW)


def bench_decoder(a):
    """(b)"""
    feat, inp, HH, WW = inputs(a)
    feat.requires_grad_(True)
    torch.manual_seed(1)
    dec = T.Decoder().cuda()
    P = {k: v.detach().clone().requires_grad_(True) for k, v in dec.named_parameters()}
    gout = torch.randn(B, 3, HH, WW, device="cuda")

    def engine():
        for p in dec.parameters():
            p.grad = None
        feat.grad = None
        dec(feat, inp, [0.5], (HH, WW))[0].backward(gout)

    def autograd():
        for p in P.values():
            p.grad = None
        feat.grad = None
        torch_decoder(P, feat, inp, 0.5, HH, WW).backward(gout)

    with torch.no_grad():
        d = (dec(feat, inp, [0.5], (HH, WW))[0] - torch_decoder(P, feat, inp, 0.5, HH, WW)).abs().max()
    print(f"(b) max |engine - torch| of the forward: {float(d):.2e}")
    def engine_det():
        with T.deterministic():
            engine()

    fns = {"engine": engine, "torch": autograd}
    if a.deterministic:
        fns["engine deterministic"] = engine_det
    r = timed(fns, a.rounds, a.warmup)
    me = show(f"(b) train.Decoder forward + backward, {B}x{HH}x{WW}", r["engine"])
    if a.deterministic:
        md = show("(b) the same under train.deterministic()", r["engine deterministic"])
        print(" " * 60 + f"deterministic / atomic medians = {md / me:.2f}x")
    mt = show("(b) the same decoder by torch autograd (fp32)", r["torch"])
    print(" " * 60 + f"torch / engine = {mt / me:.2f}")
    torch.cuda.reset_peak_memory_stats()
    engine()
    torch.cuda.synchronize()
    pe = torch.cuda.max_memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    autograd()
    torch.cuda.synchronize()
    print(f"(b) peak allocated bytes of one step: engine {pe / 2**30:.2f} GiB, torch autograd "
          f"{torch.cuda.max_memory_allocated() / 2**30:.2f} GiB ({pe / (B * HH * WW) / 1024:.1f} KiB per HR pixel on "
          "the engine, the inputs included)")


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
    if kind[0] in ("siren_fwd", "siren_bwd"):
        return f"stif_{kind[0]} {kind[1]} -> {kind[2]}"
    if kind[0].startswith("dec_x"):
        return "stif_" + kind[0]
    if kind[0] == "segsum":
        return f"stif_segsum C {kind[1]}"
    return "gen_feat: " + {"wino": "stif_conv3x3_wino", "conv": "stif_conv2d_nhwc", "wgrad": "stif_conv3x3_wgrad",
                           "wgrad_cat": "stif_conv3x3_wgrad_cat", "dcn": "stif_dcn_nhwc",
                           "dcn_bwd": "stif_dcn_bwd_nhwc", "dcn_bwd_contrib": "stif_dcn_bwd_contrib"}.get(kind[0], kind[0])


def bench_step(a):
    """(c)"""
    g = torch.Generator().manual_seed(0)
    x = torch.rand(B, 2, 3, H, W, generator=g).cuda()
    HH, WW = a.scale * H, a.scale * W
    gt = torch.rand(B, 1, 3, HH, WW, generator=g).cuda()
    torch.manual_seed(1)
    net = T.LunaTokis(5, 40, "f16x3").cuda()
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, T.DCN_sep):
                m.conv_offset_mask.weight.normal_(0, 0.01)
    crit = T.TimesLoss(T.CharbonnierLoss())

    def step():
        for p in net.parameters():
            p.grad = None
        crit(net(x, [0.5], (HH, WW)), gt).backward()

    def det_step():
        with T.deterministic():
            step()

    fns = {"step": step}
    if a.deterministic:
        fns["deterministic"] = det_step
    r = timed(fns, a.rounds, a.warmup)
    ms = show(f"(c) train.LunaTokis f16x3 forward + loss + backward, {B}x2x3x{H}x{W} -> {HH}x{WW}", r["step"])
    if a.deterministic:
        md = show("(c) the same step under train.deterministic()", r["deterministic"])
        print(" " * 60 + f"deterministic / atomic medians = {md / ms:.2f}x")
    print(f"(c) range_status {net.range_status()}")
    per, whole = defaultdict(list), []
    for _ in range(max(3, a.rounds // 3)):
        tr = Tracer()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ops.TRACE = tr
        try:
            e0.record()
            (det_step if a.deterministic else step)()
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
    print(f"(c) split of one traced {'deterministic ' if a.deterministic else ''}step (events around every call): {wm:9.1f} us", flush=True)
    for k, us in sorted(per.items(), key=lambda kv: -statistics.median(kv[1])):
        m = statistics.median(us)
        print(f"      {k:56s} {m:9.1f} us  {100 * m / wm:5.1f} %", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scale", type=int, default=2, help="HR size = scale x 128 (the reference trains at 1..4)")
    ap.add_argument("--only", choices=["kernels", "decoder", "step"])
    ap.add_argument("--deterministic", action="store_true",
                    help="add the ordered-sum paths (ops.dec_x3_bwd(deterministic=True), train.deterministic()) beside "
                         "the atomic ones in every section; the traced step of (c) is then the deterministic one")
    a = ap.parse_args()
    print(f"device: {torch.cuda.get_device_name(0)}, rounds {a.rounds}, warm-up {a.warmup}, scale x{a.scale}")
    for name, fn in (("kernels", bench_kernels), ("decoder", bench_decoder), ("step", bench_step)):
        if a.only in (None, name):
            fn(a)
