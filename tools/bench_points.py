"""Point-query microbenchmark: the benchmark's C0 latent (7 frames of 128 x 128, six pairs) decoded on the 512 x 512
grid at N random points per item, each at its own time (model.decoding_points), against the two ways the same values
are obtained without point queries: the full decode followed by an index, and decoding(window=) of a square with the
same pixel count.  Device events around each call, WARM warm-up rounds, then REPS rounds that alternate the three
(so drift hits them alike); per line the median and the spread (min .. max) over the rounds.
PARENT=<checkout of another commit with its library built>: the full decode and the window are measured on that
checkout's package and library, in this process, on its own latent of the same frames.
ENSEMBLE=1: the three ways with the local ensemble -- decoding_points(ensemble=True), the full ensemble decode
followed by an index, and decoding(window=, ensemble=True) of equal pixel count."""
import importlib.util
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import stif_pkg  # noqa: E402
import bench  # noqa: E402

PKG = "stif-continuous-video-representation_amd"
counts = [int(v) for v in os.environ.get("N", "256,4096,65536").split(",")]
reps, warm = int(os.environ.get("REPS", "7")), int(os.environ.get("WARM", "2"))
mode = os.environ.get("MFMA", "f16x3")
ens = os.environ.get("ENSEMBLE", "0") not in ("", "0")
kw = dict(ensemble=True) if ens else {}
stif = stif_pkg.load()
base, base_name = stif, "this tree"
if os.environ.get("PARENT"):
    d = os.path.join(os.path.abspath(os.environ["PARENT"]), PKG)
    spec = importlib.util.spec_from_file_location("stif_parent", os.path.join(d, "__init__.py"),
                                                  submodule_search_locations=[d])
    base = importlib.util.module_from_spec(spec)
    sys.modules["stif_parent"] = base
    spec.loader.exec_module(base)
    base_name = os.environ["PARENT"]
dev = torch.device("cuda", 0)
nframes, H, W, _, _, _ = bench.CONFIGS["c0"]
HH, WW = 4 * H, 4 * W
sd = stif.weights.make_state_dict(seed=0)
frames = bench.synth_frames(0, nframes, H, W, dev)


def latent(pkg):
    m = pkg.LunaTokis(64, 6, 8, 5, 40, device=dev, mfma=mode)
    m.load_state_dict(sd, strict=True)
    with torch.no_grad():
        m.gen_feat_window(frames)
    return m


model = latent(stif)
parent = model if base is stif else latent(base)
B = nframes - 1
tq = [torch.tensor([[0.5]], device=dev)]


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def line(name, ms):
    print(f"  {name:{46 if ens else 34}s} {statistics.median(ms):9.3f} ms   ({min(ms):.3f} .. {max(ms):.3f})", flush=True)


print(f"C0 latent, {B} items, grid {HH} x {WW}, {mode}{', local ensemble' if ens else ''}; full decode and window "
      f"on: {base_name}", flush=True)
with torch.no_grad():
    for n in counts:
        g = torch.Generator(device=dev).manual_seed(n)
        y = torch.randint(0, HH, (B, n), device=dev, dtype=torch.int32, generator=g)
        x = torch.randint(0, WW, (B, n), device=dev, dtype=torch.int32, generator=g)
        t = torch.rand(B, n, device=dev, generator=g)
        yl, xl = y.long(), x.long()
        side = int(round(n ** 0.5))
        win = ((HH - side) // 2, (WW - side) // 2, side, n // side)
        def full_index():
            o = parent.decoding(tq, **kw)[0]
            return torch.stack([o[b][:, yl[b], xl[b]] for b in range(B)])

        e = ", ensemble=True" if ens else ""
        ways = {
            f"decoding_points({e[2:]})" if ens else "decoding_points": lambda: model.decoding_points(y, x, t, **kw),
            f"full {'ensemble ' if ens else ''}decode + index": full_index,
            f"decoding(window={win[2]}x{win[3]}{e})": lambda: parent.decoding(tq, window=win, **kw),
        }
        ms = {k: [] for k in ways}
        for r in range(warm + reps):
            for k, fn in ways.items():
                v = timed(fn)
                if r >= warm:
                    ms[k].append(v)
        print(f"n = {n} points per item ({100.0 * n / (HH * WW):.2f} % of the grid)", flush=True)
        for k, v in ms.items():
            line(k, v)
