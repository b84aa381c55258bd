"""Time what data-parallel training adds to a step on one GPU: the gradient arena's two kernels
on the full model's real layout, and a DataParallel step at world 1 against optimize_step.

The layout is train.LunaTokis(5, 40)'s after one real backward: the 434 gradient tensors autograd allocated, N floats
in the arena.  Device events around warmed-up loops, the arms alternating within every round, the median of the rounds:

  grad_pack           GradArena.pack(): 434 tensors -> the arena, one launch, with the host work of a step (434
                      .grad reads, checks and pointer comparisons; the table's pointers are already uploaded)
  stif_grad_pack      the launch alone through the C ABI on the resident table: the kernel's own time
  torch.cat           the same movement with torch: torch.cat([g.reshape(-1) for g in grads]) (no 4-float rounding)
  rank_sum R          stif_rank_sum over a [R, N] slab into the arena, R = 2 and 8
  slab.sum(0) R       the same reduction with torch (its own order of addition)
  step                train.DataParallel(world 1).step against train.optimize_step on the same batch from the same
                      weights, each with its own net and Adam, alternating; host clock around a synchronised step

Every arm is also timed on the host without a device wait: where that is the larger number the arm is bound by Python,
and the device column shows the host's pace, not the kernel's.  Bytes are counted from the shapes: grad_pack reads
4 N and writes 4 N (rounded), rank_sum reads 4 R N and writes 4 N.
Not measured here: several GPUs (RCCL all-gather / all-reduce time and scaling), and overlap of the exchange with the
backward, which is not built.

  python tools/bench_ddp.py [--iters 20] [--reps 9] [--steps 20] [--batch 2] [--lq 32]
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


def make(stif):
    TR = stif.train
    net = TR.LunaTokis(5, 40)
    sd = stif.weights.make_state_dict(seed=0)
    net.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in sd.items()}, strict=True)
    net = net.cuda()
    opt, _ = TR.make_optimizer(net, dict(lr_G=1e-4, beta1=0.9, beta2=0.99, lr_scheme="MultiStepLR", lr_steps=[10 ** 9],
                                         lr_gamma=0.5))
    return net, opt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--lq", type=int, default=32)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_ddp needs the GPU"
    stif = stif_pkg.load()
    TR, ops = stif.train, stif.ops
    crit = TR.TimesLoss(TR.CharbonnierLoss())
    B, lq = a.batch, a.lq
    g = torch.Generator().manual_seed(0)
    x = torch.rand(B, 2, 3, lq, lq, generator=g).cuda()
    gt = torch.rand(B, 3, 3, 4 * lq, 4 * lq, generator=g).cuda()
    times = [torch.full((B, 1), t) for t in (0.125, 0.5, 0.875)]
    inputs = (x, times, (4 * lq, 4 * lq))

    # ---- the kernels on the real layout
    net, opt = make(stif)
    crit(net(*inputs), gt).backward()
    arena = TR.GradArena([(k, p) for k, p in net.named_parameters() if p.grad is not None])
    grads, N = arena.grads(), arena.arena.numel()
    print(f"layout: {len(grads)} gradient tensors of {len(list(net.parameters()))} parameters, {sum(arena.sizes)} floats, "
          f"arena {N} floats ({4 * N / 2 ** 20:.1f} MiB), smallest tensor {min(arena.sizes)}, largest {max(arena.sizes)}")
    arena.pack()
    flat = torch.cat([t.reshape(-1) for t in grads])
    views = arena.views()
    assert all(torch.equal(v, t) for v, t in zip(views, grads)), "grad_pack moved the gradients bit for bit"
    slabs = {R: torch.randn(R, N, device="cuda", generator=torch.Generator(device="cuda").manual_seed(R)) for R in (2, 8)}
    dst = torch.empty(N, device="cuda")
    L, lib = stif._lib, stif._lib.lib()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    tab, nseg, base = arena.table.dev.data_ptr(), len(grads), arena.arena.data_ptr()

    def pack_alone():
        L.check(lib.stif_grad_pack(tab, nseg, base, N, st), "stif_grad_pack")

    arms = {"grad_pack": lambda: arena.pack(), "stif_grad_pack": pack_alone,
            "torch.cat": lambda: torch.cat([t.reshape(-1) for t in grads])}
    for R, slab in slabs.items():
        arms[f"rank_sum R={R}"] = lambda slab=slab: ops.rank_sum(slab, dst)
        arms[f"slab.sum(0) R={R}"] = lambda slab=slab: slab.sum(0)
    res = timed_interleaved(arms, a.iters, a.reps)
    moved = {"grad_pack": 8.0 * N, "stif_grad_pack": 8.0 * N, "torch.cat": 8.0 * flat.numel()}
    for R in slabs:
        moved[f"rank_sum R={R}"] = moved[f"slab.sum(0) R={R}"] = 4.0 * (R + 1) * N
    for name, (med, lo, hi) in res.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.iters):
            arms[name]()
        host = (time.perf_counter() - t0) * 1e6 / a.iters
        torch.cuda.synchronize()
        print(f"  {name:18s}: {med:9.1f} us (min {lo:.1f}, max {hi:.1f})  {moved[name] / med / 1e3:7.1f} GB/s, "
              f"host {host:7.1f} us to issue")
    del slabs, dst, flat

    # ---- the step at world 1 against optimize_step
    net_b, opt_b = make(stif)
    dp = TR.DataParallel(net_b, opt_b)
    step_arms = {"optimize_step": lambda: TR.optimize_step(net, opt, crit, inputs, gt),
                 "DataParallel.step": lambda: dp.step(crit, inputs, gt)}
    t = {k: [] for k in step_arms}
    for k in range(a.steps + 2):
        for name, fn in step_arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if k >= 2:
                t[name].append((time.perf_counter() - t0) * 1e3)
    same = all(torch.equal(p, q) for p, q in zip(net.parameters(), net_b.parameters()))
    print(f"step at batch {B}, LQ {lq} x {lq} -> {4 * lq} x {4 * lq}, 3 times, {a.steps} timed steps each, alternating "
          f"(atomic backward: parameters equal bit for bit afterwards: {same})")
    for name, v in t.items():
        print(f"  {name:18s}: median {statistics.median(v):8.2f} ms (min {min(v):.2f}, max {max(v):.2f})")
    ratio = statistics.median(t["DataParallel.step"]) / statistics.median(t["optimize_step"])
    print(f"  DataParallel.step / optimize_step = {ratio:.3f}")
    print(f"  range status {dp.range_status()}")


if __name__ == "__main__":
    main()
