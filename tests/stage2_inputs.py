"""Seeded inputs that take decoder stage 2 out of the near-identity regime (shared by tests/test_oracle.py and
tests/test_gpu_decoder_stages.py; a plain module, not a fixture): flows of several HR pixels, flows clamped at the
frame edge, integer flows, and flows whose warped grid lands on the clamp value +-(1 - 1e-6) or one fp32 ulp inside
it.  Everything is fp32, so the kernel and the oracle read the same values."""
import numpy as np

F32 = np.float32
KINDS = ["uniform", "huge", "integer", "edge"]
LO, HI = F32(-1.0) + F32(1e-6), F32(1.0) - F32(1e-6)              # the decoder's clamp (Sakuya_arch_test.py:428,441)
LO_IN, HI_IN = np.nextafter(LO, F32(0)), np.nextafter(HI, F32(0))  # one fp32 ulp inside it


def linspace_f32(n):
    """torch.linspace(-1, 1, n) in fp32 (warplayer.py:27-30; the oracle's and coords' linspace_f32)."""
    step = F32(2.0 / (n - 1))
    i = np.arange(n)
    lo = (F32(-1.0) + step * i.astype(F32)).astype(F32)
    hi = (F32(1.0) - step * (n - 1 - i).astype(F32)).astype(F32)
    return np.where(i < n // 2, lo, hi).astype(F32)


def warped_grid_f32(flow, HH, WW):
    """Stage 2's unclamped grids in the kernel's fp32 arithmetic: base + flow / ((n - 1) / 2), [B,HH,WW,4]
    (x1, y1, x2, y2)."""
    dx, dy = (F32(WW) - F32(1)) / F32(2), (F32(HH) - F32(1)) / F32(2)
    base = np.empty((1, HH, WW, 4), F32)
    base[..., 0::2] = linspace_f32(WW)[None, None, :, None]
    base[..., 1::2] = linspace_f32(HH)[None, :, None, None]
    d = np.array([dx, dy, dx, dy], F32)
    return (base + (flow / d).astype(F32)).astype(F32), base, d


def _edge(rng, f, HH, WW):
    """A third of the entries of ``f`` aimed at the clamp: the fp32 grid lands exactly on +-(1 - 1e-6), one ulp
    inside it, or a few ulps outside it (and is clamped onto it).  The flow that does it is searched among the
    fp32 neighbours of (target - base) * d; entries with none keep a flow one pixel past the target (clamped)."""
    _, base, d = warped_grid_f32(f, HH, WW)
    base = np.broadcast_to(base, f.shape)
    d = np.broadcast_to(d, f.shape)
    pick = rng.random(f.shape) < 1 / 3
    targets = np.array([HI, HI_IN, np.nextafter(np.nextafter(HI, F32(2)), F32(2)),
                        LO, LO_IN, np.nextafter(np.nextafter(LO, F32(-2)), F32(-2))], F32)
    tgt = targets[rng.integers(0, len(targets), f.shape)]
    f0 = ((tgt - base) * d).astype(F32)
    out = (f0 + np.sign(tgt)).astype(F32)                           # the fallback: a pixel outside, clamped
    found = np.zeros(f.shape, bool)
    up, dn = f0, f0
    for _ in range(17):
        for cand in (up, dn):
            hit = ((base + (cand / d).astype(F32)).astype(F32) == tgt) & ~found
            out[hit] = cand[hit]
            found |= hit
        up, dn = np.nextafter(up, F32(np.inf)), np.nextafter(dn, F32(-np.inf))
    f = f.copy()
    f[pick] = out[pick]
    return f


def flows(kind, B, HH, WW, seed=5):
    """[B,HH,WW,4] fp32 flows in HR pixels (x1, y1, x2, y2)."""
    rng = np.random.default_rng(seed)
    f = rng.uniform(-3.5, 3.5, (B, HH, WW, 4)).astype(F32)
    if kind == "uniform":
        return f
    if kind == "huge":                                               # as synthetic_flow of test_gpu_window.py
        f[rng.random(f.shape) < 0.1] = F32(1e4)
        f[rng.random(f.shape) < 0.1] = F32(-1e4)
        return f
    if kind == "integer":                                            # bilinear weights exactly 0 or 1
        return np.rint(f).astype(F32)
    if kind == "edge":
        return _edge(rng, f, HH, WW)
    raise ValueError(kind)


def hrfeat(B, HH, WW, seed=11):
    """[B,HH,WW,64] fp32, U(-0.5, 0.5)."""
    return (np.random.default_rng(seed).random((B, HH, WW, 64), dtype=F32) - F32(0.5)).astype(F32)


def latent(B, H, W, seed=13):
    """A random latent [B,3,64,H,W] = 0.5 N(0,1) and frame pair [B,2,3,H,W] = U(0,1), fp32."""
    rng = np.random.default_rng(seed)
    return (F32(0.5) * rng.standard_normal((B, 3, 64, H, W), dtype=F32)).astype(F32), rng.random((B, 2, 3, H, W), dtype=F32)


def bound_ratio(got, ref, rtol=1e-4, atol=1e-6):
    """|got - ref| / (rtol |ref| + atol) elementwise: the project's oracle tolerance holds where it is <= 1."""
    ref = np.asarray(ref, np.float64)
    return np.abs(np.asarray(got, np.float64) - ref) / (rtol * np.abs(ref) + atol)
