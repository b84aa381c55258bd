"""stif_yuv_to_rgb / stif_rgb_to_yuv on the GPU against a float64 numpy restatement of the formulas of
include/stif.h (stif_yuv_format): shapes with odd edges and partial chroma boxes, every depth family, both matrices
and ranges, strided RGB on either side, and the argument validation."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

#         chroma     depth  W    H
SHAPES = [("420jpeg", 8, 13, 11), ("420jpeg", 10, 16, 8), ("422", 10, 14, 9), ("444", 8, 5, 3), ("420jpeg", 16, 2, 2),
          ("420jpeg", 16, 1, 1), ("420jpeg", 8, 130, 67)]                 # the last one crosses a workgroup
IDS = [f"{c}-{d}bit-{w}x{h}" for c, d, w, h in SHAPES]
COLOURS = [("bt601", False), ("bt601", True), ("bt709", False), ("bt709", True)]
N = 2


# ----------------------------------------------------------------------------- float64 reference
def coeffs(fmt):
    kr, kb = (0.2126, 0.0722) if fmt.matrix == "bt709" else (0.299, 0.114)
    up = 2.0 ** (fmt.depth - 8)
    maxv = 2.0 ** fmt.depth - 1
    if fmt.full_range:
        return kr, 1 - kr - kb, kb, 0.0, maxv, maxv, 128 * up, maxv
    return kr, 1 - kr - kb, kb, 16 * up, 219 * up, 224 * up, 128 * up, maxv


def upsample(c, sub, size):
    """one axis (the first) of a chroma plane: sample k sits at the centre of luma pixels 2k, 2k + 1"""
    if not sub:
        return c
    p = np.arange(size)
    k = p >> 1
    o = np.clip(k + np.where(p & 1, 1, -1), 0, c.shape[0] - 1)
    return 0.75 * c[k] + 0.25 * c[o]


def ref_to_rgb(fmt, y, u, v, clamp=True):
    kr, kg, kb, yoff, yrange, crange, coff, _ = coeffs(fmt)
    H, W = fmt.height, fmt.width
    full = [upsample(upsample(c.astype(np.float64), fmt.sub_y, H).T, fmt.sub_x, W).T for c in (u, v)]
    yy = (y.astype(np.float64) - yoff) / yrange
    cb, cr = (full[0] - coff) / crange, (full[1] - coff) / crange
    r = yy + 2 * (1 - kr) * cr
    b = yy + 2 * (1 - kb) * cb
    g = (yy - kr * r - kb * b) / kg
    rgb = np.stack([r, g, b])
    return np.clip(rgb, 0, 1) if clamp else rgb


def box_mean(c, sub_y, sub_x):
    """mean over the pixels of each chroma box that exist (partial boxes at odd edges)"""
    for axis, sub in ((0, sub_y), (1, sub_x)):
        if sub:
            n = c.shape[axis]
            even, odd = c.take(range(0, n, 2), axis), c.take(range(1, n, 2), axis)
            if n & 1:
                last = even.take([-1], axis)
                c = np.concatenate([(even.take(range(n // 2), axis) + odd) / 2, last], axis)
            else:
                c = (even + odd) / 2
    return c


def ref_to_yuv(fmt, rgb):
    """(pre-rounding float64 planes, quantised integer planes) of one frame [3, H, W]"""
    kr, kg, kb, yoff, yrange, crange, coff, maxv = coeffs(fmt)
    r, g, b = np.clip(rgb.astype(np.float64), 0, 1)
    yy = kr * r + kg * g + kb * b
    cb, cr = (b - yy) / (2 * (1 - kb)), (r - yy) / (2 * (1 - kr))
    pre = [yoff + yrange * yy, coff + crange * box_mean(cb, fmt.sub_y, fmt.sub_x),
           coff + crange * box_mean(cr, fmt.sub_y, fmt.sub_x)]
    return pre, [np.clip(np.rint(p), 0, maxv).astype(np.int64) for p in pre]      # np.rint: half to even


def random_frames(fmt, seed):
    """N frame payloads with samples over the whole 0 .. 2^depth - 1 span (outside the nominal range too)"""
    rng = np.random.default_rng(seed)
    cw, ch = fmt.chroma_size
    planes = [[rng.integers(0, 2 ** fmt.depth, s) for s in ((fmt.height, fmt.width), (ch, cw), (ch, cw))]
              for _ in range(N)]
    dt = "<u2" if fmt.depth > 8 else np.uint8
    raw = np.stack([np.concatenate([p.astype(dt).reshape(-1).view(np.uint8) for p in fr]) for fr in planes])
    assert raw.shape == (N, fmt.frame_bytes)
    return planes, torch.from_numpy(raw).cuda()


def unpack(fmt, out):
    return [[p.astype(np.int64) for p in fmt.planes(fr)] for fr in out.cpu().numpy()]


def make(stif, chroma, depth, W, H, matrix="bt601", full=False):
    return stif.y4m.YuvFormat(W, H, chroma, depth, matrix, full)


# ----------------------------------------------------------------------------- yuv -> rgb
# fp32 error budget: about a dozen roundings on magnitudes below 2 -> 12 * 2 * 6e-8 ~ 1.5e-6
ATOL = 2e-6
CASES = [s + c for s in SHAPES[:1] for c in COLOURS] + [s + COLOURS[0] for s in SHAPES[1:]]
CASE_IDS = [f"{c}-{d}bit-{w}x{h}-{m}-{'full' if f else 'limited'}" for c, d, w, h, m, f in CASES]


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_yuv_to_rgb_matches_float64(stif, case):
    fmt = make(stif, *case)
    planes, dev = random_frames(fmt, 11)
    want = np.stack([ref_to_rgb(fmt, *fr) for fr in planes])
    got = stif.ops.yuv_to_rgb(dev, fmt)
    assert got.shape == (N, 3, fmt.height, fmt.width) and got.dtype == torch.float32
    err = float(np.abs(got.cpu().numpy().astype(np.float64) - want).max())
    print(f"max |gpu - fp64| = {err:.3e}")
    assert err <= ATOL
    assert float(got.min()) >= 0.0 and float(got.max()) <= 1.0
    # through strides into a padded tensor: the same values, and not one bit outside the frame is touched
    hn, wn = 4 * -(-fmt.height // 4) + 4, 4 * -(-fmt.width // 4)
    pad = torch.full((N, 3, hn, wn), -7.0, device="cuda")
    assert stif.ops.yuv_to_rgb(dev, fmt, out=pad) is pad
    assert torch.equal(pad[:, :, :fmt.height, :fmt.width], got)
    pad[:, :, :fmt.height, :fmt.width] = -7.0
    assert bool((pad == -7.0).all())
    # three plane views of one buffer instead of the frame bytes
    cw, ch = fmt.chroma_size
    b = fmt.bytes_per_sample
    ny, nc = fmt.height * fmt.width * b, ch * cw * b
    views = (dev[:, :ny].view(N, fmt.height, fmt.width * b), dev[:, ny:ny + nc].view(N, ch, cw * b),
             dev[:, ny + nc:].view(N, ch, cw * b))
    assert torch.equal(stif.ops.yuv_to_rgb(views, fmt), got)


# ----------------------------------------------------------------------------- rgb -> yuv
@pytest.mark.parametrize("depth", [8, 10, 16])
@pytest.mark.parametrize("matrix, full", COLOURS)
def test_rgb_to_yuv_in_gamut_is_exact(stif, depth, matrix, full):
    """RGB that decodes from integer samples E must encode to exactly E: the pre-rounding values sit within the
    arithmetic's error of integers, far from any tie."""
    fmt = make(stif, "444", depth, 5, 3, matrix, full)
    rng = np.random.default_rng(3)
    E = [ref_to_yuv(fmt, rng.uniform(0.1, 0.9, (3, 3, 5)))[1] for _ in range(N)]
    rgb = np.stack([ref_to_rgb(fmt, *e, clamp=False) for e in E])
    assert rgb.min() > 0 and rgb.max() < 1                                # in gamut: the clamp does nothing
    out = stif.ops.rgb_to_yuv(torch.from_numpy(rgb.astype(np.float32)).cuda(), fmt)
    for got, want in zip(unpack(fmt, out), E):
        assert all(np.array_equal(g, w) for g, w in zip(got, want))


def tie_check(fmt, rgb, out):
    worst = 0.0
    for fr, got in zip(rgb, unpack(fmt, out)):
        pre, want = ref_to_yuv(fmt, fr)
        for p, w, g in zip(pre, want, got):
            assert g.shape == w.shape
            d = g != w
            assert np.abs(g - w).max() <= 1
            if d.any():                                                   # only genuine ties may round the other way
                off = np.abs(np.abs(p[d] - np.floor(p[d])) - 0.5)
                worst = max(worst, float(off.max()))
                assert off.max() < 1e-3, (p[d], g[d], w[d])
    return worst


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_rgb_to_yuv_differs_only_at_ties(stif, case):
    fmt = make(stif, *case)
    rng = np.random.default_rng(17)
    rgb = rng.uniform(-0.2, 1.2, (N, 3, fmt.height, fmt.width)).astype(np.float32)
    out = stif.ops.rgb_to_yuv(torch.from_numpy(rgb).cuda(), fmt)
    assert out.shape == (N, fmt.frame_bytes) and out.dtype == torch.uint8
    print("largest distance from a tie among differing samples:", tie_check(fmt, rgb, out))


@pytest.mark.parametrize("case", [SHAPES[0], SHAPES[2], SHAPES[6]], ids=[IDS[0], IDS[2], IDS[6]])
def test_rgb_to_yuv_strided_crop(stif, case):
    """The top-left crop of a larger tensor, converted in place, gives the bytes of its contiguous copy."""
    fmt = make(stif, *case)
    big = torch.rand(N, 3, fmt.height + 3, fmt.width + 5, generator=torch.Generator().manual_seed(9)).cuda() * 1.4 - 0.2
    crop = big[:, :, :fmt.height, :fmt.width]
    assert not crop.is_contiguous()
    a = stif.ops.rgb_to_yuv(crop, fmt)
    assert torch.equal(a, stif.ops.rgb_to_yuv(crop.contiguous(), fmt))
    assert tie_check(fmt, crop.cpu().numpy(), a) < 1e-3
    # into plane views of a pitched buffer: the same samples, the gaps untouched
    cw, ch = fmt.chroma_size
    b = fmt.bytes_per_sample
    py, pc = fmt.width * b + 6, cw * b + 2
    buf = torch.full((N, fmt.height * py + 2 * ch * pc + 8,), 0xAB, dtype=torch.uint8, device="cuda")
    oy, ou, ov = 0, fmt.height * py, fmt.height * py + ch * pc
    views = tuple(buf[:, o:o + r * p].view(N, r, p)[:, :, :rb] for o, r, p, rb in
                  ((oy, fmt.height, py, fmt.width * b), (ou, ch, pc, cw * b), (ov, ch, pc, cw * b)))
    stif.ops.rgb_to_yuv(crop, fmt, out=views)
    ny, nc = fmt.height * fmt.width * b, ch * cw * b
    for v, (lo, hi) in zip(views, ((0, ny), (ny, ny + nc), (ny + nc, ny + 2 * nc))):
        assert torch.equal(v.reshape(N, -1), a[:, lo:hi])
        v.fill_(0xAB)
    assert bool((buf == 0xAB).all())


# ----------------------------------------------------------------------------- validation
def test_bad_arguments_are_rejected_before_any_launch(stif):
    """Return code and message only; every pointer handed over is a real 1 MiB device buffer, far larger than
    anything an 8 x 4 frame addresses."""
    L = stif._lib
    lib = L.lib()
    bufs = [torch.zeros(1 << 20, dtype=torch.uint8, device="cuda") for _ in range(4)]
    y, u, v, rgb = [b.data_ptr() for b in bufs]

    def fmt(**kw):
        f = L.YuvFormat(8, 4, 1, 1, 8, L.YUV_BT601, 0)
        for k, val in kw.items():
            setattr(f, k, val)
        return f

    def both(f, n=1, y=y, u=u, v=v, rgb=rgb, strides=(0, 0, 0)):
        fp = C.byref(f) if f is not None else None
        rcs = [lib.stif_yuv_to_rgb(fp, y, u, v, n, rgb, *strides, None)]
        msg = lib.stif_last_error()
        rcs.append(lib.stif_rgb_to_yuv(fp, rgb, *strides, n, y, u, v, None))
        return rcs, msg + b" | " + lib.stif_last_error()

    bad = [
        (dict(f=None), b"format is null"),
        (dict(f=fmt(), y=None), b"plane pointer is null"), (dict(f=fmt(), u=None), b"plane pointer is null"),
        (dict(f=fmt(), v=None), b"plane pointer is null"), (dict(f=fmt(), rgb=None), b"is null"),
        (dict(f=fmt(), n=0), b">= 1"), (dict(f=fmt(width=0)), b">= 1"), (dict(f=fmt(height=-3)), b">= 1"),
        (dict(f=fmt(sub_x=2)), b"sub_x"), (dict(f=fmt(sub_y=-1)), b"sub_y"),
        (dict(f=fmt(depth=7)), b"depth"), (dict(f=fmt(depth=17)), b"depth"),
        (dict(f=fmt(matrix=2)), b"matrix"), (dict(f=fmt(full_range=2)), b"full_range"),
        (dict(f=fmt(pitch_y=7)), b"pitch below"), (dict(f=fmt(pitch_c=3)), b"pitch below"),
        (dict(f=fmt(depth=10, pitch_y=15)), b"pitch below"), (dict(f=fmt(depth=10, pitch_y=17)), b"2-byte aligned"),
        (dict(f=fmt(depth=10), u=u + 1), b"2-byte aligned"),
        (dict(f=fmt(pitch_y=-8)), b"negative"), (dict(f=fmt(frame_stride=16), n=2), b"frame stride"),
        (dict(f=fmt(), strides=(96, 32, 7)), b"strides"), (dict(f=fmt(), strides=(96, 31, 8)), b"strides"),
        (dict(f=fmt(), n=2, strides=(95, 32, 8)), b"strides"),
    ]
    for kw, word in bad:
        rcs, msg = both(**kw)
        assert rcs == [L.E_INVALID, L.E_INVALID], (kw, rcs, msg)
        assert msg.count(word) == 2, (kw, msg)
    torch.cuda.synchronize()
    assert all(int(b.sum()) == 0 for b in bufs)                            # nothing ran
    rcs, _ = both(fmt(), n=2, strides=(96, 32, 8))                         # the same calls with good arguments
    assert rcs == [0, 0]
    with pytest.raises(ValueError):
        stif.ops.yuv_to_rgb(bufs[0][:47], stif.y4m.YuvFormat(8, 4))
