"""Windowed decoding on the GPU: any rectangle of the virtual output grid, rendered at the cost of that rectangle,
is bit-identical to the crop of the full-frame decode (both operand modes, decoding and decoding_test), is pinned
to the oracle at its own pixels, and its pieces (the bounding-box kernel, stage 2 over a rectangle, tiling, the
zoom call) are checked one by one.  Latent: gen_feat of a seeded 16x20 pair, B = 2, a different time per item."""
import numpy as np
import pytest
import torch

from oracle import stif_oracle as O

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-4, 1e-6                      # the project's oracle tolerance (tests/test_gpu_fullsize.py)
F32 = np.float32
TIMES = [[0.3, 0.7], [0.55, 0.1]]            # two queries, each with a different time per item
GRIDS = [(37, 45), (64, 80)]                 # non-integer scale with nearest-index ties, and 4x
# flow_imnet's last layer is used as make_state_dict(seed=0) gives it (factor 1): warpgrid's linspace base sits up
# to half a pixel off the pixel centre, so the gathers leave an interior window by a pixel even for small flows
FLOW_SCALE = 1.0
# the same layer times 64: flows up to about 4 HR pixels (make_state_dict's last flow layer is U(+-0.005) over 256
# sines plus a +-0.05 bias), so the F rectangle is set by the flows and not by the half-pixel base offset
LARGE_FLOW_SCALE = 64.0


def windows(HH, WW):
    return {
        "interior": (9, 11, 13, 17),
        "top_left": (0, 0, 13, 17),
        "top_right": (0, WW - 17, 13, 17),
        "bottom_left": (HH - 13, 0, 13, 17),
        "bottom_right": (HH - 13, WW - 17, 13, 17),
        "row_strip": (HH // 2, 0, 1, WW),
        "col_strip": (0, WW // 3, HH, 1),
        "sub_wave": (5, 7, 3, 5),                       # 15 pixels: less than one 16-pixel wave group
        "three_workgroups": (3, 2, 19, 23),             # 437 pixels: > 2 x 128, not a multiple of 16
        "whole": (0, 0, HH, WW),
    }


WNAMES = sorted(windows(37, 45))


class Lat:
    """One model per operand mode with the shared latent, and its full-frame decodes (computed once)."""

    def __init__(self, stif, sd, mode, flow_scale=FLOW_SCALE):
        sd = dict(sd)
        for k in ("flow_imnet.net.3.weight", "flow_imnet.net.3.bias"):
            sd[k] = (np.asarray(sd[k]) * F32(flow_scale)).astype(F32)
        self.sd = sd
        self.m = stif.LunaTokis(64, 6, 8, 5, 40, mfma=mode)
        self.m.load_state_dict(sd, strict=True)
        self.x = torch.rand(2, 2, 3, 16, 20, generator=torch.Generator().manual_seed(77)).cuda()
        self.tq = [torch.tensor(t, dtype=torch.float32).reshape(2, 1) for t in TIMES]
        with torch.no_grad():
            self.m.gen_feat(self.x)
        self.full = {}

    def decode(self, kind, grid, **kw):
        with torch.no_grad():
            if kind == "decoding":
                return self.m.decoding(self.tq, grid, **kw)
            return self.m.decoding_test(self.tq, 4, **kw)

    def full_frame(self, kind, grid):
        if (kind, grid) not in self.full:
            self.full[kind, grid] = [o.clone() for o in self.decode(kind, grid)]
        return self.full[kind, grid]


@pytest.fixture(scope="module")
def lats(stif, sd):
    cache = {}

    def get(mode, flow_scale=FLOW_SCALE):
        if (mode, flow_scale) not in cache:
            cache[mode, flow_scale] = Lat(stif, sd, mode, flow_scale)
        return cache[mode, flow_scale]
    return get


CASES = [("decoding", g) for g in GRIDS] + [("decoding_test", (64, 80))]


@pytest.mark.parametrize("wname", WNAMES)
@pytest.mark.parametrize("kind,grid", CASES, ids=[f"{k}-{g[0]}x{g[1]}" for k, g in CASES])
@pytest.mark.parametrize("mode", ["f16x3", "f32"])
def test_window_is_the_crop_of_the_full_decode(lats, mode, kind, grid, wname):
    crop_of_the_full_decode(lats(mode), mode, kind, grid, wname)


def crop_of_the_full_decode(la, mode, kind, grid, wname):
    y0, x0, hh, ww = windows(*grid)[wname]
    full = la.full_frame(kind, grid)
    got = la.decode(kind, grid, window=(y0, x0, hh, ww))
    assert len(got) == len(full)
    fy0, fx0, fh, fw = la.m.last_window_F
    assert fy0 <= y0 and fx0 <= x0 and fy0 + fh >= y0 + hh and fx0 + fw >= x0 + ww      # F holds W
    assert 0 <= fy0 and 0 <= fx0 and fy0 + fh <= grid[0] and fx0 + fw <= grid[1]
    for g, f in zip(got, full):
        assert tuple(g.shape) == (2, 3, hh, ww)
        assert torch.equal(g, f[:, :, y0:y0 + hh, x0:x0 + ww]), (mode, kind, grid, wname, la.m.last_window_F)
    assert la.m.range_reruns == 0


@pytest.mark.parametrize("wname", ["interior", "top_left", "bottom_right", "sub_wave", "three_workgroups"])
@pytest.mark.parametrize("grid", GRIDS, ids=[f"{g[0]}x{g[1]}" for g in GRIDS])
@pytest.mark.parametrize("mode", ["f16x3", "f32"])
def test_window_is_the_crop_of_the_full_decode_with_large_flows(lats, mode, grid, wname):
    """The same bit-for-bit equality on a latent whose flows really leave the window (flow_imnet's last layer times
    LARGE_FLOW_SCALE): the interior window's F rectangle exceeds it by 3 pixels or more on some side, so the
    data-dependent feat-only pass over F and stage 2's gathers rows away from their pixel are what is compared.
    (Large flows against the oracle: tests/test_gpu_decoder_stages.py.)"""
    la = lats(mode, LARGE_FLOW_SCALE)
    crop_of_the_full_decode(la, mode, "decoding", grid, wname)
    if wname == "interior":
        y0, x0, hh, ww = windows(*grid)[wname]
        fy0, fx0, fh, fw = la.m.last_window_F
        grown = (y0 - fy0, x0 - fx0, fy0 + fh - (y0 + hh), fx0 + fw - (x0 + ww))
        print("large flows", mode, grid, "interior window", (y0, x0, hh, ww), "last_window_F", la.m.last_window_F,
              "grown by (top, left, bottom, right)", grown)
        assert max(grown) >= 3, (la.m.last_window_F, grown)


@pytest.mark.parametrize("mode", ["f16x3", "f32"])
def test_window_F_rectangles_grow_and_reach_the_border(lats, mode):
    """The data-dependent part is exercised: the gathers of an interior window leave it (F strictly larger than W,
    so the feat-only pass over F runs), and some F reaches the grid border (clamped corners)."""
    la = lats(mode)
    grew, border = [], []
    for grid in GRIDS:
        HH, WW = grid
        for name, w in windows(*grid).items():
            la.decode("decoding", grid, window=w)
            fy0, fx0, fh, fw = F = la.m.last_window_F
            if name == "interior":
                assert fh * fw > w[2] * w[3], (grid, w, F)
            if fh * fw > w[2] * w[3]:
                grew.append((grid, name, F))
            if fy0 == 0 or fx0 == 0 or fy0 + fh == HH or fx0 + fw == WW:
                border.append((grid, name, F))
    print("F larger than W:", grew)
    print("F at the border:", border)
    assert grew and border


def test_window_matches_the_oracle_at_its_pixels(lats):
    """Pinned to the reference arithmetic, not only to our own full decode: the oracle's pixel-subset decoder at
    the window's pixels, in full-grid coordinates."""
    la = lats("f16x3")
    HH, WW = 37, 45
    y0, x0, hh, ww = 9, 11, 13, 17
    got = la.decode("decoding", (HH, WW), window=(y0, x0, hh, ww))
    py, px = np.meshgrid(np.arange(y0, y0 + hh), np.arange(x0, x0 + ww), indexing="ij")
    feat = la.m.feat.cpu().numpy()
    x = la.x.cpu().numpy()
    for ti, ts in enumerate(TIMES):
        for b, t in enumerate(ts):
            ref = O.decoding_at(feat[b:b + 1], x[b:b + 1], [F32(t)], la.sd, HH, WW, py.ravel(), px.ravel())[0][0]
            g = got[ti][b].reshape(3, -1).double().cpu().numpy()
            d = np.abs(g - ref)
            lim = RTOL * np.abs(ref) + ATOL
            assert (d <= lim).all(), (ti, b, float((d / lim).max()), float(d.max()))


def synthetic_flow(kind, n, hh, ww, seed=5):
    rng = np.random.default_rng(seed)
    if kind == "uniform":
        return rng.uniform(-3.5, 3.5, (n, hh, ww, 4)).astype(F32)
    f = rng.uniform(-3.5, 3.5, (n, hh, ww, 4)).astype(F32)      # "huge": some grids clamp to the frame edge
    f[rng.random(f.shape) < 0.1] = F32(1e4)
    f[rng.random(f.shape) < 0.1] = F32(-1e4)
    return f


def box_numpy(flow, lin_y, lin_x, rect, HH, WW):
    """The box in numpy with stage 2's fp32 formula: lin + flow / d, clamp to +-(1 - 1e-6), unnormalise, floor,
    clamp the two corners into the grid."""
    y0, x0, hh, ww = rect
    lo, hi = F32(-1.0) + F32(1e-6), F32(1.0) - F32(1e-6)
    dx, dy = (F32(WW) - F32(1)) / F32(2), (F32(HH) - F32(1)) / F32(2)
    bx = lin_x[x0:x0 + ww][None, None, :]
    by = lin_y[y0:y0 + hh][None, :, None]
    xs, ys = [], []
    for k in (0, 2):
        gx = np.clip((bx + flow[..., k] / dx).astype(F32), lo, hi)
        gy = np.clip((by + flow[..., k + 1] / dy).astype(F32), lo, hi)
        fx = np.floor(((gx + F32(1)) * F32(WW) - F32(1)) / F32(2)).astype(np.int64)
        fy = np.floor(((gy + F32(1)) * F32(HH) - F32(1)) / F32(2)).astype(np.int64)
        xs += [np.clip(fx, 0, WW - 1), np.clip(fx + 1, 0, WW - 1)]
        ys += [np.clip(fy, 0, HH - 1), np.clip(fy + 1, 0, HH - 1)]
    return [int(np.min(ys)), int(np.max(ys)), int(np.min(xs)), int(np.max(xs))]


@pytest.mark.parametrize("kind", ["uniform", "huge"])
def test_bounds_kernel_matches_numpy(stif, kind):
    HH, WW = 37, 45
    rect = (9, 11, 13, 17)
    ops = stif.ops
    tab = ops.DecTablesDev(16, 20, HH, WW, "cuda")
    flow = synthetic_flow(kind, 2, rect[2], rect[3])
    box = torch.full((4,), 12345, dtype=torch.int32, device="cuda")
    ops.dec_bounds(torch.from_numpy(flow).cuda(), tab, box, ops.dec_window(rect, HH, WW))
    ref = box_numpy(flow, stif.coords.linspace_f32(HH), stif.coords.linspace_f32(WW), rect, HH, WW)
    assert box.tolist() == ref, (box.tolist(), ref)
    if kind == "huge":
        assert ref == [0, HH - 1, 0, WW - 1]


@pytest.mark.parametrize("mode", ["f16x3", "f32"])
def test_stage2_window_from_a_synthetic_flow(stif, lats, mode):
    """stif_dec_stage2_win over a window, HRfeat cropped to the box of stif_dec_bounds, against stif_dec_stage2_ex
    over the whole grid: same bits, status stays 0."""
    la = lats(mode)
    m, ops = la.m, stif.ops
    HH, WW, n = 37, 45, 2
    y0, x0, hh, ww = rect = (9, 11, 13, 17)
    gen = torch.Generator().manual_seed(11)
    proj = (torch.rand(n, 16, 20, 256, generator=gen) - 0.5).cuda()
    hrf = (torch.rand(n, HH, WW, 64, generator=gen) - 0.5).cuda()
    t = torch.tensor([0.3, 0.7], device="cuda")
    wflow = torch.from_numpy(synthetic_flow("uniform", n, hh, ww)).cuda()
    flow = torch.zeros(n, HH, WW, 4, device="cuda")
    flow[:, y0:y0 + hh, x0:x0 + ww] = wflow
    mlp, tab, fl = m.layers["dec.mlp"], m._tab(16, 20, HH, WW), m._dec_flags
    full = torch.empty(n, 3, HH, WW, device="cuda")
    ops.dec_stage2(proj, mlp, hrf, flow, tab, t, full, flags=fl)
    box = torch.empty(4, dtype=torch.int32, device="cuda")
    ops.dec_bounds(wflow, tab, box, ops.dec_window(rect, HH, WW))
    ymin, ymax, xmin, xmax = box.tolist()
    fy0, fx0 = min(ymin, y0), min(xmin, x0)
    frect = (fy0, fx0, max(ymax + 1, y0 + hh) - fy0, max(xmax + 1, x0 + ww) - fx0)
    assert frect[2] * frect[3] > hh * ww and frect[2] * frect[3] < HH * WW
    hf = hrf[:, fy0:fy0 + frect[2], fx0:fx0 + frect[3]].contiguous()
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    out = torch.full((n, 3, hh, ww), float("nan"), device="cuda")
    ops.dec_stage2(proj, mlp, hf, wflow, tab, t, out, flags=fl, status=st, window=ops.dec_window(rect, HH, WW, frect))
    assert int(st.item()) == 0
    assert torch.equal(out, full[:, :, y0:y0 + hh, x0:x0 + ww])


def test_tiled_decode_equals_untiled_with_bounded_scratch(lats):
    la = lats("f16x3")
    HH, WW = 37, 45
    full = la.full_frame("decoding", (HH, WW))
    keep = la.m.dec_chunk_px
    la.m.dec_chunk_px = 1000                 # below 37 * 45: the full-frame decode could not honour it at all
    try:
        got = la.decode("decoding", (HH, WW), tile=(16, 16))     # 3 x 3 tiles, ragged last row / column
        peak = la.m.window_peak_scratch_bytes
    finally:
        la.m.dec_chunk_px = keep
    for g, f in zip(got, full):
        assert tuple(g.shape) == (2, 3, HH, WW) and torch.equal(g, f)
    print("peak windowed scratch", peak, "B; one full-frame HRfeat", HH * WW * 256, "B")
    assert 0 < peak < HH * WW * 64 * 4


def test_decoding_window_is_decoding_of_the_centred_rectangle(stif, lats):
    la = lats("f16x3")
    grid, center, size = (64, 80), (-0.9, 0.95), (24, 28)
    win = stif.coords.window_from_center(center, grid[0], grid[1], size)
    assert win == (0, 52, 24, 28)            # rows: int(0.05 * 64) = 3 -> 3 - 12 < 0 -> 0; cols: 78 + 14 > 80 -> 52
    with torch.no_grad():
        got = la.m.decoding_window(la.tq, grid, center, size)
    ref = la.decode("decoding", grid, window=win)
    full = la.full_frame("decoding", grid)
    for g, r, f in zip(got, ref, full):
        assert torch.equal(g, r) and torch.equal(g, f[:, :, 0:24, 52:80])
    with torch.no_grad():                    # default size: 4H x 4W of a larger virtual grid
        d = la.m.decoding_window(la.tq, (128, 160), (0.0, 0.0))
    assert tuple(d[0].shape) == (2, 3, 64, 80)
