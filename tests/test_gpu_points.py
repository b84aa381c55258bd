"""Point queries on the GPU: LunaTokis.decoding_points decodes any set of pixels of the virtual grid, each at its own
time, bit-identical to the full scalar-time decode at those pixels (both operand modes), pinned to the oracle's
decoding_at, with its argument forms, its flow output, its index safety and the C ABI's argument checks.
Latent: tests/test_gpu_window.py's -- gen_feat of a seeded 16x20 pair, B = 2, a different time per item."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import stif_oracle as O

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-4, 1e-6                      # the project's oracle tolerance (tests/test_gpu_fullsize.py)
F32 = np.float32
MODES = ["f16x3", "f32"]
TIMES = [[0.3, 0.7], [0.55, 0.1]]            # two queries, each with a different time per item
GRIDS = [(37, 45), (64, 80)]                 # non-integer scale with nearest-index ties, and 4x
# flow_imnet's last layer as make_state_dict(seed=0) gives it, and times 64: every flow then exceeds 3 HR pixels, so
# a point's corners lie rows away from it
FLOW_SCALES = [1.0, 64.0]
# below and across the 16- and 32-pixel wave groups, past one and past three workgroups
COUNTS = [1, 15, 17, 129, 437]
POINT_TIMES = [0.1, 0.55, 0.9]


def points(HH, WW, n):
    """[2, n] rows and columns: the four grid corners, the centre and three mid-edge pixels, then seeded random
    pixels; item 1 takes them in reverse order."""
    y = [0, 0, HH - 1, HH - 1, HH // 2, 0, HH // 2, HH - 1]
    x = [0, WW - 1, 0, WW - 1, WW // 2, WW // 2, 0, WW // 2]
    rng = np.random.default_rng(11)
    m = max(0, n - 8)
    y = np.concatenate([y, rng.integers(0, HH, m)])[:n].astype(np.int64)
    x = np.concatenate([x, rng.integers(0, WW, m)])[:n].astype(np.int64)
    return np.stack([y, y[::-1]]), np.stack([x, x[::-1]])


class Lat:
    """One model per (operand mode, flow scale) with the shared latent and its full-frame decodes (computed once)."""

    def __init__(self, stif, sd, mode, flow_scale):
        sd = dict(sd)
        for k in ("flow_imnet.net.3.weight", "flow_imnet.net.3.bias"):
            sd[k] = (np.asarray(sd[k]) * F32(flow_scale)).astype(F32)
        self.sd = sd
        self.m = stif.LunaTokis(64, 6, 8, 5, 40, mfma=mode)
        self.m.load_state_dict(sd, strict=True)
        self.x = torch.rand(2, 2, 3, 16, 20, generator=torch.Generator().manual_seed(77)).cuda()
        with torch.no_grad():
            self.m.gen_feat(self.x)
        self._full = {}

    def full(self, grid, t):
        """The full decode [2, 3, HH, WW] at ``t``: a float, or a pair of per-item times."""
        key = (grid, tuple(t) if isinstance(t, list) else t)
        if key not in self._full:
            tq = torch.tensor(t, dtype=torch.float32).reshape(-1, 1)
            with torch.no_grad():
                self._full[key] = self.m.decoding([tq], grid)[0].clone()
        return self._full[key]

    def at(self, grid, t, y, x):
        """[2, 3, n]: the full decode at t indexed at the [2, n] pixels."""
        f = self.full(grid, t)
        iy, ix = torch.as_tensor(y).cuda(), torch.as_tensor(x).cuda()
        return torch.stack([f[b][:, iy[b], ix[b]] for b in range(2)])


@pytest.fixture(scope="module")
def lats(stif, sd):
    cache = {}

    def get(mode, flow_scale=64.0):
        if (mode, flow_scale) not in cache:
            cache[mode, flow_scale] = Lat(stif, sd, mode, flow_scale)
        return cache[mode, flow_scale]
    return get


def pts(m, *a, **kw):
    with torch.no_grad():
        return m.decoding_points(*a, **kw)


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: f"{g[0]}x{g[1]}")
@pytest.mark.parametrize("flow_scale", FLOW_SCALES)
@pytest.mark.parametrize("mode", MODES)
def test_points_equal_the_full_decode(lats, mode, flow_scale, grid, n):
    la = lats(mode, flow_scale)
    y, x = points(*grid, n)
    for t in TIMES:
        out = pts(la.m, y, x, torch.tensor(t), grid)
        assert out.shape == (2, 3, n) and out.dtype == torch.float32 and out.is_cuda
        assert torch.equal(out, la.at(grid, t, y, x)), (mode, flow_scale, grid, n, t)
    assert la.m.range_reruns == 0


@pytest.mark.parametrize("flow_scale", FLOW_SCALES)
@pytest.mark.parametrize("mode", MODES)
def test_every_point_at_its_own_time(lats, mode, flow_scale):
    """The times dealt round-robin over the points: each point is the full decode at its scalar time."""
    la, grid, n = lats(mode, flow_scale), GRIDS[0], 437
    y, x = points(*grid, n)
    tp = np.array([POINT_TIMES[p % 3] for p in range(n)], F32)
    out = pts(la.m, y, x, tp, grid)                                     # [n]: shared by the items
    out2 = pts(la.m, torch.from_numpy(y).cuda().int(), torch.from_numpy(x).cuda().int(),
               torch.from_numpy(np.stack([tp, tp])).cuda(), grid)       # [B, n] on the device, read in place
    assert torch.equal(out, out2)
    for v in POINT_TIMES:
        sel = torch.from_numpy(np.flatnonzero(tp == F32(v))).cuda()
        assert torch.equal(out[:, :, sel], la.at(grid, v, y, x)[:, :, sel]), (mode, flow_scale, v)
    assert la.m.range_reruns == 0


@pytest.mark.parametrize("mode", MODES)
def test_argument_forms(lats, mode):
    la, grid = lats(mode), GRIDS[0]
    HH, WW = grid
    m = la.m
    y, x = points(HH, WW, 437)
    t = TIMES[0]
    # [n] points are the same points for every item
    shared = pts(m, y[0], x[0], torch.tensor(t), grid)
    assert torch.equal(shared, pts(m, np.stack([y[0], y[0]]), np.stack([x[0], x[0]]), torch.tensor(t), grid))
    assert torch.equal(shared, la.at(grid, t, np.stack([y[0], y[0]]), np.stack([x[0], x[0]])))
    # one pixel 40 times: with equal times equal values, with different times the values of those times
    ry, rx = np.full(40, 20), np.full(40, 31)
    same = pts(m, ry, rx, 0.55, grid)
    ref = {v: la.at(grid, v, np.stack([ry[:1]] * 2), np.stack([rx[:1]] * 2)) for v in POINT_TIMES}
    assert torch.equal(same, ref[0.55].expand(2, 3, 40))
    tp = np.array([POINT_TIMES[p % 3] for p in range(40)], F32)
    mixed = pts(m, ry, rx, tp, grid)
    for p in range(40):
        assert torch.equal(mixed[:, :, p], ref[POINT_TIMES[p % 3]][:, :, 0]), p
    # pairs=[1]: item 1's slice
    both = pts(m, y, x, torch.tensor(t), grid)
    one = pts(m, y[1], x[1], t[1], grid, pairs=[1])
    assert one.shape == (1, 3, 437) and torch.equal(one[0], both[1])
    # several passes over items and points change no bit
    keep = m.dec_chunk_px
    m.dec_chunk_px = 8 * 64
    try:
        chunked, cflow = pts(m, y, x, torch.tensor(t), grid, return_flow=True)
    finally:
        m.dec_chunk_px = keep
    whole, wflow = pts(m, y, x, torch.tensor(t), grid, return_flow=True)
    assert torch.equal(chunked, both) and torch.equal(whole, both) and torch.equal(cflow, wflow)
    assert m.range_reruns == 0


@pytest.mark.parametrize("mode", MODES)
def test_points_match_the_oracle(lats, mode):
    """437 points of the 37 x 45 grid with flows of several pixels against O.decoding_at on the engine's own latent,
    per item and per time; some of the oracle's warped samples are clamped at the frame edge."""
    la, (HH, WW) = lats(mode, 64.0), GRIDS[0]
    y, x = points(HH, WW, 437)
    feat, inp = la.m.feat.cpu().numpy(), la.m.inp.cpu().numpy()
    for t in TIMES:
        got = pts(la.m, y, x, torch.tensor(t), (HH, WW)).double().cpu().numpy()
        for b in range(2):
            st = {}
            ref = O.decoding_at(feat[b:b + 1], inp[b:b + 1], [t[b]], la.sd, HH, WW, y[b], x[b], stats=st)[0][0]
            assert st["clamped"] > 0
            d, lim = np.abs(got[b] - ref), RTOL * np.abs(ref) + ATOL
            print(f"points vs oracle {mode} t={t[b]} item {b}: clamped {st['clamped']}, max err / limit "
                  f"{float((d / lim).max()):.3f}, max err {float(d.max()):.3e}")
            assert (d <= lim).all(), (mode, t[b], b, float((d / lim).max()), float(d.max()))


@pytest.mark.parametrize("flow_scale", FLOW_SCALES)
@pytest.mark.parametrize("mode", MODES)
def test_return_flow_is_stage_one_flow(stif, lats, mode, flow_scale):
    la, (HH, WW) = lats(mode, flow_scale), GRIDS[0]
    m, ops = la.m, stif.ops
    y, x = points(HH, WW, 437)
    t = torch.tensor(TIMES[1])
    out, flow = pts(m, y, x, t, (HH, WW), return_flow=True)
    assert flow.shape == (2, 4, 437)
    proj = m._projection()
    hrf, fl = torch.empty(2, HH, WW, 64, device="cuda"), torch.empty(2, HH, WW, 4, device="cuda")
    ops.dec_stage1(proj, m.layers["dec.mlp"], m._tab(16, 20, HH, WW), t.cuda(), hrf, fl, flags=m._dec_flags)
    iy, ix = torch.from_numpy(y).cuda(), torch.from_numpy(x).cuda()
    ref = torch.stack([fl[b][iy[b], ix[b]].T for b in range(2)])
    assert torch.equal(flow, ref)
    if flow_scale == 64.0:
        assert float(flow.abs().amax(1).min()) > 3.0     # every point's flow exceeds 3 HR pixels
    assert torch.equal(out, la.at((HH, WW), TIMES[1], y, x))


@pytest.mark.parametrize("mode", MODES)
def test_indices_outside_the_grid(lats, mode):
    la, (HH, WW) = lats(mode), GRIDS[0]
    m = la.m
    y, x = points(HH, WW, 17)
    good = pts(m, y, x, 0.3, (HH, WW))
    bad = y.copy()
    bad[1, 5] = HH
    with pytest.raises(IndexError):                      # host data: before any launch
        pts(m, bad, x, 0.3, (HH, WW))
    dy, dx = torch.from_numpy(bad).cuda().int(), torch.from_numpy(x).cuda().int()
    with pytest.raises(IndexError):                      # device data: the kernels' flag, read once afterwards
        pts(m, dy, dx, 0.3, (HH, WW))
    dx2 = dx.clone()
    dx2[0, 3] = -7
    with pytest.raises(IndexError):
        pts(m, torch.from_numpy(y).cuda().int(), dx2, 0.3, (HH, WW))
    keep = m.range_check
    m.range_check = "off"
    try:
        out = pts(m, dy, dx, 0.3, (HH, WW))              # not read back: clamped, finite
    finally:
        m.range_check = keep
    assert torch.isfinite(out).all()
    sel = [p for p in range(17) if p != 5]
    assert torch.equal(out[0], good[0]) and torch.equal(out[1][:, sel], good[1][:, sel])
    clamped = bad.copy()
    clamped[1, 5] = HH - 1
    assert torch.equal(out, la.at((HH, WW), 0.3, clamped, x))
    assert torch.equal(pts(m, y, x, 0.3, (HH, WW)), good)     # the flag does not outlive the call


def test_point_entry_points_validate_before_launching(stif):
    """A null pointer, npts < 1, n * 8 * npts past INT_MAX, a negative stride and tables with hr_y / hr_x are
    STIF_E_INVALID with a message naming the cause, for all three entry points."""
    L = stif._lib
    lib = L.lib()
    A = 4096                                             # a fake address: validation comes first
    p = C.c_void_p(A)
    tab, tab_hr = L.DecTables(*[A] * 14), L.DecTables(*[A] * 16)
    HH, WW = 37, 45
    good = L.DecPointList(A, A, A, 17, 17, 17, 1, 17)

    def s1(q=good, tab=tab, proj=p, n=2):
        return lib.stif_dec_stage1_pts(proj, p, C.byref(tab), C.byref(q) if q is not None else None, p, p, n, 16, 20,
                                       HH, WW, 0, None, None)

    def co(q=good, tab=tab, proj=p, n=2):
        return lib.stif_dec_corners_pts(proj, C.byref(tab), C.byref(q) if q is not None else None, p, p, p, n, HH, WW,
                                        None, None)

    def s2(q=good, tab=tab, proj=p, n=2):
        return lib.stif_dec_stage2_pts(proj, p, p, p, C.byref(tab), C.byref(q) if q is not None else None, p, n, 16,
                                       20, HH, WW, 0, None, None)

    def rejected(rc, text, me):
        err = lib.stif_last_error().decode()
        assert rc == L.E_INVALID, (text, err)
        assert err.startswith(me + ": ") and text in err, (text, err)

    for fn, me in ((s1, "stif_dec_stage1_pts"), (co, "stif_dec_corners_pts"), (s2, "stif_dec_stage2_pts")):
        rejected(fn(proj=None), "null pointer", me)
        rejected(fn(q=None), "null point list", me)
        for k in range(3):
            ptrs = [A, A, A]
            ptrs[k] = None
            rejected(fn(q=L.DecPointList(*ptrs, 17, 17, 17, 1, 17)), "null point list", me)
        for npts in (0, -3):
            rejected(fn(q=L.DecPointList(A, A, A, 17, 17, 17, 1, npts)), "npts < 1", me)
        rejected(fn(q=L.DecPointList(A, A, A, 0, 0, 0, 0, 2 ** 27), n=2), "exceeds INT_MAX", me)
        rejected(fn(q=L.DecPointList(A, A, A, 0, 0, 0, 0, 2 ** 30), n=1), "exceeds INT_MAX", me)
        for k in range(4):
            strides = [17, 17, 17, 1]
            strides[k] = -1
            rejected(fn(q=L.DecPointList(A, A, A, *strides, 17)), "negative point stride", me)
        rejected(fn(tab=tab_hr), "hr_y / hr_x", me)
