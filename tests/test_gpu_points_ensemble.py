"""Point queries of the local ensemble on the GPU: ``decoding_points(ensemble=True)`` is bit-identical to the full
``decoding(ensemble=True)`` at the points (both operand modes), with every argument form of the plain point path, its
remap and flow stages pinned on their own, the result pinned to the oracle's decoding_localensemble, and the plain
path's index safety.  Setup as tests/test_gpu_points.py: the seeded 16x20 pair, B = 2, a different time per item; the
full ensemble decode is computed once per (mode, flow scale, grid, time)."""
import numpy as np
import pytest
import torch

from oracle import stif_oracle as O
from test_gpu_points import ATOL, COUNTS, FLOW_SCALES, GRIDS, MODES, POINT_TIMES, RTOL, TIMES, Lat, points

pytestmark = pytest.mark.gpu
F32 = np.float32


class ELat(Lat):
    """test_gpu_points' latent with the full ensemble decodes in place of the plain ones."""

    def full(self, grid, t):
        key = (grid, tuple(t) if isinstance(t, list) else t)
        if key not in self._full:
            tq = torch.tensor(t, dtype=torch.float32).reshape(-1, 1)
            with torch.no_grad():
                self._full[key] = self.m.decoding([tq], grid, ensemble=True)[0].clone()
        return self._full[key]


@pytest.fixture(scope="module")
def lats(stif, sd):
    cache = {}

    def get(mode, flow_scale=64.0):
        if (mode, flow_scale) not in cache:
            cache[mode, flow_scale] = ELat(stif, sd, mode, flow_scale)
        return cache[mode, flow_scale]
    return get


def pts(m, *a, **kw):
    with torch.no_grad():
        return m.decoding_points(*a, ensemble=True, **kw)


# ---- 1: against the full ensemble decode
@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: f"{g[0]}x{g[1]}")
@pytest.mark.parametrize("flow_scale", FLOW_SCALES)
@pytest.mark.parametrize("mode", MODES)
def test_points_equal_the_full_ensemble_decode(lats, mode, flow_scale, grid, n):
    la = lats(mode, flow_scale)
    y, x = points(*grid, n)
    for t in TIMES:
        out = pts(la.m, y, x, torch.tensor(t), grid)
        assert out.shape == (2, 3, n) and out.dtype == torch.float32 and out.is_cuda
        assert torch.equal(out, la.at(grid, t, y, x)), (mode, flow_scale, grid, n, t)
    assert la.m.range_reruns == 0


# ---- 2: per-point times
@pytest.mark.parametrize("flow_scale", FLOW_SCALES)
@pytest.mark.parametrize("mode", MODES)
def test_every_point_at_its_own_time(lats, mode, flow_scale):
    """The times dealt round-robin over the points: each point is the full ensemble decode at its scalar time."""
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


# ---- 3: argument forms
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
    assert torch.equal(both, la.at(grid, t, y, x))
    one = pts(m, y[1], x[1], t[1], grid, pairs=[1])
    assert one.shape == (1, 3, 437) and torch.equal(one[0], both[1])
    # several passes over items and points change no bit
    keep = m.dec_chunk_px
    m.dec_chunk_px = 8 * 64
    try:
        chunked = pts(m, y, x, torch.tensor(t), grid)
    finally:
        m.dec_chunk_px = keep
    assert torch.equal(chunked, both)
    # ensemble=False is the call without the keyword
    with torch.no_grad():
        plain = m.decoding_points(y, x, torch.tensor(t), grid)
        assert torch.equal(m.decoding_points(y, x, torch.tensor(t), grid, ensemble=False), plain)
    assert not torch.equal(plain, both)
    assert m.range_reruns == 0


# ---- 4: the new stages on their own
def test_remap_equals_the_host_tables(stif, lats):
    la, (HH, WW) = lats("f32"), GRIDS[0]
    m, ops = la.m, stif.ops
    y, x = points(HH, WW, 437)
    dy, dx = torch.from_numpy(y).cuda().int(), torch.from_numpy(x).cuda().int()
    t = torch.tensor(TIMES[0]).cuda().reshape(2, 1)
    pl = ops.DecPoints(dy, dx, t, 437, 437, 1, 0, 437, 2)
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    identity = True
    for s in ops.ENSEMBLE_SHIFTS:
        tab = m._tab(16, 20, HH, WW, s)
        ry, rx = (torch.empty(2, 437, dtype=torch.int32, device="cuda") for _ in range(2))
        rem = ops.dec_remap_pts(tab, pl, 2, ry, rx, status=status)
        assert np.array_equal(ry.cpu().numpy(), tab.hr_y[y]) and np.array_equal(rx.cpu().numpy(), tab.hr_x[x])
        assert rem.npts == 437 and rem.strides == (437, 437, 1, 0)
        identity &= np.array_equal(tab.hr_y[y], y) and np.array_equal(tab.hr_x[x], x)
    assert not identity                                   # the shifted remaps differ from the identity
    assert int(status.item()) == 0
    # a row outside the grid on the device: clamped and flagged, the other entries unchanged
    dy2 = dy.clone()
    dy2[1, 5] = HH + 3
    tab = m._tab(16, 20, HH, WW, ops.ENSEMBLE_SHIFTS[0])
    ry2, rx2 = (torch.empty(2, 437, dtype=torch.int32, device="cuda") for _ in range(2))
    ops.dec_remap_pts(tab, ops.DecPoints(dy2, dx, t, 437, 437, 1, 0, 437, 2), 2, ry2, rx2, status=status)
    assert int(status.item()) == 8
    yc = y.copy()
    yc[1, 5] = HH - 1
    assert np.array_equal(ry2.cpu().numpy(), tab.hr_y[yc]) and np.array_equal(rx2.cpu().numpy(), tab.hr_x[x])


@pytest.mark.parametrize("flow_scale", FLOW_SCALES)
@pytest.mark.parametrize("mode", MODES)
def test_flow_stage_equals_the_whole_grid_flow(stif, lats, mode, flow_scale):
    """stif_dec_flow_pts over the compact operand against the flow of stif_dec_stage1_ex with the same shifted tables
    over the whole grid, at the points: the same bits for each shift."""
    la, (HH, WW) = lats(mode, flow_scale), GRIDS[0]
    m, ops = la.m, stif.ops
    n = 437
    y, x = points(HH, WW, n)
    dy, dx = torch.from_numpy(y).cuda().int(), torch.from_numpy(x).cuda().int()
    iy, ix = torch.from_numpy(y).cuda(), torch.from_numpy(x).cuda()
    t = torch.tensor(TIMES[1]).cuda()
    pl = ops.DecPoints(dy, dx, t, n, n, 1, 0, n, 2)
    mlp, fl = m.layers["dec.mlp"], m._dec_flags
    proj = m._projection()
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    for s in ops.ENSEMBLE_SHIFTS:
        tab = m._tab(16, 20, HH, WW, s)
        hrf, flow = torch.empty(2, HH, WW, 64, device="cuda"), torch.empty(2, HH, WW, 4, device="cuda")
        ops.dec_stage1(proj, mlp, tab, t, hrf, flow, flags=fl)
        ref = torch.stack([flow[b][iy[b], ix[b]] for b in range(2)])
        ints = lambda: torch.empty(2, n, dtype=torch.int32, device="cuda")
        rem = ops.dec_remap_pts(tab, pl, 2, ints(), ints(), status=status)
        op = torch.empty(2, n, 64, device="cuda")
        ops.dec_stage1_pts(proj, mlp, tab.plain, rem, op, None, flags=fl, status=status)
        got = torch.empty(2, n, 4, device="cuda")
        ops.dec_flow_pts(proj, mlp, tab, pl, op, got, flags=fl, status=status)
        assert torch.equal(got, ref), (mode, flow_scale, s)
        # the operand is the whole-grid HRfeat of the shifted query at the remapped pixel
        ry, rx = torch.from_numpy(tab.hr_y[y]).cuda().long(), torch.from_numpy(tab.hr_x[x]).cuda().long()
        assert torch.equal(op, torch.stack([hrf[b][ry[b], rx[b]] for b in range(2)]))
    assert int(status.item()) & 8 == 0


# ---- 5: against the oracle
@pytest.mark.parametrize("mode", MODES)
def test_points_match_the_oracle(lats, mode):
    """437 points of the 37 x 45 grid with flows of several pixels against O.decoding_localensemble on the engine's
    own latent, per item.  Bound per element, as tests/test_gpu_ensemble.py::test_ensemble_meets_the_oracle: each of
    the four decodes meets the project's bar, so the blend is within sum_k w_k (RTOL |p_k| + ATOL); the engine's
    blend adds four fp32 roundings, 4 * 2^-23 * sum_k w_k |p_k|."""
    la, (HH, WW) = lats(mode, 64.0), GRIDS[0]
    y, x = points(HH, WW, 437)
    feat, inp = la.m.feat.cpu().numpy(), la.m.inp.cpu().numpy()
    got = [pts(la.m, y, x, torch.tensor(t), (HH, WW)).double().cpu().numpy() for t in TIMES]
    for b in range(2):
        ts = [F32(t[b]) for t in TIMES]
        ref = O.decoding_localensemble(feat[b:b + 1], inp[b:b + 1], ts, la.sd, (HH, WW))
        ps, areas = [], []
        for vx in (-1, 1):
            for vy in (-1, 1):
                p, a = O._decode(feat[b:b + 1], inp[b:b + 1], ts, la.sd, HH, WW, np.float64, shift=(vx, vy))
                ps.append(p)
                areas.append(a)
        tot = areas[0] + areas[1] + areas[2] + areas[3]
        ws = [(areas[3 - k] / tot).reshape(1, HH, WW) for k in range(4)]
        for q in range(len(TIMES)):
            pk = [ps[k][q][0] for k in range(4)]
            lim = sum(w * (RTOL * np.abs(p) + ATOL) for w, p in zip(ws, pk)) + \
                4 * 2.0 ** -23 * sum(w * np.abs(p) for w, p in zip(ws, pk))
            d = np.abs(got[q][b] - ref[q][:, y[b], x[b]])
            lim = lim[:, y[b], x[b]]
            print(f"ensemble points vs oracle {mode} t={ts[q]} item {b}: max err / limit "
                  f"{float((d / lim).max()):.3f}, max err {float(d.max()):.3e}")
            assert (d <= lim).all(), (mode, ts[q], b, float((d / lim).max()), float(d.max()))


# ---- 6: index safety
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


def test_return_flow_is_rejected(lats):
    la, grid = lats("f32"), GRIDS[0]
    y, x = points(*grid, 17)
    with pytest.raises(ValueError, match="return_flow"):
        pts(la.m, y, x, 0.3, grid, return_flow=True)
