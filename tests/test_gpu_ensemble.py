"""The local ensemble for batches, windows, tiles and streamed video on the GPU: ``decoding(ensemble=True)`` is
bit-identical to ``decoding_localensemble`` item by item, a window or a tiling of it to the crop of the full ensemble
decode, it meets the oracle's blend of four shifted decodes at the project's tolerance plus the blend's roundings,
the windowed flow stage equals the whole-grid one and flags a too-small HRfeat rectangle instead of reading outside
it, the stream renderer passes the flag through, and the scratch is one shift's.  Setup as tests/test_gpu_window.py:
gen_feat of a seeded 16x20 pair, B = 2, a different time per item."""
import gc

import numpy as np
import pytest
import torch

from oracle import stif_oracle as O
from test_gpu_window import ATOL, FLOW_SCALE, GRIDS, LARGE_FLOW_SCALE, RTOL, TIMES, WNAMES, Lat, windows

pytestmark = pytest.mark.gpu
F32 = np.float32
MODES = ["f16x3", "f32"]
SCALES = [FLOW_SCALE, LARGE_FLOW_SCALE]
GRID_IDS = [f"{g[0]}x{g[1]}" for g in GRIDS]


class ELat(Lat):
    """test_gpu_window's latent with the full ensemble decodes computed once per grid."""

    def __init__(self, *a):
        super().__init__(*a)
        self.ens, self.ens_F, self.demo = {}, {}, {}

    def ensemble(self, grid, **kw):
        with torch.no_grad():
            return self.m.decoding(self.tq, grid, ensemble=True, **kw)

    def full_ensemble(self, grid):
        if grid not in self.ens:
            self.ens[grid] = [o.clone() for o in self.ensemble(grid)]
            self.ens_F[grid] = self.m.last_window_F
        return self.ens[grid]

    def localensemble_of_item(self, i, grid):
        """decoding_localensemble of item i alone at its query times, [len(TIMES), 3, HH, WW]: the latent is set to
        that item as decoding_pairs sets it, and put back."""
        if (i, grid) not in self.demo:
            m = self.m
            feat, inp = m._feat, m.inp
            idx = torch.tensor([i], device=feat.device, dtype=torch.long)
            m._feat, m.inp = feat.index_select(1, idx), inp.index_select(0, idx)
            try:
                with torch.no_grad():
                    self.demo[i, grid] = m.decoding_localensemble([ts[i] for ts in TIMES], grid).clone()
            finally:
                m._feat, m.inp = feat, inp
        return self.demo[i, grid]


@pytest.fixture(scope="module")
def lats(stif, sd):
    cache = {}

    def get(mode, flow_scale=FLOW_SCALE):
        if (mode, flow_scale) not in cache:
            cache[mode, flow_scale] = ELat(stif, sd, mode, flow_scale)
        return cache[mode, flow_scale]
    return get


# ---- 1: against the existing path
@pytest.mark.parametrize("flow_scale", SCALES)
@pytest.mark.parametrize("grid", GRIDS, ids=GRID_IDS)
@pytest.mark.parametrize("mode", MODES)
def test_batched_ensemble_equals_decoding_localensemble_item_by_item(lats, mode, grid, flow_scale):
    la = lats(mode, flow_scale)
    got = la.full_ensemble(grid)
    assert len(got) == len(TIMES)
    for q in range(len(TIMES)):
        assert tuple(got[q].shape) == (2, 3, *grid)
        for i in range(2):
            assert torch.equal(got[q][i], la.localensemble_of_item(i, grid)[q]), (mode, grid, flow_scale, q, i)
    assert la.ens_F[grid] == (0, 0, *grid)          # the whole grid: F is the whole grid, nothing is read back
    assert la.m.range_reruns == 0


# ---- 2: a window is the crop of the full ensemble decode
@pytest.mark.parametrize("wname", WNAMES)
@pytest.mark.parametrize("flow_scale", SCALES)
@pytest.mark.parametrize("grid", GRIDS, ids=GRID_IDS)
@pytest.mark.parametrize("mode", MODES)
def test_ensemble_window_is_the_crop_of_the_full_ensemble_decode(lats, mode, grid, flow_scale, wname):
    la = lats(mode, flow_scale)
    y0, x0, hh, ww = windows(*grid)[wname]
    full = la.full_ensemble(grid)
    got = la.ensemble(grid, window=(y0, x0, hh, ww))
    fy0, fx0, fh, fw = F = la.m.last_window_F
    assert 0 <= fy0 and 0 <= fx0 and fy0 + fh <= grid[0] and fx0 + fw <= grid[1]
    assert len(got) == len(full)
    for g, f in zip(got, full):
        assert tuple(g.shape) == (2, 3, hh, ww)
        assert torch.equal(g, f[:, :, y0:y0 + hh, x0:x0 + ww]), (mode, grid, flow_scale, wname, F)
    assert la.m.range_reruns == 0
    if wname == "interior" and flow_scale == LARGE_FLOW_SCALE:
        grown = (y0 - fy0, x0 - fx0, fy0 + fh - (y0 + hh), fx0 + fw - (x0 + ww))
        print("large flows", mode, grid, "interior window", (y0, x0, hh, ww), "largest F of the four shifts", F,
              "grown by (top, left, bottom, right)", grown)
        assert max(grown) >= 3, (F, grown)


# ---- 3: tiles, and a selection of pairs
@pytest.mark.parametrize("grid", GRIDS, ids=GRID_IDS)
@pytest.mark.parametrize("mode", MODES)
def test_tiled_ensemble_equals_untiled_and_pairs_are_the_permuted_slices(lats, mode, grid):
    la = lats(mode)
    full = la.full_ensemble(grid)
    got = la.ensemble(grid, tile=(16, 24))
    for g, f in zip(got, full):
        assert tuple(g.shape) == (2, 3, *grid) and torch.equal(g, f)
    with torch.no_grad():
        sel = la.m.decoding_pairs([1, 0], [t[[1, 0]] for t in la.tq], grid, ensemble=True)
    for s, f in zip(sel, full):
        assert torch.equal(s, f[[1, 0]])
    assert la.m.feat.shape[0] == 2                   # the latent is left as it was


# ---- 4: against the oracle
@pytest.mark.parametrize("flow_scale", SCALES)
@pytest.mark.parametrize("grid", GRIDS, ids=GRID_IDS)
@pytest.mark.parametrize("mode", MODES)
def test_ensemble_meets_the_oracle(lats, mode, grid, flow_scale):
    """ref = sum_k w_k p_k with p_k the oracle's decode of shift k (float64, the engine's own latent) and w_k the
    diagonally opposite area over the total.  Bound per element: each decode meets the project's bar, so the blend
    of the four is within sum_k w_k (RTOL |p_k| + ATOL); the engine's blend adds four fp32 roundings,
    4 * 2^-23 * sum_k w_k |p_k|."""
    la = lats(mode, flow_scale)
    HH, WW = grid
    got = la.full_ensemble(grid)
    feat = la.m.feat.cpu().numpy()
    x = la.x.cpu().numpy()
    for b in range(2):
        ts = [F32(row[b]) for row in TIMES]
        ps, areas = [], []
        for vx in (-1, 1):
            for vy in (-1, 1):
                p, a = O._decode(feat[b:b + 1], x[b:b + 1], ts, la.sd, HH, WW, np.float64, shift=(vx, vy))
                ps.append(p)
                areas.append(a)
        tot = areas[0] + areas[1] + areas[2] + areas[3]
        ws = [(areas[3 - k] / tot).reshape(1, HH, WW) for k in range(4)]      # the reference's swap (:1079-1080)
        for q in range(len(TIMES)):
            pk = [ps[k][q][0] for k in range(4)]
            ref = sum(w * p for w, p in zip(ws, pk))
            lim = sum(w * (RTOL * np.abs(p) + ATOL) for w, p in zip(ws, pk)) + \
                4 * 2.0 ** -23 * sum(w * np.abs(p) for w, p in zip(ws, pk))
            d = np.abs(got[q][b].double().cpu().numpy() - ref)
            print(mode, grid, flow_scale, "item", b, "query", q, "max |got - ref| / bound", float((d / lim).max()),
                  "max |got - ref|", float(d.max()))
            assert (d <= lim).all(), (mode, grid, flow_scale, b, q, float((d / lim).max()), float(d.max()))


# ---- 5: the flow stage on its own
@pytest.mark.parametrize("wname", ["interior", "bottom_right"])
@pytest.mark.parametrize("grid", GRIDS, ids=GRID_IDS)
@pytest.mark.parametrize("mode", MODES)
def test_flow_stage_over_a_window(stif, lats, mode, grid, wname):
    """stif_dec_flow_win over a window, HRfeat cropped to the remap rectangle, against the flow of stif_dec_stage1_ex
    with the same remap tables over the whole grid: same bits, status 0.  Then with F one row short of the remap
    rectangle (every argument valid): the call completes, bit 2 is reported, the rows that did not need the missing
    row are unchanged."""
    la = lats(mode)
    m, ops = la.m, stif.ops
    HH, WW = grid
    n = 2
    rect = y0, x0, hh, ww = windows(HH, WW)[wname]
    gen = torch.Generator().manual_seed(13)
    proj = (torch.rand(n, 16, 20, 256, generator=gen) - 0.5).cuda()
    t = torch.tensor([0.3, 0.7], device="cuda")
    mlp, fl = m.layers["dec.mlp"], m._dec_flags
    for shift in ops.ENSEMBLE_SHIFTS:
        tab = m._tab(16, 20, HH, WW, shift)
        hrf = torch.empty(n, HH, WW, 64, device="cuda")
        flow = torch.empty(n, HH, WW, 4, device="cuda")
        ops.dec_stage1(proj, mlp, tab, t, hrf, flow, flags=fl)
        want = flow[:, y0:y0 + hh, x0:x0 + ww]
        ry0, rx0, rh, rw = rrect = tab.remap_rect(rect)
        hy = stif.coords.dec_tables(16, 20, HH, WW, shift)["hr_y"]
        assert (ry0, ry0 + rh - 1) == (hy[y0], hy[y0 + hh - 1])
        st = torch.zeros(1, dtype=torch.int32, device="cuda")
        got = torch.full((n, hh, ww, 4), float("nan"), device="cuda")
        ops.dec_flow_win(proj, mlp, tab, t, hrf[:, ry0:ry0 + rh, rx0:rx0 + rw].contiguous(), got, flags=fl, status=st,
                         window=ops.dec_window(rect, HH, WW, rrect))
        assert int(st.item()) == 0
        assert torch.equal(got, want), (mode, grid, wname, shift)
        # F one row short at the bottom
        short = (ry0, rx0, rh - 1, rw)
        got = torch.full((n, hh, ww, 4), float("nan"), device="cuda")
        ops.dec_flow_win(proj, mlp, tab, t, hrf[:, ry0:ry0 + rh - 1, rx0:rx0 + rw].contiguous(), got, flags=fl,
                         status=st, window=ops.dec_window(rect, HH, WW, short))
        torch.cuda.synchronize()
        assert int(st.item()) & 4
        inside = torch.from_numpy(hy[y0:y0 + hh] < ry0 + rh - 1).cuda()
        assert bool(inside.any()) and not bool(inside.all())
        assert torch.equal(got[:, inside], want[:, inside])
        assert bool(torch.isfinite(got).all())


# ---- 6: streaming
SH, SW = 14, 18                   # padded to 16 x 20; outputs 56 x 72 of the padded frame's 64 x 80 grid
_MODELS, _REF = {}, {}


def stream_model(stif, sd):
    if "m" not in _MODELS:
        m = stif.LunaTokis(64, 6, 8, 5, 40, mfma="f16x3")
        m.load_state_dict(sd, strict=True)
        _MODELS["m"] = m
    return _MODELS["m"]


def clip(n):
    return torch.rand(n, 3, SH, SW, generator=torch.Generator().manual_seed(2024)).cuda()


def stream_reference(stif, sd, frames, key, pair, t, ensemble=True):
    key = (key, float(t), ensemble)
    if key not in _REF:
        _REF[key] = stif.video.run_sequence(stream_model(stif, sd), frames, times=[float(t)], ensemble=ensemble)
    return _REF[key][pair][0][:, :4 * SH, :4 * SW]


@pytest.mark.parametrize("chunk", [1, 3])
def test_stream_with_ensemble_is_bit_identical_to_run_sequence(stif, sd, chunk):
    V = stif.video
    n = 5
    sched = list(V.frame_schedule(25, 50, n))
    outs = list(V.render_stream(stream_model(stif, sd), iter(clip(n)), 25, 50, scale=4, chunk_pairs=chunk,
                                ensemble=True))
    assert len(outs) == len(sched)
    plain = 0
    for o, (pair, t) in zip(outs, sched):
        assert tuple(o.shape) == (3, 4 * SH, 4 * SW)
        assert torch.equal(o, stream_reference(stif, sd, clip(n), "clip", pair, t)), (pair, t)
        plain += int(torch.equal(o, stream_reference(stif, sd, clip(n), "clip", pair, t, ensemble=False)))
    assert plain < len(outs)                         # the ensemble is another picture than the plain decode


def test_stream_without_the_flag_is_unchanged_and_held_frames_take_the_ensemble(stif, sd):
    V = stif.video
    m = stream_model(stif, sd)
    n = 4
    frames = clip(n)
    sched = list(V.frame_schedule(25, 50, n))
    outs = list(V.render_stream(m, iter(frames), 25, 50, scale=4, chunk_pairs=2))
    pair, t = sched[1]
    assert torch.equal(outs[1], V.run_sequence(m, frames, times=[float(t)])[pair][0][:, :4 * SH, :4 * SW])
    # pair 1 forced to a cut: its outputs repeat frame 1 (t < 1/2) or frame 2, rendered standing still -- with the
    # ensemble when it is asked for
    held = list(V.render_stream(m, iter(frames), 25, 50, scale=4, chunk_pairs=2, hold_pairs=[1], ensemble=True))
    assert len(held) == len(sched)
    seen = 0
    for o, (pair, t) in zip(held, sched):
        if pair != 1:
            continue
        f = frames[1 if 2 * t < 1 else 2]
        want = stream_reference(stif, sd, torch.stack([f, f]), ("held", 1 if 2 * t < 1 else 2), 0, 0.0)
        assert torch.equal(o, want), (pair, t)
        seen += 1
    assert seen == 2


# ---- 7: scratch
def test_ensemble_scratch_is_one_shifts(lats):
    la = lats("f16x3")
    grid = (64, 80)
    la.ensemble(grid, window=windows(*grid)["interior"])
    win_peak = la.m.window_peak_scratch_bytes
    la.ensemble(grid)
    whole_peak = la.m.window_peak_scratch_bytes
    print("window_peak_scratch_bytes: interior window", win_peak, "whole grid", whole_peak)
    assert 0 < win_peak < whole_peak

    m = la.m
    feat, inp = m._feat, m.inp
    idx = torch.tensor([0], device=feat.device, dtype=torch.long)
    m._feat, m.inp = feat.index_select(1, idx), inp.index_select(0, idx)
    peaks = {}
    try:
        for name, fn in (("ensemble", lambda: m.decoding([0.3], grid, ensemble=True)),
                         ("localensemble", lambda: m.decoding_localensemble([0.3], grid))):
            with torch.no_grad():
                fn()                                 # tables and weight maps exist after this
                gc.collect()
                torch.cuda.synchronize()
                base = torch.cuda.memory_allocated()
                torch.cuda.reset_peak_memory_stats()
                out = fn()
                torch.cuda.synchronize()
                peaks[name] = torch.cuda.max_memory_allocated() - base
                del out
    finally:
        m._feat, m.inp = feat, inp
    print("peak bytes above the level before the call:", peaks)
    assert peaks["ensemble"] < peaks["localensemble"]
