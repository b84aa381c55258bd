"""Time fields on the GPU: decoder stages 1 and 2 and model.decoding with a query time per output pixel.

The field variants of k_dec1 (MODE 0 / 1, whole grid and windowed), k_dec2<false, 0, WIN> (f32) and k_dec2q<WIN> (f16x3)
are checked three ways: against the oracle composite (tests/timefield_inputs.py: the unchanged oracle stages, one call
per distinct value, selected per pixel) within the project bound |gpu - oracle| <= 1e-4 |oracle| + 1e-6; bit for bit
against the scalar launches (a pixel whose field value is v gets what the launch with t = v gives it); and bit for bit
across the ways a field can be laid out in memory (dense, item-broadcast, row field, a crop of a larger NaN-filled
tensor -- a read outside the field shows as NaN).  tests/test_timefield_host.py shows that a field read one row or
column off, flipped, or replaced by its mean breaks the bound by more than 10x at every pixel concerned.

Shapes: the latent of tests/test_gpu_decoder_stages.py (seeded 16 x 20 pair, B = 2, one model per operand mode); grid
37 x 45 -- 2 * 1665 pixels are no multiple of the 128 pixels a workgroup of any of the three kernels takes (tail lanes
exist) and 1665 is no multiple of 32 or 16 (one wave straddles the two items); WINDOW and an F rectangle around it
with a different margin on every side."""
import os

import numpy as np
import pytest
import torch

import stage2_inputs as S
import timefield_inputs as TF

pytestmark = pytest.mark.gpu
F32 = np.float32
MODES = ["f16x3", "f32"]
HH, WW = 37, 45
WINDOW = (9, 11, 13, 17)
FRECT = (5, 6, 21, 29)
FIELD = TF.random_field(2, HH, WW)                # [2,37,45], a different seed per item; read only


class Lat:
    """A model of one operand mode with the latent of the seeded pair."""

    def __init__(self, stif, sd, mode):
        self.m = stif.LunaTokis(64, 6, 8, 5, 40, mfma=mode)
        self.m.load_state_dict(sd, strict=True)
        x = torch.rand(2, 2, 3, 16, 20, generator=torch.Generator().manual_seed(77)).cuda()
        with torch.no_grad():
            self.m.gen_feat(x)
            self.proj = self.m._projection()
        self.feat = self.m.feat.cpu().numpy()            # [B,3,64,H,W]
        self.inp = self.m.inp.cpu().numpy()              # [B,2,3,H,W]
        self.mlp, self.tab, self.flags = self.m.layers["dec.mlp"], self.m._tab(16, 20, HH, WW), self.m._dec_flags


_LATS, _ORACLE1, _GPU1 = {}, {}, {}


@pytest.fixture(scope="module")
def lats(stif, sd):
    def get(mode):
        if mode not in _LATS:
            _LATS[mode] = Lat(stif, sd, mode)
        return _LATS[mode]
    yield get
    _LATS.clear(), _ORACLE1.clear(), _GPU1.clear()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def vec(v):
    return torch.full((2,), float(v), dtype=torch.float32, device="cuda")


def in_nan_canvas(field):
    """``field`` [B,HH,WW] as a crop of a larger NaN-filled device tensor (row pitch > WW, item pitch > HH * pitch)."""
    big = torch.full((field.shape[0], HH + 5, WW + 7), float("nan"), device="cuda")
    big[:, 2:2 + HH, 3:3 + WW] = dev(field)
    return big[:, 2:2 + HH, 3:3 + WW]


def stage1_oracle(la, mode, sd):
    """Per mode (each mode's model makes its own latent): the oracle's stage 1 per value, read only."""
    if mode not in _ORACLE1:
        per = TF.stage1_per_value(la.feat, la.inp, TF.VALUES, sd, HH, WW)
        for h, f in per.values():
            h.setflags(write=False), f.setflags(write=False)
        _ORACLE1[mode] = per
    return _ORACLE1[mode]


def run_stage1(la, ops, t, window=None, with_flow=True):
    """One ops.dec_stage1 call (t: a [2] vector or an ops.DecTime) into fresh NaN buffers -> (hrfeat, flow)."""
    if window is None:
        hs, fs = (HH, WW), (HH, WW)
    else:
        hs, fs = ((window.fh, window.fw) if window.fh or window.fw else (window.hh, window.ww)), (window.hh, window.ww)
    hrf = torch.full((2, *hs, 64), float("nan"), device="cuda")
    flow = torch.full((2, *fs, 4), float("nan"), device="cuda") if with_flow else None
    ops.dec_stage1(la.proj, la.mlp, la.tab, t, hrf, flow, flags=la.flags, window=window)
    torch.cuda.synchronize()
    return hrf, flow


def stage1_field(la, ops, mode):
    """The whole-grid stage 1 of FIELD (dense), shared and read only."""
    if mode not in _GPU1:
        _GPU1[mode] = run_stage1(la, ops, ops.DecTime.of(dev(FIELD)))
    return _GPU1[mode]


def check(tag, got, ref):
    ratio = S.bound_ratio(got, ref)
    worst = float(ratio.max())
    print(f"{tag}: worst |gpu - oracle| / bound = {worst:.4f}, max |d| = {float(np.abs(got - ref).max()):.3e}")
    assert worst <= 1.0, (tag, worst, np.unravel_index(int(ratio.argmax()), ratio.shape))


# ----------------------------------------------------------------------------- stage 1
@pytest.mark.parametrize("mode", MODES)
def test_stage1_field_matches_the_oracle_composite(stif, sd, lats, mode):
    """k_dec1<0, false, ., false, TF> over the whole grid: HRfeat and flow of every pixel against the oracle call of
    the pixel's own value."""
    la = lats(mode)
    hrf, flow = (x.cpu().numpy() for x in stage1_field(la, stif.ops, mode))
    assert np.isfinite(hrf).all() and np.isfinite(flow).all()
    ref_h, ref_f = TF.stage1_composite(stage1_oracle(la, mode, sd), FIELD)
    check(f"stage1 field {mode} hrfeat", hrf, ref_h)
    check(f"stage1 field {mode} flow", flow, ref_f)


@pytest.mark.parametrize("mode", MODES)
def test_stage1_field_is_the_scalar_launch_of_each_value(stif, lats, mode):
    """At the pixels of each value v, bit-identical to the scalar launch with t = v (fused and feat-only kernel)."""
    la, ops = lats(mode), stif.ops
    hrf, flow = stage1_field(la, ops, mode)
    hrf1, _ = run_stage1(la, ops, ops.DecTime.of(dev(FIELD)), with_flow=False)      # k_dec1<1, ., TF>, whole grid
    assert torch.equal(hrf1, hrf)
    seen = torch.zeros(2, HH, WW, dtype=torch.bool, device="cuda")
    for v in TF.VALUES:
        sh, sf = run_stage1(la, ops, vec(v))
        m = dev(FIELD == v)
        assert torch.equal(hrf[m], sh[m]) and torch.equal(flow[m], sf[m]), float(v)
        seen |= m
    assert bool(seen.all())


@pytest.mark.parametrize("form", ["query", "inside_f", "feat_only"])
@pytest.mark.parametrize("mode", MODES)
def test_stage1_field_window_is_the_crop(stif, lats, mode, form):
    """The windowed field kernels against the crop of the whole-grid field result, bit for bit: the field is indexed
    by the coordinates of the virtual grid, and the feat-only pass over FRECT reads it at F's pixels, outside WINDOW.
    The field is handed over as a crop of a NaN canvas, so a read at the rectangle's own coordinates -- or anywhere
    else outside the field -- cannot pass."""
    la, ops = lats(mode), stif.ops
    full_h, full_f = stage1_field(la, ops, mode)
    t = ops.DecTime.of(in_nan_canvas(FIELD))
    y0, x0, hh, ww = WINDOW
    fy0, fx0, fh, fw = FRECT
    crop = lambda a, r: a[:, r[0]:r[0] + r[2], r[1]:r[1] + r[3]]
    if form == "query":
        hrf, flow = run_stage1(la, ops, t, window=ops.dec_window(WINDOW, HH, WW))
        assert torch.equal(hrf, crop(full_h, WINDOW)) and torch.equal(flow, crop(full_f, WINDOW))
    elif form == "inside_f":
        hrf, flow = run_stage1(la, ops, t, window=ops.dec_window(WINDOW, HH, WW, FRECT))
        assert torch.equal(flow, crop(full_f, WINDOW))
        inside = torch.zeros(fh, fw, dtype=torch.bool, device="cuda")
        inside[y0 - fy0:y0 - fy0 + hh, x0 - fx0:x0 - fx0 + ww] = True
        assert torch.equal(hrf[:, inside], crop(full_h, WINDOW).reshape(2, hh * ww, 64))
        assert torch.isnan(hrf[:, ~inside]).all()
    else:
        hrf, flow = run_stage1(la, ops, t, window=ops.dec_window(FRECT, HH, WW), with_flow=False)
        assert flow is None and torch.equal(hrf, crop(full_h, FRECT))


# ----------------------------------------------------------------------------- stage 2
def run_stage2(la, ops, hrf, flow, t, window=None, frect=None):
    """One ops.dec_stage2 call on synthetic inputs (numpy, whole grid; cropped here for a window) -> (out, status).
    Windowed: written into a view of a NaN-filled whole-grid tensor, which is returned."""
    out = torch.full((2, 3, HH, WW), float("nan"), device="cuda")
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    if window is None:
        ops.dec_stage2(la.proj, la.mlp, dev(hrf), dev(flow), la.tab, t, out, flags=la.flags, status=st)
    else:
        y0, x0, hh, ww = window
        fy0, fx0, fh, fw = frect
        ops.dec_stage2(la.proj, la.mlp, dev(hrf[:, fy0:fy0 + fh, fx0:fx0 + fw]), dev(flow[:, y0:y0 + hh, x0:x0 + ww]),
                       la.tab, t, out[:, :, y0:y0 + hh, x0:x0 + ww], flags=la.flags, status=st,
                       window=ops.dec_window(window, HH, WW, frect))
    torch.cuda.synchronize()
    return out, int(st.item())


def stage2_frect(la, ops, flow):
    """The F rectangle of WINDOW for these flows (stif_dec_bounds), as model._window_steps derives it."""
    y0, x0, hh, ww = WINDOW
    box = torch.empty(4, dtype=torch.int32, device="cuda")
    ops.dec_bounds(dev(flow[:, y0:y0 + hh, x0:x0 + ww]), la.tab, box, ops.dec_window(WINDOW, HH, WW))
    ymin, ymax, xmin, xmax = box.tolist()
    fy0, fx0 = min(ymin, y0), min(xmin, x0)
    return (fy0, fx0, max(ymax + 1, y0 + hh) - fy0, max(xmax + 1, x0 + ww) - fx0)


@pytest.mark.parametrize("kind", ["uniform", "huge", "integer"])
@pytest.mark.parametrize("mode", MODES)
def test_stage2_field_matches_the_oracle_and_the_scalar_launches(stif, sd, lats, mode, kind):
    """k_dec2q<false, false, TF> (f16x3) / k_dec2<false, 0, false, false, TF> (f32) over the whole grid on synthetic
    HRfeat and flows of several pixels, clamped flows and whole-pixel flows: against O.decode_stage2 composited per
    value, and bit for bit against the scalar launch of each value at that value's pixels."""
    la, ops = lats(mode), stif.ops
    hrf, flow = S.hrfeat(2, HH, WW), S.flows(kind, 2, HH, WW)
    out, st = run_stage2(la, ops, hrf, flow, ops.DecTime.of(dev(FIELD)))
    assert st == 0
    got = out.cpu().numpy()
    assert np.isfinite(got).all()
    check(f"stage2 field {mode} {kind}", got, TF.stage2_composite(la.feat, la.inp, hrf, flow, FIELD, sd, HH, WW))
    for v in TF.VALUES:
        so, st = run_stage2(la, ops, hrf, flow, vec(v))
        m = dev(FIELD == v)[:, None].expand(2, 3, HH, WW)
        assert st == 0 and torch.equal(out[m], so[m]), float(v)


@pytest.mark.parametrize("mode", MODES)
def test_stage2_field_window_matches_the_oracle_and_the_scalar_launches(stif, sd, lats, mode):
    """The windowed field kernels (k_dec2q<true, false, TF> / k_dec2<false, 0, true, false, TF>) with flows of several
    pixels and HRfeat over the F rectangle of stif_dec_bounds: the oracle composite's crop, nothing written outside
    the window, the field (a crop of a NaN canvas) read at the coordinates of the virtual grid, and the scalar windowed
    launches' bits."""
    la, ops = lats(mode), stif.ops
    y0, x0, hh, ww = WINDOW
    hrf, flow = S.hrfeat(2, HH, WW), S.flows("uniform", 2, HH, WW)
    frect = stage2_frect(la, ops, flow)
    assert frect[0] <= y0 - 3 and frect[1] <= x0 - 3
    out, st = run_stage2(la, ops, hrf, flow, ops.DecTime.of(in_nan_canvas(FIELD)), WINDOW, frect)
    assert st == 0
    got = out.cpu().numpy()
    inside = np.zeros((HH, WW), bool)
    inside[y0:y0 + hh, x0:x0 + ww] = True
    assert np.isnan(got[:, :, ~inside]).all() and np.isfinite(got[:, :, inside]).all()
    ref = TF.stage2_composite(la.feat, la.inp, hrf, flow, FIELD, sd, HH, WW)
    check(f"stage2 field window {mode}", got[:, :, y0:y0 + hh, x0:x0 + ww], ref[:, :, y0:y0 + hh, x0:x0 + ww])
    for v in TF.VALUES:
        so, st = run_stage2(la, ops, hrf, flow, vec(v), WINDOW, frect)
        m = dev((FIELD == v) & inside)[:, None].expand(2, 3, HH, WW)
        assert st == 0 and torch.equal(out[m], so[m]), float(v)


# ----------------------------------------------------------------------------- the ways a field lies in memory
def stride_forms(ops):
    """name -> (ops.DecTime, the dense [2,HH,WW] field it stands for)."""
    rows = TF.VALUES[np.random.default_rng(7).integers(0, 4, (2, HH, 1))]
    both = np.stack([FIELD[0], FIELD[0]])
    forms = {
        "item_broadcast": (ops.DecTime.of(dev(FIELD[:1])), both),                       # item = 0
        "item_expanded": (ops.DecTime.of(dev(FIELD[:1]).expand(2, HH, WW)), both),      # the same through a stride-0 view
        "row": (ops.DecTime.of(dev(rows)), np.broadcast_to(rows, (2, HH, WW)).copy()),  # col = 0
        "crop": (ops.DecTime.of(in_nan_canvas(FIELD)), FIELD),                          # row pitch > WW
    }
    assert forms["item_broadcast"][0].item == 0 and forms["item_expanded"][0].item == 0
    assert forms["row"][0].col == 0 and forms["row"][0].item == HH
    assert forms["crop"][0].row == WW + 7 and forms["crop"][0].item == (HH + 5) * (WW + 7)
    return forms


@pytest.mark.parametrize("form", ["item_broadcast", "item_expanded", "row", "crop"])
@pytest.mark.parametrize("mode", MODES)
def test_stride_forms_equal_the_dense_field(stif, lats, mode, form):
    """Stage 1 (HRfeat, flow) and stage 2 (RGB) of a field given through strides equal those of the dense field it
    stands for, bit for bit, and no NaN of the canvas around a cropped field is read."""
    la, ops = lats(mode), stif.ops
    t, dense = stride_forms(ops)[form]
    d = ops.DecTime.of(dev(dense))
    assert (d.item, d.row, d.col) == (HH * WW, WW, 1)
    h, f = run_stage1(la, ops, t)
    dh, df = run_stage1(la, ops, d)
    assert not torch.isnan(h).any() and not torch.isnan(f).any()
    assert torch.equal(h, dh) and torch.equal(f, df)
    hrf, flow = S.hrfeat(2, HH, WW), S.flows("uniform", 2, HH, WW)
    o, st = run_stage2(la, ops, hrf, flow, t)
    do, dst = run_stage2(la, ops, hrf, flow, d)
    assert st == 0 and dst == 0 and not torch.isnan(o).any() and torch.equal(o, do)


def test_dectime_slices_like_a_vector(stif):
    ops = stif.ops
    t = ops.DecTime.of(in_nan_canvas(np.stack([FIELD[0], FIELD[1], FIELD[0]])))
    s = t[1:3]
    assert s.shape == (2,) and s.c.t == t.c.t + 4 * t.item and (s.item, s.row, s.col) == (t.item, t.row, t.col)
    b = ops.DecTime.of(dev(FIELD[:1]))
    assert b[1:2] is b and b.shape == (None,)
    with pytest.raises(ValueError):
        ops.DecTime.of(torch.zeros(2, HH, WW))                       # not on the device
    with pytest.raises(ValueError):
        ops.DecTime.of(torch.zeros(HH, WW, device="cuda"))           # not [b, hh, ww]


# ----------------------------------------------------------------------------- model.decoding
@pytest.mark.parametrize("mode", MODES)
def test_decoding_constant_field_is_the_scalar_decode(lats, mode):
    """model.decoding with a constant field equals the scalar decode bit for bit: whole grid, window=, tile=."""
    m = lats(mode).m
    const = torch.full((HH, WW), 0.3125)
    scalar = [torch.tensor([[0.3125]])]
    with torch.no_grad():
        for kw in ({}, {"window": WINDOW}, {"tile": (16, 16)}):
            a = m.decoding([const], (HH, WW), **kw)[0]
            b = m.decoding(scalar, (HH, WW), **kw)[0]
            assert a.shape == b.shape and torch.equal(a, b), kw
    assert m.range_reruns == 0


@pytest.mark.parametrize("mode", MODES)
def test_decoding_field_windows_and_tiles_are_crops(lats, mode):
    """A random field's windowed and tiled decodes are the bit-identical crops of its whole decode, in every form the
    model takes a field in; the window's F rectangle is larger than the window, so the feat-only pass reads the field
    outside it.  decoding_pairs selects the field's items with the latent's."""
    m = lats(mode).m
    y0, x0, hh, ww = WINDOW
    field = dev(FIELD)
    with torch.no_grad():
        whole = m.decoding([field], (HH, WW))[0]
        assert tuple(whole.shape) == (2, 3, HH, WW) and bool(torch.isfinite(whole).all())
        win = m.decoding([in_nan_canvas(FIELD)], (HH, WW), window=WINDOW)[0]
        F = m.last_window_F
        tiled = m.decoding([torch.from_numpy(FIELD.copy()).reshape(2, 1, HH, WW)], (HH, WW), tile=(16, 16))[0]
        flat = m.decoding([field.reshape(2, HH * WW)], (HH, WW))[0]
        one = m.decoding_pairs([1], [field], (HH, WW))[0]
        both0 = m.decoding([field[0]], (HH, WW))[0]                     # [HH, WW]: every item the same field
    assert torch.equal(win, whole[:, :, y0:y0 + hh, x0:x0 + ww])
    assert F[2] * F[3] > hh * ww and F[0] <= y0 and F[1] <= x0 and F[0] + F[2] >= y0 + hh and F[1] + F[3] >= x0 + ww
    assert torch.equal(tiled, whole) and torch.equal(flat, whole)
    assert tuple(one.shape) == (1, 3, HH, WW) and torch.equal(one, whole[1:2])
    assert torch.equal(both0[0], whole[0]) and not torch.equal(both0[1], whole[1])
    assert m.range_reruns == 0


@pytest.mark.parametrize("case", ["random", "ramp"])
@pytest.mark.parametrize("mode", MODES)
def test_decoding_field_matches_the_reference(lats, golden, mode, case):
    """The reference's own decoding with a [1, HH*WW] time tensor (tests/golden/timefield_16x20.npz) against
    model.decoding on the engine's own gen_feat of the fixture's input, at the bar tests/test_gpu_model.py uses for
    decoders_16x20 (rtol 1e-4, atol 1e-6).  random: four values at the default 64 x 80, as [1, HH, WW]; ramp: one time
    per row at 37 x 45, in the reference's own [1, HH*WW] form."""
    m = lats(mode).m
    fx = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "timefield_16x20.npz"))
    field, ref = fx[f"{case}_field"], fx[f"{case}_out"]
    keep = m._feat, m.inp
    try:
        with torch.no_grad():
            m.gen_feat(torch.from_numpy(golden["model_16x20"]["x"]).cuda())
            if case == "random":
                out = m.decoding([torch.from_numpy(field)])[0]
            else:
                out = m.decoding([torch.from_numpy(field).reshape(1, -1)], field.shape[1:])[0]
    finally:
        m._feat, m.inp = keep
    got = out.cpu().numpy()
    assert got.shape == ref.shape
    check(f"decoding field {mode} {case} vs reference", got, ref)
