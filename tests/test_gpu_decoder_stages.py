"""Decoder stages 1 and 2 on their own, and the decoder at the edges of its grid shapes, against the CPU oracle.

Stage 1 (k_dec1) is called through ops.dec_stage1 on the model's own latent and checked on both of its outputs,
HRfeat and flow, against oracle.decode_stage1.  The RGB cannot pin them: with make_state_dict's initialisation the
flows are ~0.03 HR pixels and stage 2 attenuates an error in them by two orders of magnitude (tests/test_oracle.py
asserts at least 50x), while every wrong stage 1 tried there -- the other item's time, the wrong image, table or
HRfeat row, replicate padding -- breaks the bound on one of the two outputs by at least 190x.  Every one of the 18
k_dec1<MODE, HRIMG, F16, WIN> instantiations runs in at least one test (F16 1 / 0 = the modes f16x3 / f32):
  <0, false|true, *, false>  test_stage1_matches_the_oracle, the whole-grid cases with the LR / the HR image
  <1, false, *, false>       the same test's shifted cases (the local ensemble: HRfeat map first, then the flow stage)
  <2, false, *, false>       its shifted cases with the LR image
  <2, true, *, false>        its shifted cases with the HR image (no model call asks for this form)
  <0, false|true, *, true>   test_stage1_window_is_the_crop, forms `query` and `inside_f`
  <1, false|true, *, true>   its form `feat_only`
and the whole-grid and the ensemble form are launched per item and three times over
(test_stage1_items_are_independent_and_launches_repeat).  The cases are tests/stage1_cases.py.

Stage 2 (k_dec2 / k_dec2q, their windowed and HR-image variants) is called through ops.dec_stage2 with synthetic
HRfeat and flows (tests/stage2_inputs.py) that no SIREN-initialised model produces: flows of several HR pixels,
flows clamped at the frame edge, whole-pixel flows, and grids on the clamp value or one ulp inside it.  The kernel
and oracle.decode_stage2 read the same fp32 tensors; tests/test_oracle.py shows that a wrong divisor, padding rule,
warp base, x/y order or grid order breaks the bound by two orders of magnitude on these inputs.  The end-to-end
part decodes at the smallest grids the ABI takes, at scale 1 and below it.

Latent: gen_feat of a seeded 16x20 pair, B = 2 (as tests/test_gpu_window.py), one model per operand mode.
Bound everywhere: |gpu - oracle| <= 1e-4 |oracle| + 1e-6, the project's oracle tolerance."""
import numpy as np
import pytest
import torch

import stage1_cases as C1
import stage2_inputs as S
from oracle import stif_oracle as O

pytestmark = pytest.mark.gpu
F32 = np.float32
T_ITEMS = C1.T_ITEMS                          # a different time per item
MODES = ["f16x3", "f32"]
WINDOW = (9, 11, 13, 17)                      # of 37 x 45


class Lat:
    """A model of one operand mode with the latent of the seeded pair, and what every case of it shares."""

    def __init__(self, stif, sd, mode):
        self.m = stif.LunaTokis(64, 6, 8, 5, 40, mfma=mode)
        self.m.load_state_dict(sd, strict=True)
        x = torch.rand(2, 2, 3, 16, 20, generator=torch.Generator().manual_seed(77)).cuda()
        with torch.no_grad():
            self.m.gen_feat(x)
        self.feat = self.m.feat.cpu().numpy()            # [B,3,64,H,W]
        self.inp = self.m.inp.cpu().numpy()              # [B,2,3,H,W]
        self.t = torch.tensor(T_ITEMS, dtype=torch.float32, device="cuda")
        self._proj, self._hr, self._img = {}, None, {}

    def proj(self, image):
        if image not in self._proj:
            with torch.no_grad():
                self._proj[image] = self.m._projection(lr_image=not image)
        return self._proj[image]

    def hr_image(self):
        """decoding_test's HRinp as the oracle builds it: the x4 bilinear upsample of the pair, [B,6,4H,4W]."""
        if self._hr is None:
            self._hr = O.upsample_bilinear(self.inp.reshape(2, 6, 16, 20), 4)
        return self._hr


    def image(self, ops, HH, WW, shift=None):
        """The HR image on the device with its tables at the (shifted) HH x WW query grid."""
        if (HH, WW, shift) not in self._img:
            self._img[HH, WW, shift] = ops.DecImageDev(self.m.inp, 4, HH, WW, shift)
        return self._img[HH, WW, shift]


@pytest.fixture(scope="module")
def lats(stif, sd):
    cache = {}

    def get(mode):
        if mode not in cache:
            cache[mode] = Lat(stif, sd, mode)
        return cache[mode]
    return get


def check(tag, got, ref):
    ratio = S.bound_ratio(got, ref)
    worst = float(ratio.max())
    print(f"{tag}: worst |gpu - oracle| / bound = {worst:.4f}, max |d| = {float(np.abs(got - ref).max()):.3e}")
    assert worst <= 1.0, (tag, worst, np.unravel_index(int(ratio.argmax()), ratio.shape))


# ----------------------------------------------------------------------------- stage 1
# Per (operand mode, case): the oracle's (hrfeat, flow) -- each mode's model makes its own latent, so the key holds
# the mode -- and the whole-grid GPU result the window and the per-item launches are compared with.  Read only.
_ORACLE1, _GPU1 = {}, {}
FRECT = (5, 6, 21, 29)                        # an F rectangle around WINDOW with a different margin on every side


def stage1_oracle(la, mode, sd, case):
    if (mode, case) not in _ORACLE1:
        (HH, WW), image, shift = case
        ref = O.decode_stage1(la.feat, la.inp, np.array(T_ITEMS, F32), sd, HH, WW,
                              img=la.hr_image() if image else None, shift=shift)
        for r in ref:
            r.setflags(write=False)
        _ORACLE1[mode, case] = ref
    return _ORACLE1[mode, case]


def run_stage1(la, ops, case, items=(0, 2), window=None, with_flow=True):
    """One ops.dec_stage1 call for the items [a, b) into fresh NaN buffers -> (hrfeat, flow) on the device."""
    (HH, WW), image, shift = case
    a, b = items
    n = b - a
    img = la.image(ops, HH, WW, shift).items(a, b) if image else None
    if window is None:
        hs, fs = (HH, WW), (HH, WW)
    else:
        hs, fs = ((window.fh, window.fw) if window.fh or window.fw else (window.hh, window.ww)), (window.hh, window.ww)
    hrf = torch.full((n, *hs, 64), float("nan"), device="cuda")
    flow = torch.full((n, *fs, 4), float("nan"), device="cuda") if with_flow else None
    ops.dec_stage1(la.proj(image)[a:b], la.m.layers["dec.mlp"], la.m._tab(16, 20, HH, WW, shift), la.t[a:b], hrf, flow,
                   img, flags=la.m._dec_flags, window=window)
    torch.cuda.synchronize()
    return hrf, flow


def stage1_whole(la, ops, mode, case):
    if (mode, case) not in _GPU1:
        _GPU1[mode, case] = run_stage1(la, ops, case)
    return _GPU1[mode, case]


@pytest.mark.parametrize("case", C1.CASES, ids=[C1.case_id(c) for c in C1.CASES])
@pytest.mark.parametrize("mode", MODES)
def test_stage1_matches_the_oracle(stif, sd, lats, mode, case):
    """ops.dec_stage1 over the whole grid, HRfeat and flow against oracle.decode_stage1.  Without a shift: the fused
    k_dec1<0, HRIMG>.  With one (the local ensemble's tables with hr_y / hr_x): k_dec1<1, false> for the HRfeat map,
    then k_dec1<2, HRIMG>, whose flow stage reads HRfeat at the HR pixel nearest to the shifted query and, with the
    HR image, samples it at that query too.  The batch is 2 and 37 x 45 is 1665 pixels per item, so a 128-pixel
    workgroup straddles the items and the last one is partial."""
    la, ops = lats(mode), stif.ops
    hrf, flow = (x.cpu().numpy() for x in stage1_whole(la, ops, mode, case))
    assert np.isfinite(hrf).all() and np.isfinite(flow).all()
    ref_h, ref_f = stage1_oracle(la, mode, sd, case)
    tag = f"stage1 {mode} {C1.case_id(case)}"
    worst = [float(S.bound_ratio(g, r).max()) for g, r in ((hrf, ref_h), (flow, ref_f))]
    print(f"{tag}: worst |gpu - oracle| / bound: hrfeat {worst[0]:.4f}, flow {worst[1]:.4f}")
    check(tag + " hrfeat", hrf, ref_h)
    check(tag + " flow", flow, ref_f)


@pytest.mark.parametrize("form", ["query", "inside_f", "feat_only"])
@pytest.mark.parametrize("image", [False, True], ids=["lr", "hrimg"])
@pytest.mark.parametrize("mode", MODES)
def test_stage1_window_is_the_crop(stif, lats, mode, image, form):
    """stif_dec_stage1_win at 37 x 45 against the crop of the whole-grid result of the same mode and image, bit for
    bit.  query: HRfeat and flow over WINDOW.  inside_f: the same query with HRfeat held over the larger FRECT -- the
    query's rows land at their place in F and nothing else of the NaN-filled F buffer is written.  feat_only: HRfeat
    over FRECT with no flow, as _window_steps issues it (k_dec1<1, HRIMG, ., true>)."""
    la, ops = lats(mode), stif.ops
    HH, WW = 37, 45
    case = ((HH, WW), image, None)
    full_h, full_f = stage1_whole(la, ops, mode, case)
    y0, x0, hh, ww = WINDOW
    fy0, fx0, fh, fw = FRECT
    crop = lambda t, r: t[:, r[0]:r[0] + r[2], r[1]:r[1] + r[3]]
    if form == "query":
        hrf, flow = run_stage1(la, ops, case, window=ops.dec_window(WINDOW, HH, WW))
        assert torch.equal(hrf, crop(full_h, WINDOW)) and torch.equal(flow, crop(full_f, WINDOW))
    elif form == "inside_f":
        hrf, flow = run_stage1(la, ops, case, window=ops.dec_window(WINDOW, HH, WW, FRECT))
        assert tuple(hrf.shape) == (2, fh, fw, 64)
        assert torch.equal(flow, crop(full_f, WINDOW))
        inside = torch.zeros(fh, fw, dtype=torch.bool, device="cuda")
        inside[y0 - fy0:y0 - fy0 + hh, x0 - fx0:x0 - fx0 + ww] = True
        assert torch.equal(hrf[:, inside], crop(full_h, WINDOW).reshape(2, hh * ww, 64))
        assert torch.isnan(hrf[:, ~inside]).all()
    else:
        hrf, flow = run_stage1(la, ops, case, window=ops.dec_window(FRECT, HH, WW), with_flow=False)
        assert flow is None and torch.equal(hrf, crop(full_h, FRECT))


@pytest.mark.parametrize("shift", [None, (-1, 1)], ids=["whole", "ensemble"])
@pytest.mark.parametrize("mode", MODES)
def test_stage1_items_are_independent_and_launches_repeat(stif, lats, mode, shift):
    """At 37 x 45 with the LR image: item b of the two-item launch is the one-item launch of item b, and three
    launches into fresh NaN buffers agree, all bit for bit (a weight segment consumed before its DMA landed would
    show here first)."""
    la, ops = lats(mode), stif.ops
    case = ((37, 45), False, shift)
    full_h, full_f = stage1_whole(la, ops, mode, case)
    assert not torch.isnan(full_h).any() and not torch.isnan(full_f).any()
    for b in range(2):
        hrf, flow = run_stage1(la, ops, case, items=(b, b + 1))
        assert torch.equal(hrf[0], full_h[b]) and torch.equal(flow[0], full_f[b]), b
    for _ in range(3):
        hrf, flow = run_stage1(la, ops, case)
        assert torch.equal(hrf, full_h) and torch.equal(flow, full_f)


# ----------------------------------------------------------------------------- stage 2
STAGE2 = ([(False, g, k) for g in [(37, 45), (64, 80)] for k in S.KINDS] + [(True, (64, 80), k) for k in S.KINDS])


@pytest.mark.parametrize("image,grid,kind", STAGE2,
                         ids=[f"{'hrimg' if i else 'lr'}-{g[0]}x{g[1]}-{k}" for i, g, k in STAGE2])
@pytest.mark.parametrize("mode", MODES)
def test_stage2_matches_the_oracle(stif, sd, lats, mode, image, grid, kind):
    """ops.dec_stage2 over the whole grid: k_dec2q (f16x3), k_dec2<false, 0> (f32) and, with the HR image and the
    proj_hrimg projection, k_dec2<true, .> (decoding_test).  37 x 45: 1665 pixels per item, so a workgroup
    straddles the items and the total is no multiple of 16 or 128."""
    la, ops = lats(mode), stif.ops
    HH, WW = grid
    hrf, flow = S.hrfeat(2, HH, WW), S.flows(kind, 2, HH, WW)
    img = ops.DecImageDev(la.m.inp, 4, HH, WW) if image else None
    out = torch.full((2, 3, HH, WW), float("nan"), device="cuda")
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    ops.dec_stage2(la.proj(image), la.m.layers["dec.mlp"], torch.from_numpy(hrf).cuda(), torch.from_numpy(flow).cuda(),
                   la.m._tab(16, 20, HH, WW), la.t, out, img, flags=la.m._dec_flags, status=st)
    got = out.cpu().numpy()
    assert int(st.item()) == 0
    assert np.isfinite(got).all()
    ref = O.decode_stage2(la.feat, la.inp, hrf, flow, np.array(T_ITEMS, F32), sd, HH, WW,
                          img=la.hr_image() if image else None)
    check(f"stage2 {mode} {'hrimg' if image else 'lr'} {HH}x{WW} {kind}", got, ref)


@pytest.mark.parametrize("mode", MODES)
def test_stage2_window_matches_the_oracle(stif, sd, lats, mode):
    """stif_dec_stage2_win: the window's pixels with flows of several pixels, HRfeat cropped to the F rectangle of
    stif_dec_bounds, written into a view of a larger tensor -- the oracle's crop, and not a value outside it."""
    la, ops = lats(mode), stif.ops
    HH, WW = 37, 45
    y0, x0, hh, ww = WINDOW
    hrf, flow = S.hrfeat(2, HH, WW), S.flows("uniform", 2, HH, WW)
    tab = la.m._tab(16, 20, HH, WW)
    wflow = torch.from_numpy(np.ascontiguousarray(flow[:, y0:y0 + hh, x0:x0 + ww])).cuda()
    box = torch.empty(4, dtype=torch.int32, device="cuda")
    ops.dec_bounds(wflow, tab, box, ops.dec_window(WINDOW, HH, WW))
    ymin, ymax, xmin, xmax = box.tolist()
    fy0, fx0 = min(ymin, y0), min(xmin, x0)
    frect = (fy0, fx0, max(ymax + 1, y0 + hh) - fy0, max(xmax + 1, x0 + ww) - fx0)
    print("stage2 window", mode, "F rectangle", frect)
    assert fy0 <= y0 - 3 and fx0 <= x0 - 3 and fy0 + frect[2] >= y0 + hh + 3 and fx0 + frect[3] >= x0 + ww + 3
    hf = torch.from_numpy(np.ascontiguousarray(hrf[:, fy0:fy0 + frect[2], fx0:fx0 + frect[3]])).cuda()
    big = torch.full((2, 3, HH, WW), float("nan"), device="cuda")
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    ops.dec_stage2(la.proj(False), la.m.layers["dec.mlp"], hf, wflow, tab, la.t, big[:, :, y0:y0 + hh, x0:x0 + ww],
                   flags=la.m._dec_flags, status=st, window=ops.dec_window(WINDOW, HH, WW, frect))
    got = big.cpu().numpy()
    assert int(st.item()) == 0
    inside = np.zeros((HH, WW), bool)
    inside[y0:y0 + hh, x0:x0 + ww] = True
    assert np.isnan(got[:, :, ~inside]).all()
    assert np.isfinite(got[:, :, inside]).all()
    ref = O.decode_stage2(la.feat, la.inp, hrf, flow, np.array(T_ITEMS, F32), sd, HH, WW)
    check(f"stage2 window {mode}", got[:, :, y0:y0 + hh, x0:x0 + ww], ref[:, :, y0:y0 + hh, x0:x0 + ww])


# (2, 2) the smallest grid the ABI takes; one-row / one-column-pair strips; (16, 20) scale 1: rel ~ 0 and every nearest
# index the pixel itself; (7, 9) a downscale; (17, 21) one more than the latent
EDGE_GRIDS = [(2, 2), (2, 97), (61, 3), (16, 20), (7, 9), (17, 21)]


@pytest.mark.parametrize("grid", EDGE_GRIDS, ids=[f"{g[0]}x{g[1]}" for g in EDGE_GRIDS])
@pytest.mark.parametrize("mode", MODES)
def test_decoding_at_the_grid_shape_edges(sd, lats, mode, grid):
    la = lats(mode)
    HH, WW = grid
    with torch.no_grad():
        outs = la.m.decoding([torch.tensor(T_ITEMS, dtype=torch.float32).reshape(2, 1)], scale=grid)
    assert len(outs) == 1 and tuple(outs[0].shape) == (2, 3, HH, WW)
    assert la.m.range_reruns == 0
    ref = np.stack([O.decoding(la.feat[b:b + 1], la.inp[b:b + 1], [F32(t)], sd, grid)[0][0]
                    for b, t in enumerate(T_ITEMS)])
    check(f"decoding {mode} {HH}x{WW}", outs[0].cpu().numpy(), ref)
