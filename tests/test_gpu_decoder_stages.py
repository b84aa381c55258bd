"""Decoder stage 2 on its own, and the decoder at the edges of its grid shapes, against the CPU oracle.

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

import stage2_inputs as S
from oracle import stif_oracle as O

pytestmark = pytest.mark.gpu
F32 = np.float32
T_ITEMS = [0.3, 0.7]                          # a different time per item
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
        self._proj, self._hr = {}, None

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
