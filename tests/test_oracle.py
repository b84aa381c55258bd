"""The CPU oracle against the golden fixtures produced by the reference itself
(tests/golden/make_golden.py).  CPU only."""
import os

import numpy as np
import pytest

from oracle import stif_oracle as O


def relmax(a, b):
    return float(np.abs(np.asarray(a, np.float64) - b).max() / max(np.abs(b).max(), 1e-30))


def test_dcn_zero_offset_kat(golden):
    """DCNv2/test.py:32-67: zero offset, mask = sigmoid(0), identity kernel -> 2*dcn(x) == x."""
    x = golden["ops"]["kat_input"].astype(np.float64)
    N, C, H, W = x.shape
    w = np.zeros((C, C, 3, 3))
    for p in range(C):
        w[p, p, 1, 1] = 1.0
    out = O.dcn_v2_forward(x, w, np.zeros(C), np.zeros((N, 18, H, W), np.float32),
                           np.full((N, 9, H, W), 0.5), 3, 3, 1, 1, 1, 1, 1, 1, 1)
    assert np.abs(x - 2 * out).max() < 1e-10


def test_dcn_sep_module(golden, sd):
    g = golden["ops"]
    out = O.dcn_sep(g["dcnsep_in"], g["dcnsep_fea"], sd, "pcd_align.L2_dcnpack_1")
    assert relmax(out, g["dcnsep_out"]) < 2e-5


def test_upsample(golden):
    g = golden["ops"]
    assert relmax(O.upsample2x(g["up2_in"].astype(np.float64)), g["up2_out"]) < 1e-6


def test_grid_sample_bilinear(golden):
    g = golden["ops"]
    img = g["gs_in"]
    grid = g["gs_grid"][0, 0]
    out = O.bilinear_sample(img, grid[None, :, 0], grid[None, :, 1])   # [1,Q,C]
    ref = g["gs_bilinear"][0, :, 0].T
    assert relmax(out[0], ref) < 1e-5


def test_siren(golden, sd):
    g = golden["ops"]
    assert relmax(O.siren(g["siren_in"].astype(np.float64), sd, "feat_imnet.", 3, np.float64), g["siren_out"]) < 1e-5


def test_convlstm_cell(golden, sd):
    g = golden["ops"]
    h, c = O.conv_lstm_cell(g["cell_x"], g["cell_h"], g["cell_c"], sd, "ConvBLSTM.forward_net.cell_list.0.", np.float64)
    assert relmax(h, g["cell_hn"]) < 1e-5
    assert relmax(c, g["cell_cn"]) < 1e-5


def test_make_coord_and_linspace(golden):
    g = golden["ops"]
    c = g["coord_40x50"].reshape(40, 50, 2)
    assert np.array_equal(O.make_coord_1d(40), c[:, 0, 0])
    assert np.array_equal(O.make_coord_1d(50), c[0, :, 1])
    # warpgrid base (flow = 0 part of warp_grid)
    fl = g["warp_flow"][0]
    grid = g["warp_grid"][0]
    gx = O.linspace_f32(16)[None, :] + fl[0] / ((16 - 1.0) / 2.0)
    gy = O.linspace_f32(12)[:, None] + fl[1] / ((12 - 1.0) / 2.0)
    assert np.abs(gx - grid[..., 0]).max() < 1e-6
    assert np.abs(gy - grid[..., 1]).max() < 1e-6


@pytest.fixture(scope="module")
def model_run(golden, sd):
    g = golden["model_16x20"]
    cap = {}
    outs = O.forward(g["x"], [float(t) for t in g["times"]], sd, capture=cap)
    return g, cap, outs


def test_model_intermediates(model_run):
    g, cap, _ = model_run
    assert relmax(cap["pcd_align"][0], g["pcd_align"]) < 1e-5
    assert relmax(cap["fusion"][0], g["fusion"]) < 1e-5
    assert relmax(cap["bilstm"][0], g["bilstm"]) < 1e-5
    assert relmax(cap["feat"][0], g["feat"]) < 1e-5
    assert relmax(cap["hrfeat"][2][0], g["hrfeat_t05"]) < 1e-5
    assert relmax(cap["flow"][2][0], g["flow_t05"]) < 1e-5


def test_model_outputs(model_run, sd):
    g, cap, outs = model_run
    for i in range(len(outs)):
        assert relmax(outs[i][0], g["out"][i]) < 1e-5
    o25 = O.decoding(cap["feat"], g["x"], [0.5], sd, scale=(40, 50))[0]
    assert relmax(o25[0], g["out_scale_40x50"]) < 1e-5


def test_window(golden, sd):
    g = golden["window_7x16x16"]
    fr = g["frames"]
    x = np.stack([fr[:-1], fr[1:]], axis=1)      # 6 pairs batched: pairs are independent
    outs = O.forward(x, [0.5], sd)[0]
    assert relmax(outs, g["out"]) < 1e-5


@pytest.mark.parametrize("which", ["test", "test_scale3", "fast", "fast_40x50", "ens", "ens_40x50"])
def test_oracle_decoder_variants_match_reference(sd, golden, which):
    """decoding_test / decoding_fasttest / decoding_localensemble restatements against the
    reference's own outputs (tests/golden/decoders_16x20.npz, same latent as model_16x20)."""
    g, d = golden["model_16x20"], golden["decoders_16x20"]
    feat, x = g["feat"][None], g["x"]
    if which == "test":
        got, ref = np.stack([o[0] for o in O.decoding_test(feat, x, list(d["test_times"]), sd)]), d["test_out"]
    elif which == "test_scale3":
        got, ref = O.decoding_test(feat, x, [0.5], sd, scale=3)[0][0], d["test_out_scale3"]
    elif which == "fast":
        got, ref = O.decoding_fasttest(feat, x, list(d["fast_times"]), sd), d["fast_out"]
    elif which == "fast_40x50":
        got, ref = O.decoding_fasttest(feat, x, [0.5], sd, (40, 50)), d["fast_out_40x50"]
    elif which == "ens":
        got, ref = O.decoding_localensemble(feat, x, [0.5], sd), d["ens_out"]
    else:
        got, ref = O.decoding_localensemble(feat, x, [0.25], sd, (40, 50)), d["ens_out_40x50"]
    assert np.abs(got - ref).max() <= 1e-5 * np.abs(ref).max()


def test_oracle_imresize_matches_reference():
    """data.util.imresize_np(uint8 BGR frame, 1/2, True) restatement vs the reference's outputs."""
    h = np.load(os.path.join(os.path.dirname(__file__), "golden", "harness.npz"))
    w, i0, s0, s1 = O.resize_weights_indices(37, 19, 0.5)
    assert np.array_equal(w, h["w_37_19"]) and np.array_equal(i0, h["i_37_19"][:, 0])
    assert (s0, s1) == tuple(h["sym_37_19"])
    for k in ("37x50", "64x90", "21x33"):
        assert np.abs(O.imresize_np(h["img_" + k], 0.5) - h["half_" + k]).max() < 1e-3


def _dcn_fd_case(seed, B=2, C=2, H=4, W=4, Co=2, dg=1, k=3, s=1, p=1, d=1):
    """DCNv2/test.py:69-103 check_gradient_dconv inputs: input U[0,1)*0.01, offset N(0,1)*2,
    mask sigmoid(U[0,1)), weight N(0,1), bias U[0,1)."""
    rng = np.random.default_rng(seed)
    Ho = (H + 2 * p - (d * (k - 1) + 1)) // s + 1
    Wo = (W + 2 * p - (d * (k - 1) + 1)) // s + 1
    x = rng.random((B, C, H, W)) * 0.01
    off = (rng.standard_normal((B, dg * 2 * k * k, Ho, Wo)) * 2).astype(np.float32)
    msk = 1 / (1 + np.exp(-rng.random((B, dg * k * k, Ho, Wo))))
    w = rng.standard_normal((Co, C, k, k))
    b = rng.random(Co)
    go = rng.standard_normal((B, Co, Ho, Wo))
    return x, w, b, off, msk, go, (k, k, s, s, p, p, d, d, dg)


@pytest.mark.parametrize("case", [dict(seed=3), dict(seed=4, dg=2, C=4, Co=3),
                                  dict(seed=5, H=6, W=5, s=2, d=2, p=2, C=2, Co=2)])
def test_dcn_backward_oracle_matches_finite_differences(case):
    """The backward restatement (dcn_v2_cuda_backward) against central differences of the forward
    restatement at the reference's own gradcheck configuration and tolerances (DCNv2/test.py:69-103:
    eps 1e-3, atol 1e-4, rtol 1e-2), over every input of dcn_v2_conv."""
    x, w, b, off, msk, go, dims = _dcn_fd_case(**case)
    gi, goff, gm, gw, gb = O.dcn_v2_backward(x, w, b, off, msk, go, *dims)
    f = lambda x_, w_, b_, o_, m_: float((O.dcn_v2_forward(x_, w_, b_, o_, m_, *dims) * go).sum())
    args = [x, w, b, off, msk]

    def fd(ai, eps):
        num = np.zeros(args[ai].shape)
        for idx in np.ndindex(args[ai].shape):
            ap, am = [a.copy() for a in args], [a.copy() for a in args]
            ap[ai][idx] += eps
            am[ai][idx] -= eps
            num[idx] = (f(*ap) - f(*am)) / (2 * eps)
        return num
    for ai, g in zip(range(5), (gi, gw, gb, goff, gm)):
        num = fd(ai, 1e-3)
        tol = dict(atol=1e-4 * max(1.0, np.abs(num).max()), rtol=1e-2)
        if ai == 3:
            # the output is piecewise bilinear in the offsets: a sample within eps of a cell edge or of
            # the (-1, H) gate has no derivative there; such elements are the ones whose difference
            # quotient changes with eps (at most a few of them)
            smooth = np.isclose(num, fd(ai, 2.5e-4), **tol)
            assert smooth.mean() > 0.98
            g, num = g[smooth], num[smooth]
        np.testing.assert_allclose(g, num, **tol)


@pytest.mark.parametrize("size", [None, (40, 50)], ids=["4x", "2.5x"])
def test_decoding_at_pixels_equals_full_decode(golden, sd, size):
    """decoding_at (the pixel-subset decoder the full-size GPU tests pin against) = the full oracle
    decode at every pixel it is asked for, incl. the 2.5x round-half-even tie rows/columns, the last
    row/column and samples whose warped grid is clamped at the frame edge; and the full decode is the
    reference's own output (fixture)."""
    g = golden["model_16x20"]
    feat, x = g["feat"].reshape(1, 3, 64, *g["feat"].shape[-2:]), g["x"]
    H, W = feat.shape[-2:]
    HH, WW = size or (4 * H, 4 * W)
    full = O.decoding(feat, x, [0.5, 0.25], sd, size)
    rng = np.random.default_rng(3)
    py = np.concatenate([rng.integers(0, HH, 300), np.full(20, HH - 1), np.arange(20) % HH, [0, HH - 1]])
    px = np.concatenate([rng.integers(0, WW, 300), rng.integers(0, WW, 20), np.full(20, WW - 1), [WW - 1, 0]])
    # a strided view, as the GPU engine's latent arrives ([3,B,H,W,64] NHWC permuted)
    fv = np.ascontiguousarray(feat.transpose(1, 0, 3, 4, 2)).transpose(1, 0, 4, 2, 3)
    st = {}
    sub = O.decoding_at(fv, x, [0.5, 0.25], sd, HH, WW, py, px, stats=st)
    for a, b in zip(sub, full):
        assert relmax(a, b[:, :, py, px]) < 1e-12
    assert st["clamped"] > 0
    if size is None:
        assert relmax(full[0][0], g["out"][2]) < 1e-5                    # t = 0.5
    else:
        assert relmax(full[0], g["out_scale_40x50"]) < 1e-5


def test_c1_pin_fixture_is_consistent():
    """c1_pair_pins.npz (make_golden.py c1: the reference's own 256x256 pair) keeps exactly the positions
    make_golden.c1_pins() names -- tile seams, frame edges, random pixels -- with finite values, and its
    input is bench.py's frames 0-1 (seeds 1234 / 1235)."""
    import importlib.util
    import torch
    here = os.path.dirname(os.path.abspath(__file__))
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(here, "golden", "make_golden.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    g = np.load(os.path.join(here, "golden", "c1_pair_pins.npz"))
    fy, fx, oy, ox = mg.c1_pins()
    for k, v in (("feat_y", fy), ("feat_x", fx), ("out_y", oy), ("out_x", ox)):
        assert np.array_equal(g[k], v), k
    assert g["feat"].shape == (3, 64, len(fy)) and g["out"].shape == (3, len(oy))
    assert np.isfinite(g["feat"]).all() and np.isfinite(g["out"]).all()
    for i in range(2):
        fr = torch.rand(3, 256, 256, generator=torch.Generator().manual_seed(1234 + i)).numpy()
        assert np.array_equal(g["x"][0, i], fr)


def test_chunked_dcn_shim_equals_unchunked_and_oracle():
    """the C2 / C3 / C4 latent fixtures come from make_golden's row-chunked CPU DCN shim.  Its
    equality with the unchunked shim (which the model fixtures use) was only printed by `make_golden.py
    chunk-check`; here it is asserted on that case (offsets up to 6 px, 150 rows in 32-row blocks incl. a
    partial one and both image edges), and both shims are checked against the oracle's restatement."""
    import importlib.util
    import torch
    here = os.path.dirname(os.path.abspath(__file__))
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(here, "golden", "make_golden.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    g = torch.Generator().manual_seed(5)
    B, C, H, W, dg = 1, 16, 150, 40, 2
    inp = torch.randn(B, C, H, W, generator=g)
    wt = torch.randn(8, C, 3, 3, generator=g)
    bs = torch.randn(8, generator=g)
    off = torch.rand(B, 2 * dg * 9, H, W, generator=g) * 12 - 6
    m = torch.rand(B, dg * 9, H, W, generator=g)
    a = mg.dcn_v2_forward_cpu(inp, wt, bs, off, m, 3, 3, 1, 1, 1, 1, 1, 1, dg)
    b = mg.dcn_v2_forward_cpu_chunked(inp, wt, bs, off, m, 3, 3, 1, 1, 1, 1, 1, 1, dg, rows=32)
    scale = float(a.abs().max())
    assert float((a - b).abs().max()) <= 1e-6 * scale
    ref = O.dcn_v2_forward(inp.numpy().astype(np.float64), wt.numpy().astype(np.float64), bs.numpy().astype(np.float64),
                           off.numpy(), m.numpy(), 3, 3, 1, 1, 1, 1, 1, 1, dg)
    assert np.abs(b.numpy() - ref).max() <= 1e-5 * scale


# ----------------------------------------------------------------------------- decoder stage 2 on its own
def _stage2_case(kind, HH=37, WW=45):
    import stage2_inputs as S
    feat, inp = S.latent(2, 16, 20)
    return feat, inp, S.hrfeat(2, HH, WW), S.flows(kind, 2, HH, WW), np.array([0.3, 0.7], np.float32)


def _replicate_sample(img, gx, gy, dtype=np.float64):
    """O.bilinear_sample with the out-of-range corners replicated from the border instead of zero."""
    B, C, H, W = img.shape
    ix = ((np.asarray(gx, dtype) + 1) * W - 1) / 2
    iy = ((np.asarray(gy, dtype) + 1) * H - 1) / 2
    x0, y0 = np.floor(ix), np.floor(iy)
    flat = np.asarray(img, dtype).reshape(B, C, H * W).transpose(0, 2, 1)
    b = np.arange(B)[:, None]
    out = 0
    for xx, yy, ww in ((x0, y0, (x0 + 1 - ix) * (y0 + 1 - iy)), (x0 + 1, y0, (ix - x0) * (y0 + 1 - iy)),
                       (x0, y0 + 1, (x0 + 1 - ix) * (iy - y0)), (x0 + 1, y0 + 1, (ix - x0) * (iy - y0))):
        idx = np.clip(yy.astype(np.int64), 0, H - 1) * W + np.clip(xx.astype(np.int64), 0, W - 1)
        out = out + flat[b, idx] * ww[..., None]
    return out


STAGE2_MUTANTS = ["divisor_n_over_2", "replicate_padding", "pixel_centre_base", "xy_swapped", "grids_swapped"]


@pytest.mark.parametrize("kind", ["uniform", "huge"])
def test_stage2_inputs_tell_a_wrong_stage2_from_a_right_one(sd, monkeypatch, kind):
    """The synthetic inputs of the GPU stage-2 tests discriminate: with several-pixel (uniform) or edge-clamped
    (huge) flows, each of five wrong restatements of stage 2 -- divisor n/2 for (n-1)/2, replicate for zero
    padding, a pixel-centre warp base for torch.linspace, flow x/y swapped, the two grids swapped -- breaks the
    project's oracle bound |d| <= 1e-4 |ref| + 1e-6 by at least 10x at a pixel 4 or more away from the border.
    (With the sub-pixel flows of make_state_dict's initialisation an interior pixel never sees the zero padding.)
    About the reference and the inputs only: nothing of the kernels is asked."""
    import stage2_inputs as S
    HH, WW = 37, 45
    feat, inp, hrf, flow, t = _stage2_case(kind, HH, WW)
    ref = O.decode_stage2(feat, inp, hrf, flow, t, sd, HH, WW)
    assert ref.shape == (2, 3, HH, WW) and np.isfinite(ref).all()
    worst = {}
    for name in STAGE2_MUTANTS:
        f = flow
        with monkeypatch.context() as mp:
            if name == "divisor_n_over_2":       # flow / (n / 2) = (flow (n - 1) / n) / ((n - 1) / 2)
                f = (flow.astype(np.float64) * np.array([(WW - 1) / WW, (HH - 1) / HH] * 2)).astype(np.float32)
            elif name == "replicate_padding":
                mp.setattr(O, "bilinear_sample", _replicate_sample)
            elif name == "pixel_centre_base":
                mp.setattr(O, "linspace_f32", O.make_coord_1d)
            elif name == "xy_swapped":
                f = np.ascontiguousarray(flow[..., [1, 0, 3, 2]])
            else:
                f = np.ascontiguousarray(flow[..., [2, 3, 0, 1]])
            mut = O.decode_stage2(feat, inp, hrf, f, t, sd, HH, WW)
        worst[name] = float(S.bound_ratio(mut, ref)[:, :, 4:HH - 4, 4:WW - 4].max())
    print(kind, {k: round(v, 1) for k, v in worst.items()})
    assert min(worst.values()) >= 10, worst
    assert np.array_equal(O.decode_stage2(feat, inp, hrf, flow, t, sd, HH, WW), ref)     # the patches are undone


@pytest.mark.parametrize("grid", [(37, 45), (64, 80)], ids=["37x45", "64x80"])
def test_stage2_edge_and_integer_flows_are_what_they_claim(grid):
    """In the kernel's fp32 arithmetic the `edge` flows put grids exactly on +-(1 - 1e-6), one ulp inside it and
    outside it (clamped), and the `integer` flows are whole pixels; `huge` clamps on both sides."""
    import stage2_inputs as S
    HH, WW = grid
    g = S.warped_grid_f32(S.flows("edge", 2, HH, WW), HH, WW)[0]
    for v in (S.HI, S.HI_IN, S.LO, S.LO_IN):
        assert (g == v).sum() > 50, (v, int((g == v).sum()))
    assert (g > S.HI).sum() > 50 and (g < S.LO).sum() > 50
    f = S.flows("integer", 2, HH, WW)
    assert np.array_equal(f, np.rint(f)) and np.abs(f).max() >= 3
    g = S.warped_grid_f32(S.flows("huge", 2, HH, WW), HH, WW)[0]
    assert (g > 1).mean() > 0.05 and (g < -1).mean() > 0.05
    assert np.array_equal(S.linspace_f32(WW), O.linspace_f32(WW)) and np.array_equal(S.linspace_f32(HH), O.linspace_f32(HH))


@pytest.mark.parametrize("kind", ["uniform", "huge", "integer", "edge"])
def test_stage2_oracle_in_fp32_is_within_the_bound(sd, kind):
    """The room the bound leaves: the same restatement run in fp32 stays inside |d| <= 1e-4 |ref| + 1e-6 of the
    fp64 run on every input kind (the grids differ by an fp32 rounding, the bilinear gathers are continuous)."""
    import stage2_inputs as S
    feat, inp, hrf, flow, t = _stage2_case(kind)
    ref = O.decode_stage2(feat, inp, hrf, flow, t, sd, 37, 45)
    r32 = O.decode_stage2(feat, inp, hrf, flow, t, sd, 37, 45, dtype=np.float32)
    ratio = float(S.bound_ratio(r32, ref).max())
    print(kind, "fp32 oracle / bound:", ratio)
    assert ratio <= 1.0


# ----------------------------------------------------------------------------- decoder stage 1 on its own
def _stage1_case(image):
    import stage2_inputs as S
    feat, inp = S.latent(2, 16, 20)
    img = O.upsample_bilinear(inp.reshape(2, 6, 16, 20), 4) if image else None      # decoding_test's HRinp
    return feat, inp, np.array([0.3, 0.7], np.float32), img


@pytest.mark.parametrize("image", [False, True], ids=["lr", "hrimg"])
@pytest.mark.parametrize("shift", [None, (-1, 1)], ids=["whole", "shift-1+1"])
def test_stage1_is_what_decode_records(sd, shift, image):
    """decode_stage1 is the hrfeat and the flow that _decode(..., capture=) records, bit for bit, and a time per
    item is the scalar-time decode of that item."""
    feat, inp, t, img = _stage1_case(image)
    HH, WW = 37, 45
    cap = {}
    O._decode(feat, inp, [0.3, 0.7], sd, HH, WW, np.float64, capture=cap, img=img, shift=shift)
    for k, tq in enumerate([0.3, 0.7]):
        hrf, flow = O.decode_stage1(feat, inp, np.full(2, tq), sd, HH, WW, img=img, shift=shift)
        assert hrf.shape == (2, HH, WW, 64) and flow.shape == (2, HH, WW, 4)
        assert np.array_equal(hrf.reshape(2, -1, 64), cap["hrfeat"][k])
        assert np.array_equal(flow.reshape(2, -1, 4), cap["flow"][k])
    hrf, flow = O.decode_stage1(feat, inp, t, sd, HH, WW, img=img, shift=shift)      # float32(0.3), float32(0.7)
    for b in range(2):
        one = O.decode_stage1(feat[b:b + 1], inp[b:b + 1], t[b:b + 1], sd, HH, WW, img=None if img is None else img[b:b + 1],
                              shift=shift)
        assert np.array_equal(hrf[b], one[0][0]) and np.array_equal(flow[b], one[1][0])


def _nearest_image_sample(img, gx, gy, dtype=np.float64):
    """O.bilinear_sample, but a 6-channel map (the frame pair) is read at its nearest pixel."""
    if img.shape[1] != 6:
        return _BILINEAR(img, gx, gy, dtype)
    B, C, H, W = img.shape
    idx = np.clip(O.nearest_index(gy, H), 0, H - 1) * W + np.clip(O.nearest_index(gx, W), 0, W - 1)
    return np.asarray(img, dtype).reshape(B, C, H * W).transpose(0, 2, 1)[np.arange(B)[:, None], idx]


_BILINEAR = O.bilinear_sample
_SIREN = O.siren
_AXES = O._query_axes


def _flow_time_swapped_siren(x, sd, p, n_sine, dtype):
    """O.siren, but flow_imnet reads the other item's time (its last input)."""
    if p == "flow_imnet.":
        x = x.copy()
        x[..., -1] = x[::-1, ..., -1]
    return _SIREN(x, sd, p, n_sine, dtype)


def _axes_mutant(name):
    def axes(H, W, HH, WW, shift=None):
        q, q0 = _AXES(H, W, HH, WW, shift), _AXES(H, W, HH, WW, None)
        if name == "remap_dropped":                       # the flow stage reads the pixel's own HRfeat
            q["hy"], q["hx"] = q0["hy"], q0["hx"]
        elif name == "nearest_unshifted":
            q["iy"], q["ix"] = q0["iy"], q0["ix"]
        elif name == "rel_shifted":
            q["rel_y"] = ((q["gy"] - O.make_coord_1d(H)[q["iy"]]) * np.float32(H)).astype(np.float32)
            q["rel_x"] = ((q["gx"] - O.make_coord_1d(W)[q["ix"]]) * np.float32(W)).astype(np.float32)
        elif name == "gathers_unshifted":
            q["gy"], q["gx"] = q0["gy"], q0["gx"]
        else:
            raise ValueError(name)
        return q
    return axes


STAGE1_MUTANTS = ["times_swapped", "flow_time_swapped", "rel_swapped", "replicate_padding", "nearest_image", "lr_for_hr"]
STAGE1_SHIFT_MUTANTS = ["remap_dropped", "nearest_unshifted", "rel_shifted", "gathers_unshifted"]
# what the attenuation is asserted for: wrong flows that leave HRfeat right, plus rel_swapped seen through its flow
STAGE1_FLOW_ONLY = ["flow_time_swapped", "replicate_padding", "nearest_image", "lr_for_hr", "remap_dropped",
                    "gathers_unshifted"]


def _stage1_mutant(name, mp, sd, feat, inp, t, HH, WW, img, shift):
    """(hrfeat, flow) of the wrong restatement ``name``, by patching the oracle's helpers inside ``mp`` or by
    permuting inputs / weight columns."""
    if name == "times_swapped":
        t = t[::-1]
    elif name == "flow_time_swapped":
        mp.setattr(O, "siren", _flow_time_swapped_siren)
    elif name == "rel_swapped":                           # columns 198 / 199 of feat_imnet's first layer: rel_y, rel_x
        k = "feat_imnet.net.0.linear.weight"
        w = np.array(sd[k])
        w[:, [198, 199]] = w[:, [199, 198]]
        sd = {**sd, k: w}
    elif name == "replicate_padding":
        mp.setattr(O, "bilinear_sample", _replicate_sample)
    elif name == "nearest_image":
        mp.setattr(O, "bilinear_sample", _nearest_image_sample)
    elif name == "lr_for_hr":
        img = None
    else:
        mp.setattr(O, "_query_axes", _axes_mutant(name))
    return O.decode_stage1(feat, inp, t, sd, HH, WW, img=img, shift=shift)


@pytest.mark.parametrize("grid", [(37, 45), (64, 80)], ids=["37x45", "64x80"])
@pytest.mark.parametrize("image,shift", [(False, None), (True, None), (False, (-1, 1)), (True, (1, -1))],
                         ids=["lr", "hrimg", "lr-shift-1+1", "hrimg-shift+1-1"])
def test_stage1_inputs_tell_a_wrong_stage1_from_a_right_one(sd, monkeypatch, grid, image, shift):
    """The inputs of the GPU stage-1 tests discriminate, and the RGB would not: each wrong restatement of stage 1 --
    the item times swapped (for both nets, for flow_imnet only), rel_y / rel_x swapped, replicate for zero padding
    (told at the border only: 4 pixels inside it nothing changes), the flow stage's image read at its nearest pixel,
    the LR image where the HR image was asked for; with a shift: the remap to HRfeat dropped, the nearest indices
    at the unshifted query, rel at the shifted query, the bilinear gathers at the unshifted query -- breaks the
    project's oracle bound |d| <= 1e-4 |ref| + 1e-6 on hrfeat or on flow by at least 10x.  Stage 2 run on the right
    hrfeat and a wrong flow brings the RGB at least 50x closer to the bound than that flow was (STAGE1_FLOW_ONLY,
    and rel_swapped seen through its flow).  About the reference and the inputs only: nothing of the kernels is asked."""
    import stage2_inputs as S
    HH, WW = grid
    feat, inp, t, img = _stage1_case(image)
    hrf, flow = O.decode_stage1(feat, inp, t, sd, HH, WW, img=img, shift=shift)
    assert np.isfinite(hrf).all() and np.isfinite(flow).all()
    rgb = O.decode_stage2(feat, inp, hrf, flow, t, sd, HH, WW, img=img)
    names = [n for n in STAGE1_MUTANTS if n != ("nearest_image" if image else "lr_for_hr")]
    names += STAGE1_SHIFT_MUTANTS if shift is not None else []
    worst, factor = {}, {}
    for name in names:
        with monkeypatch.context() as mp:
            mh, mf = _stage1_mutant(name, mp, sd, feat, inp, t, HH, WW, img, shift)
        rh, rf = S.bound_ratio(mh, hrf), S.bound_ratio(mf, flow)
        worst[name] = (float(rh.max()), float(rf.max()))
        if name in STAGE1_FLOW_ONLY:
            assert np.array_equal(mh, hrf), name
        if name == "replicate_padding" and shift is None:
            assert rh.max() == 0 and rf[:, 4:HH - 4, 4:WW - 4].max() == 0 and rf.max() > 0
        if name in STAGE1_FLOW_ONLY or name == "rel_swapped":
            rr = float(S.bound_ratio(O.decode_stage2(feat, inp, hrf, mf, t, sd, HH, WW, img=img), rgb).max())
            factor[name] = (float(rf.max()), rr)
    print(grid, "hrimg" if image else "lr", shift, "hrfeat / flow x bound:",
          {k: (round(a, 1), round(b, 1)) for k, (a, b) in worst.items()})
    print(grid, "hrimg" if image else "lr", shift, "flow x bound -> RGB x bound:",
          {k: (round(a, 1), round(b, 2)) for k, (a, b) in factor.items()})
    assert min(max(v) for v in worst.values()) >= 10, worst
    assert all(a >= 50 * b for a, b in factor.values()), factor
    again = O.decode_stage1(feat, inp, t, sd, HH, WW, img=img, shift=shift)              # the patches are undone
    assert np.array_equal(again[0], hrf) and np.array_equal(again[1], flow)


def test_stage1_oracle_in_fp32_is_within_the_bound(sd):
    """The room the bound leaves: decode_stage1 run in fp32 stays inside |d| <= 1e-4 |ref| + 1e-6 of the fp64 run,
    on both outputs, at every (grid, image, shift) the GPU tests use (stage1_cases.CASES)."""
    import stage1_cases as C
    import stage2_inputs as S
    worst = 0.0
    for case in C.CASES:
        (HH, WW), image, shift = case
        feat, inp, t, img = _stage1_case(image)
        ref = O.decode_stage1(feat, inp, t, sd, HH, WW, img=img, shift=shift)
        r32 = O.decode_stage1(feat, inp, t, sd, HH, WW, dtype=np.float32, img=img, shift=shift)
        assert r32[0].dtype == np.float32 and r32[1].dtype == np.float32
        ratios = [float(S.bound_ratio(a, b).max()) for a, b in zip(r32, ref)]
        print(C.case_id(case), "fp32 oracle / bound: hrfeat %.4f flow %.4f" % tuple(ratios))
        worst = max(worst, *ratios)
    assert worst <= 1.0
