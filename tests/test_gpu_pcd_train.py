"""The trainable PCD_Align on the GPU: stif_pack_conv_block_dev, stif_conv3x3_wgrad_cat, stif_upsample2x_bwd_nhwc, and
train.Upsample2x / Conv3x3Cat / DCN_sep / PCD_Align on top of them.

Reference everywhere: torch on the CPU in float64 -- F.conv2d / F.interpolate under autograd and the deformable conv of
tests/pcd_torch_ref.py, which tests/test_pcd_train_host.py pins to the numpy oracle.  RTOL = 1e-5 of max |ref| for
kernels and single modules (tests/test_gpu_conv_bwd.py), 2e-5 for the gradients of a DCN.
PCD_Align, a cascade of up to eleven layers through three deformable convs, is held to max(2e-5, 4 e32) of max |ref|
per tensor, e32 being the error of the same torch reference run in float32 on the CPU against its float64 run, computed
here: the reference's own rounding floor.  Every DCN input follows pcd_torch_ref's recipe (offsets 0.5 +- 0.3), asserted
on the float64 reference before anything is compared.

Weight-gradient shapes, from the kernel's tile of 2 x 32 pixels and its grid G = min(tiles, 2 per CU): 1x1x1, 2x5x7
(three tiles per item), 1x3x33 (a second tile on both axes, each one pixel wide or high), 3x33x70 (153 tiles), strided
items.  Every reduction runs with the shared workspace filled with NaN first; the 216 form also with NaN in the pad
channels 216..255 of gy, which it must never read."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pcd_torch_ref as R

pytestmark = pytest.mark.gpu

RTOL, RTOL_DCN, RTOL_PCD = 1e-5, 2e-5, 2e-5
WG_SHAPES = {"1x1x1": (1, 1, 1), "2x5x7": (2, 5, 7), "1x3x33": (1, 3, 33), "3x33x70": (3, 33, 70), "strided": (2, 5, 7)}
FORMS = {"cat": (2, 64, 64), "om": (1, 256, 216), "one": (1, 64, 64)}       # (nx, gy channels, cout)
MODES = ["f16x3", "f32"]


def relmax(got, ref):
    ref = torch.as_tensor(ref, dtype=torch.float64).detach()
    return float((got.detach().double().cpu() - ref).abs().max() / ref.abs().max())


def nchw64(t):
    return t.detach().double().cpu().permute(0, 3, 1, 2).contiguous()


def ints(gen, *shape):
    return torch.randint(-3, 4, shape, generator=gen).float()


def poison_workspace(ops):
    if not ops._WGRAD_WS:
        ops.conv3x3_wgrad(torch.zeros(1, 2, 2, 64, device="cuda"), torch.zeros(1, 2, 2, 64, device="cuda"))
    for ws in ops._WGRAD_WS.values():
        ws.fill_(float("nan"))


def pack_mode(stif, mfma):
    L = stif._lib
    return L.PACK_WINO | L.PACK_F16X3 if mfma == "f16x3" else L.PACK_WINO


# ---- the block packer ----

def host_pack(stif, w, b, mode):
    lay = stif.ops.pack_conv(w.numpy(), b.numpy(), mode, device="cuda", range_fallback=False)
    return lay.w, lay.b


def pack_weights(sd, kind, shape):
    if kind == "state-dict":
        name = "pcd_align.L2_offset_conv2_1" if shape[1] == 128 else "pcd_align.L1_dcnpack_2.conv_offset_mask"
        w, b = torch.from_numpy(sd[name + ".weight"]), torch.from_numpy(sd[name + ".bias"])
        assert tuple(w.shape) == shape
        return w, b
    g = torch.Generator().manual_seed(shape[0] + shape[1])
    return torch.randn(shape, generator=g), torch.randn(shape[0], generator=g)


def same_bytes(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("kind", ["random", "state-dict"])
@pytest.mark.parametrize("mfma", MODES)
@pytest.mark.parametrize("shape", [(64, 128, 3, 3), (216, 64, 3, 3)], ids=["64x128", "216x64"])
def test_block_packs_are_the_host_packers_bytes(stif, sd, shape, mfma, kind):
    ops, L, mode = stif.ops, stif._lib, pack_mode(stif, mfma)
    w, b = pack_weights(sd, kind, shape)
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    lay = ops.pack_conv_blocks_dev(w.cuda(), b.cuda(), mode, status=status)
    hw, hb = host_pack(stif, w, b, mode)
    assert lay.w.numel() == L.lib().stif_conv_weight_floats(shape[0], shape[1], 3, mode)
    assert same_bytes(lay.w, hw) and same_bytes(lay.b, hb)
    assert (lay.cout, lay.cin, lay.ks, lay.mode) == (256 if shape[0] == 216 else 64, shape[1], 3, mode)
    assert int(status.item()) == 0
    if shape[0] == 216:
        per = lay.w.numel() // 4
        last = lay.w[3 * per:].view(torch.int32)
        assert int((last != 0).sum()) > 0 and float(lay.b[216:].abs().max()) == 0.0     # 24 real rows, 40 zero rows
        padded = torch.zeros(256, 64, 3, 3)
        padded[:216] = w
        zb = torch.zeros(64)
        tail = stif.ops.pack_conv(padded[192:].numpy(), zb.numpy(), mode, device="cuda", range_fallback=False)
        assert same_bytes(lay.w[3 * per:], tail.w)


@pytest.mark.parametrize("mfma", MODES)
def test_dgrad_block_packs_are_the_packs_of_the_contiguous_slices(stif, sd, mfma):
    ops, mode = stif.ops, pack_mode(stif, mfma)
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    w, _ = pack_weights(sd, "state-dict", (216, 64, 3, 3))
    lay = ops.pack_conv_blocks_dev(w.cuda(), None, mode, dgrad=True, status=status)
    assert (lay.cout, lay.cin) == (64, 256) and lay.b.numel() == 64 and float(lay.b.abs().max()) == 0.0
    per = lay.w.numel() // 4
    padded = torch.zeros(256, 64, 3, 3)
    padded[:216] = w
    for s in range(4):
        one = ops.pack_conv_dev(padded[64 * s:64 * s + 64].contiguous().cuda(), None, mode, dgrad=True, status=status)
        assert same_bytes(lay.w[s * per:(s + 1) * per], one.w), s
    w, _ = pack_weights(sd, "random", (64, 128, 3, 3))
    for half in (0, 1):
        lay = ops.pack_conv_blocks_dev(w.cuda(), None, mode, dgrad=True, half=half, status=status)
        one = ops.pack_conv_dev(w[:, 64 * half:64 * half + 64].contiguous().cuda(), None, mode, dgrad=True,
                                status=status)
        assert (lay.cout, lay.cin) == (64, 64)
        assert same_bytes(lay.w, one.w) and same_bytes(lay.b, one.b), half
    assert int(status.item()) == 0
    with pytest.raises(ValueError, match="no block form"):
        ops.pack_conv_blocks_dev(w.cuda(), None, mode, dgrad=True)
    with pytest.raises(ValueError, match="no block form"):
        ops.pack_conv_blocks_dev(w.cuda(), None, mode, half=1)


def test_block_packer_reports_a_weight_outside_the_split_range(stif):
    ops, L = stif.ops, stif._lib
    w = torch.zeros(216, 64, 3, 3)
    w[200, 5, 0, 0] = 100.0                                   # U[0][0] = g[0][0]; in the last row slice only
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    ops.pack_conv_blocks_dev(w.cuda(), torch.zeros(216).cuda(), L.PACK_WINO | L.PACK_F16X3, status=status)
    assert int(status.item()) == L.STATUS_PACK_RANGE
    status.zero_()
    ops.pack_conv_blocks_dev(w.cuda(), torch.zeros(216).cuda(), L.PACK_WINO, status=status)       # fp32: no range
    w[200, 5, 0, 0] = 1.0
    ops.pack_conv_blocks_dev(w.cuda(), None, L.PACK_WINO | L.PACK_F16X3, dgrad=True, status=status)
    assert int(status.item()) == 0


# ---- the weight gradient in channel blocks ----

@functools.lru_cache(maxsize=None)
def wg_case(form, name):
    """(xs, gy) NHWC float32 on the GPU and the fp64 (gw, gb), computed once per case and never modified."""
    nx, gc, cout = FORMS[form]
    n, H, W = WG_SHAPES[name]
    g = torch.Generator().manual_seed(sorted(WG_SHAPES).index(name) * 3 + sorted(FORMS).index(form) + 300)
    if name == "strided":
        xs = [torch.randn(2 * n + i, H, W, 64, generator=g).cuda()[i::2][:n] for i in range(nx)]
        gy = torch.randn(2 * n + 1, H, W, gc, generator=g).cuda()[1::2]
        assert not xs[0].is_contiguous() and xs[0].stride(0) == 2 * H * W * 64 and gy.stride(0) == 2 * H * W * gc
    else:
        xs = [torch.randn(n, H, W, 64, generator=g).cuda() for _ in range(nx)]
        gy = torch.randn(n, H, W, gc, generator=g).cuda()
    gyr = nchw64(gy)[:, :cout].contiguous()
    gw = torch.nn.grad.conv2d_weight(torch.cat([nchw64(x) for x in xs], 1), (cout, 64 * nx, 3, 3), gyr, padding=1)
    if gc > cout:
        gy[..., cout:] = float("nan")
    return xs, gy, gw, gyr.sum((0, 2, 3))


@pytest.mark.parametrize("name", list(WG_SHAPES))
@pytest.mark.parametrize("form", list(FORMS))
def test_wgrad_cat_matches_fp64_and_the_64_to_64_kernel(stif, form, name):
    ops = stif.ops
    nx, gc, cout = FORMS[form]
    xs, gy, gw_ref, gb_ref = wg_case(form, name)
    poison_workspace(ops)
    gw, gb = ops.conv3x3_wgrad_cat(xs, gy, cout)
    assert tuple(gw.shape) == (cout, 64 * nx, 3, 3) and tuple(gb.shape) == (cout,)
    assert bool(torch.isfinite(gw).all()) and bool(torch.isfinite(gb).all())
    ew, eb = relmax(gw, gw_ref), relmax(gb, gb_ref)
    print(f"wgrad_cat {form} {name}: gw {ew:.3e} gb {eb:.3e} of max|ref|")
    assert ew <= RTOL and eb <= RTOL, (form, name, ew, eb)
    # block for block the bits of the 64 -> 64 kernel on the same two maps (the gy slice copied out contiguous)
    for s in range((cout + 63) // 64):
        rows = min(64, cout - 64 * s)
        gs = torch.zeros(gy.shape[:3] + (64,), device="cuda")
        gs[..., :rows] = gy[..., 64 * s:64 * s + rows]
        for i, x in enumerate(xs):
            bw, bb = ops.conv3x3_wgrad(x, gs)
            assert torch.equal(gw[64 * s:64 * s + rows, 64 * i:64 * i + 64], bw[:rows]), (form, name, s, i)
            assert torch.equal(gb[64 * s:64 * s + rows], bb[:rows]), (form, name, s, i)


@pytest.mark.parametrize("form", list(FORMS))
def test_wgrad_cat_integer_inputs_give_the_fp64_bits(stif, form):
    nx, gc, cout = FORMS[form]
    gen = torch.Generator().manual_seed(78)
    n, H, W = 2, 33, 70
    xs, gy = [ints(gen, n, H, W, 64) for _ in range(nx)], ints(gen, n, H, W, gc)
    gw, gb = stif.ops.conv3x3_wgrad_cat([x.cuda() for x in xs], gy.cuda(), cout)
    gyr = nchw64(gy)[:, :cout].contiguous()
    ref = torch.nn.grad.conv2d_weight(torch.cat([nchw64(x) for x in xs], 1), (cout, 64 * nx, 3, 3), gyr, padding=1)
    assert float(ref.abs().max()) < 2 ** 24
    assert torch.equal(gw.double().cpu(), ref)
    assert torch.equal(gb.double().cpu(), gyr.sum((0, 2, 3)))


@pytest.mark.parametrize("form", ["cat", "om"])
def test_wgrad_cat_repeats_are_bit_identical(stif, form):
    ops = stif.ops
    cout = FORMS[form][2]
    xs, gy, _, _ = wg_case(form, "3x33x70")
    first = ops.conv3x3_wgrad_cat(xs, gy, cout)
    other = wg_case("cat" if form == "om" else "om", "2x5x7")
    ops.conv3x3_wgrad_cat(other[0], other[1], FORMS["cat" if form == "om" else "om"][2])      # another shape in between
    poison_workspace(ops)
    again = ops.conv3x3_wgrad_cat(xs, gy, cout)
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])


# ---- the upsample's adjoint ----

UP_SHAPES = [(1, 1), (5, 1), (1, 7), (3, 5), (16, 20)]


@pytest.mark.parametrize("scale", [1.0, 2.0])
@pytest.mark.parametrize("c", [4, 64, 256])
@pytest.mark.parametrize("hw", UP_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_upsample_backward_is_the_exact_transpose(stif, hw, c, scale):
    """Integer gy: every weight is k / 16, so the sums are exact and equality with the fp64 autograd is bit for bit."""
    ops = stif.ops
    h, w = hw
    gen = torch.Generator().manual_seed(h * 100 + w + c)
    n = 2
    gy = ints(gen, n, 2 * h, 2 * w, c)
    x = torch.zeros(n, c, h, w, dtype=torch.float64, requires_grad=True)
    (R.up2(x) * scale).backward(gy.double().permute(0, 3, 1, 2))
    want = x.grad.permute(0, 2, 3, 1)
    got = ops.upsample2x_bwd(gy.cuda(), scale)
    assert tuple(got.shape) == (n, h, w, c)
    assert torch.equal(got.double().cpu(), want), (hw, c, scale)
    # strided items
    wide = torch.full((2 * n + 1, 2 * h, 2 * w, c), float("nan"))
    wide[1::2] = gy
    view = wide.cuda()[1::2]
    assert n == 1 or not view.is_contiguous()
    assert torch.equal(ops.upsample2x_bwd(view, scale), got)
    # <up(x), g> = <x, up_bwd(g)> with the forward kernel
    xr = torch.randn(n, h, w, c, generator=gen).cuda()
    gr = torch.randn(n, 2 * h, 2 * w, c, generator=gen).cuda()
    up = torch.empty(n, 2 * h, 2 * w, c, device="cuda")
    ops.upsample2x(xr, up, scale)
    lhs = float((up.double() * gr.double()).sum())
    rhs = float((xr.double() * ops.upsample2x_bwd(gr, scale).double()).sum())
    norm = float((up.double() * gr.double()).abs().sum())
    assert abs(lhs - rhs) <= 1e-6 * norm, (lhs, rhs, norm)


# ---- the modules ----

MOD_SHAPES = [(1, 5, 7), (2, 12, 20)]
shape_id = lambda s: "x".join(map(str, s))


def leaf(t):
    return t.detach().clone().requires_grad_(True)


def gpu_leaf(t):
    return t.detach().float().cuda().requires_grad_(True)


def check(name, got, ref, tol):
    e = relmax(got, ref)
    print(f"  {name}: {e:.3e} of max|ref| (tol {tol:.1e})")
    assert e <= tol, (name, e, tol)


@pytest.mark.parametrize("scale", [1.0, 2.0])
@pytest.mark.parametrize("shape", MOD_SHAPES, ids=shape_id)
def test_upsample_module(stif, shape, scale):
    n, h, w = shape
    g = torch.Generator().manual_seed(h + w)
    x, gout = torch.randn(n, 64, h, w, generator=g).double(), torch.randn(n, 64, 2 * h, 2 * w, generator=g).double()
    xr = leaf(x)
    ref = R.up2(xr) * scale
    ref.backward(gout)
    xg = gpu_leaf(x)
    out = stif.train.Upsample2x(scale)(xg)
    out.backward(gout.float().cuda())
    assert tuple(out.shape) == (n, 64, 2 * h, 2 * w)
    check("out", out, ref, RTOL)
    check("gx", xg.grad, xr.grad, RTOL)


@pytest.mark.parametrize("mfma", MODES)
@pytest.mark.parametrize("act", [None, "relu", "lrelu"])
@pytest.mark.parametrize("shape", MOD_SHAPES, ids=shape_id)
def test_conv3x3cat_module(stif, shape, act, mfma):
    n, h, w = shape
    g = torch.Generator().manual_seed(h * w + len(act or ""))
    rnd = lambda *s: torch.randn(*s, generator=g).double()
    a, b, gout = rnd(n, 64, h, w), rnd(n, 64, h, w), rnd(n, 64, h, w)
    torch.manual_seed(1)
    m = stif.train.Conv3x3Cat(act, mfma)
    with torch.no_grad():
        m.bias.copy_(rnd(64) * 0.1)
    fn = {None: lambda t: t, "relu": F.relu, "lrelu": R.lrelu}[act]
    ar, br, wr, biasr = leaf(a), leaf(b), leaf(m.weight.double()), leaf(m.bias.double())
    ref = fn(F.conv2d(torch.cat([ar, br], 1), wr, biasr, padding=1))
    ref.backward(gout)
    m = m.cuda()
    ag, bg = gpu_leaf(a), gpu_leaf(b)
    out = m(ag, bg)
    out.backward(gout.float().cuda())
    check("out", out, ref, RTOL)
    for name, got, want in (("ga", ag.grad, ar.grad), ("gb", bg.grad, br.grad), ("gw", m.weight.grad, wr.grad),
                            ("gbias", m.bias.grad, biasr.grad)):
        check(name, got, want, RTOL)
    assert m.range_status() == 0
    # only the gradients that are asked for are computed
    ag2 = gpu_leaf(a)
    m.zero_grad()
    m.weight.requires_grad_(False)
    m(ag2, b.float().cuda()).backward(gout.float().cuda())
    assert m.weight.grad is None and torch.equal(ag2.grad, ag.grad)


def dcn_module_case(shape, seed):
    n, h, w = shape
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g).double()
    inp, fea, gout = rnd(n, 64, h, w), rnd(n, 64, h, w), rnd(n, 64, h, w)
    P = {"weight": rnd(64, 64, 3, 3) / 24, "bias": rnd(64) * 0.1,
         "conv_offset_mask.weight": rnd(216, 64, 3, 3) / 24, "conv_offset_mask.bias": rnd(216) * 0.1}
    R.tame_dcn(P["conv_offset_mask.weight"], P["conv_offset_mask.bias"], fea)
    return inp, fea, gout, P


@pytest.mark.parametrize("mfma", MODES)
@pytest.mark.parametrize("act", [None, "lrelu"])
@pytest.mark.parametrize("shape", MOD_SHAPES, ids=shape_id)
def test_dcn_sep_module(stif, shape, act, mfma):
    inp, fea, gout, P = dcn_module_case(shape, sum(shape))
    Pr = {k: leaf(v) for k, v in P.items()}
    ir, fr = leaf(inp), leaf(fea)
    offset, mask = R.offset_mask(fr, Pr["conv_offset_mask.weight"], Pr["conv_offset_mask.bias"])
    R.assert_offsets_tame(offset)
    ref = R.dcn(ir, offset, mask, Pr["weight"], Pr["bias"])
    if act:
        ref = R.lrelu(ref)
    ref.backward(gout)
    m = stif.train.DCN_sep(act, mfma)
    m.load_state_dict({k: v.float() for k, v in P.items()}, strict=True)
    m = m.cuda()
    ig, fg = gpu_leaf(inp), gpu_leaf(fea)
    out = m(ig, fg)
    out.backward(gout.float().cuda())
    assert tuple(out.shape) == tuple(ref.shape)
    check("out", out, ref, RTOL)
    got = dict(m.named_parameters())
    check("g_input", ig.grad, ir.grad, RTOL_DCN)
    check("g_fea", fg.grad, fr.grad, RTOL_DCN)
    for k in P:
        check("g_" + k, got[k].grad, Pr[k].grad, RTOL_DCN)
    assert m.range_status() == 0


@functools.lru_cache(maxsize=None)
def pcd_case(shape):
    """Inputs, tamed float64 parameters, the float64 output and gradients, and e32 per quantity: computed once."""
    B, H, W = shape
    fea1, fea2 = R.pyramid_inputs(B * H + W, B, H, W)
    P = R.random_pcd_params(B + H)
    R.tame_offsets(P, fea1, fea2)
    R.assert_pcd_offsets_tame(P, fea1, fea2)
    gout = torch.randn(B, 128, H, W, generator=torch.Generator().manual_seed(9)).double()
    res = {}
    for dt in (torch.float64, torch.float32):
        Pl = {k: leaf(v.to(dt)) for k, v in P.items()}
        f1, f2 = [leaf(t.to(dt)) for t in fea1], [leaf(t.to(dt)) for t in fea2]
        out = R.pcd_align(Pl, f1, f2)
        out.backward(gout.to(dt))
        q = {"out": out.detach()}
        q.update({"g_" + k: v.grad for k, v in Pl.items()})
        q.update({f"g_fea{i + 1}_L{l + 1}": t.grad for i, f in enumerate((f1, f2)) for l, t in enumerate(f)})
        res[dt] = q
    ref = res[torch.float64]
    e32 = {k: relmax(res[torch.float32][k], ref[k]) for k in ref}
    return fea1, fea2, P, gout, ref, e32


@pytest.mark.parametrize("mfma", MODES)
@pytest.mark.parametrize("shape", [(1, 8, 12), (2, 12, 20)], ids=shape_id)
def test_pcd_align_output_and_every_gradient(stif, shape, mfma):
    fea1, fea2, P, gout, ref, e32 = pcd_case(shape)
    net = stif.train.PCD_Align(mfma)
    net.load_state_dict({k: v.float() for k, v in P.items()}, strict=True)
    net = net.cuda()
    f1, f2 = [gpu_leaf(t) for t in fea1], [gpu_leaf(t) for t in fea2]
    out = net(f1, f2)
    assert tuple(out.shape) == (shape[0], 128, shape[1], shape[2])
    out.backward(gout.float().cuda())
    got = {"out": out}
    got.update({"g_" + k: p.grad for k, p in net.named_parameters()})
    got.update({f"g_fea{i + 1}_L{l + 1}": t.grad for i, f in enumerate((f1, f2)) for l, t in enumerate(f)})
    assert sorted(got) == sorted(ref) and len(ref) == 1 + 64 + 6
    ratios, worst = {}, None
    for k in ref:
        assert got[k] is not None, k
        tol = max(RTOL_PCD, 4 * e32[k])
        e = relmax(got[k], ref[k])
        ratios[k] = (e / tol, e, e32[k])
    for kind in ("out", "g_fea", "conv_offset_mask.weight", "conv_offset_mask.bias", "dcnpack", "offset_conv",
                 "fea_conv"):
        ks = [k for k in ratios if kind in k]
        k = max(ks, key=lambda q: ratios[q][0])
        print(f"  pcd {shape_id(shape)} {mfma} worst {kind}: {k} err {ratios[k][1]:.3e} e32 {ratios[k][2]:.3e} "
              f"ratio {ratios[k][0]:.3f}")
    bad = {k: v for k, v in ratios.items() if v[0] > 1.0}
    assert not bad, bad
    assert net.range_status() == 0


def test_one_optimiser_step_through_frame_features_and_pcd_align(stif):
    T = stif.train

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.enc = T.FrameFeatures(front_RBs=1)
            self.pcd_align = T.PCD_Align()

        def forward(self, a, b):
            return self.pcd_align(list(self.enc(a)), list(self.enc(b)))

    torch.manual_seed(3)
    net = Net().cuda()
    with torch.no_grad():        # the zero-initialised offset convs would leave their inputs without a gradient
        for m in net.modules():
            if isinstance(m, T.DCN_sep):
                m.conv_offset_mask.weight.normal_(0, 0.01)
    g = torch.Generator().manual_seed(4)
    a, b = torch.rand(2, 3, 16, 24, generator=g).cuda(), torch.rand(2, 3, 16, 24, generator=g).cuda()
    gt = torch.rand(2, 128, 16, 24, generator=g).cuda()
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    crit = T.CharbonnierLoss()
    first = T.optimize_step(net, opt, crit, (a, b), gt)
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in net.parameters())
    assert float(net.pcd_align.L3_offset_conv1_1.weight.grad.abs().max()) > 0
    assert float(net.enc.conv_first.weight.grad.abs().max()) > 0
    with torch.no_grad():
        second = float(crit(net(a, b), gt))
    print(f"  loss {first:.4f} -> {second:.4f}")
    assert second < first
    assert net.pcd_align.range_status() == 0
