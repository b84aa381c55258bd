"""The trainable frame encoder on the GPU: stif_conv3x3s2_wgrad, stif_conv3x3s2_dgrad, stif_conv_first_wgrad,
stif_pack_conv_plain_dev, and train.ConvDown / ConvFirst / FrameFeatures on top of them.

Reference everywhere: torch on the CPU in float64 (F.conv2d under autograd, torch.nn.grad.conv2d_weight /
conv2d_input with stride=2, padding=1).  RTOL = 1e-5 of max |ref| for kernels and single modules
(tests/test_gpu_conv_bwd.py), 2e-5 of max |ref| per parameter gradient of the multi-layer module
(tests/test_gpu_train.py).

Stride-2 weight-gradient shapes (the size of x), from the kernel's tile of TH = 2 x TW = 16 output pixels and its grid
G = min(tiles, 2 per CU): 1x1x1 (centre tap only), 2x5x7 and 2x6x8 (the same 3 x 4 output, another last row / column),
one output pixel more than a tile on both axes, 3x33x70, strided items, and 2x192x192 = 1152 tiles, more than the
512 workgroups of a 256-CU device.  The data gradient's tile is DTH = 4 x DTW = 32 gy pixels: 33x70 and 64x96 cross
it on both axes.  Every reduction runs with the shared cached workspace filled with NaN first."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

from oracle import stif_oracle as O

pytestmark = pytest.mark.gpu

RTOL = 1e-5
TH, TW = 2, 16
S2_SHAPES = {"1x1x1": (1, 1, 1), "2x5x7": (2, 5, 7), "2x6x8": (2, 6, 8), "tile+1": (1, 2 * (TH + 1) - 1, 2 * (TW + 1)),
             "3x33x70": (3, 33, 70), "strided": (2, 5, 7), "many-tiles": (2, 192, 192)}
CF_SHAPES = {"1x1x1": (1, 1, 1), "2x5x7": (2, 5, 7), "3x33x70": (3, 33, 70), "2x192x192": (2, 192, 192)}
DG_SHAPES = {"1x1x1": (1, 1, 1), "2x5x7": (2, 5, 7), "2x6x8": (2, 6, 8), "3x33x70": (3, 33, 70), "2x64x96": (2, 64, 96),
             "strided": (2, 6, 7)}


def relmax(got, ref):
    ref = torch.as_tensor(ref, dtype=torch.float64).detach()
    return float((got.detach().double().cpu() - ref).abs().max() / ref.abs().max())


def nchw64(t):
    return t.detach().double().cpu().permute(0, 3, 1, 2).contiguous()


def out_size(v):
    return (v + 1) // 2


def ints(gen, *shape):
    return torch.randint(-3, 4, shape, generator=gen).float()


def poison_workspace(ops):
    if not ops._WGRAD_WS:
        ops.conv3x3_wgrad(torch.zeros(1, 2, 2, 64, device="cuda"), torch.zeros(1, 2, 2, 64, device="cuda"))
    for ws in ops._WGRAD_WS.values():
        ws.fill_(float("nan"))


# ---- stride-2 weight gradient ----

@functools.lru_cache(maxsize=None)
def s2_case(name):
    """(x, gy) NHWC float32 on the GPU and the fp64 (gw, gb), computed once per shape and never modified."""
    n, H, W = S2_SHAPES[name]
    Ho, Wo = out_size(H), out_size(W)
    g = torch.Generator().manual_seed(sorted(S2_SHAPES).index(name) + 200)
    if name == "strided":
        x = torch.randn(2 * n, H, W, 64, generator=g).cuda()[0::2]
        gy = torch.randn(2 * n + 1, Ho, Wo, 64, generator=g).cuda()[1::2]
        assert not x.is_contiguous() and x.stride(0) == 2 * H * W * 64
    else:
        x = torch.randn(n, H, W, 64, generator=g).cuda()
        gy = torch.randn(n, Ho, Wo, 64, generator=g).cuda()
    gw = torch.nn.grad.conv2d_weight(nchw64(x), (64, 64, 3, 3), nchw64(gy), stride=2, padding=1)
    return x, gy, gw, nchw64(gy).sum((0, 2, 3))


@pytest.mark.parametrize("name", list(S2_SHAPES))
def test_stride2_weight_gradient_matches_fp64(stif, name):
    ops = stif.ops
    x, gy, gw_ref, gb_ref = s2_case(name)
    poison_workspace(ops)
    gw, gb = ops.conv3x3s2_wgrad(x, gy)
    assert tuple(gw.shape) == (64, 64, 3, 3) and tuple(gb.shape) == (64,)
    ew, eb = relmax(gw, gw_ref), relmax(gb, gb_ref)
    print(f"wgrad s2 {name}: gw {ew:.3e} gb {eb:.3e} of max|ref|")
    assert ew < RTOL and eb < RTOL, (name, ew, eb)
    if name == "1x1x1":
        off_centre = gw.clone()
        off_centre[:, :, 1, 1] = 0
        assert float(off_centre.abs().max()) == 0.0            # every other tap reads padding only


def test_many_tiles_shape_has_more_tiles_than_workgroups(stif):
    n, H, W = S2_SHAPES["many-tiles"]
    part = (64 * 64 * 9 + 64) * 4
    G = stif._lib.lib().stif_conv3x3s2_wgrad_workspace_size(n, H, W, 64, 64) // part
    tiles = n * -(-out_size(H) // TH) * -(-out_size(W) // TW)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert G == min(tiles, 2 * cus) and G < tiles, (G, tiles, cus)


@pytest.mark.parametrize("hw", [(5, 35), (6, 36)])
def test_stride2_taps_against_padding(stif, hw):
    """x all ones, gy a single one at a corner output pixel: gw is exactly the 0 / 1 pattern of the taps inside x."""
    H, W = hw
    Ho, Wo, co = out_size(H), out_size(W), 37
    x = torch.ones(1, H, W, 64, device="cuda")
    for oy, ox in ((0, 0), (0, Wo - 1), (Ho - 1, 0), (Ho - 1, Wo - 1)):
        gy = torch.zeros(1, Ho, Wo, 64, device="cuda")
        gy[0, oy, ox, co] = 1.0
        gw, gb = stif.ops.conv3x3s2_wgrad(x, gy)
        want = torch.zeros(64, 64, 3, 3)
        for kh in range(3):
            for kw in range(3):
                if 0 <= 2 * oy + kh - 1 < H and 0 <= 2 * ox + kw - 1 < W:
                    want[co, :, kh, kw] = 1.0
        assert 4 <= int(want[co, 0].sum()) <= 9
        assert torch.equal(gw.cpu(), want), (hw, oy, ox, gw[co, 0].cpu(), want[co, 0])
        assert torch.equal(gb.cpu(), torch.eye(64)[co])


# ---- exactness with small integers: every product and sum is an integer below 2^24 ----

def test_integer_inputs_give_the_fp64_bits(stif):
    ops = stif.ops
    gen = torch.Generator().manual_seed(77)
    n, H, W = 2, 33, 70
    x, gy = ints(gen, n, H, W, 64), ints(gen, n, out_size(H), out_size(W), 64)
    gw, gb = ops.conv3x3s2_wgrad(x.cuda(), gy.cuda())
    ref = torch.nn.grad.conv2d_weight(nchw64(x), (64, 64, 3, 3), nchw64(gy), stride=2, padding=1)
    assert float(ref.abs().max()) < 2 ** 24
    assert torch.equal(gw.double().cpu(), ref)
    assert torch.equal(gb.double().cpu(), nchw64(gy).sum((0, 2, 3)))
    w = ints(gen, 64, 64, 3, 3)
    for H, W in ((5, 7), (6, 8), (33, 70), (34, 69)):
        gy = ints(gen, n, out_size(H), out_size(W), 64)
        gx = ops.conv3x3s2_dgrad(gy.cuda(), w.cuda(), H, W)
        ref = torch.nn.grad.conv2d_input((n, 64, H, W), w.double(), nchw64(gy), stride=2, padding=1)
        assert torch.equal(nchw64(gx), ref), (H, W, float((nchw64(gx) - ref).abs().max()))
    frames, gy = ints(gen, n, 3, 33, 70), ints(gen, n, 33, 70, 64)
    gw, gb = ops.conv_first_wgrad(frames.cuda(), gy.cuda())
    ref = torch.nn.grad.conv2d_weight(frames.double(), (64, 3, 3, 3), nchw64(gy), padding=1)
    assert torch.equal(gw.double().cpu(), ref)
    assert torch.equal(gb.double().cpu(), nchw64(gy).sum((0, 2, 3)))


# ---- stride-2 data gradient ----

def dgrad_into(stif, gy, w, gx):
    """stif_conv3x3s2_dgrad into a caller's gx (ops.conv3x3s2_dgrad allocates its own)."""
    n, H, W, _ = gx.shape
    L = stif._lib
    L.check(L.lib().stif_conv3x3s2_dgrad(gy.data_ptr(), w.data_ptr(), gx.data_ptr(), gy.stride(0), gx.stride(0), n, H,
                                         W, None, 0, torch.cuda.current_stream().cuda_stream), "stif_conv3x3s2_dgrad")


@pytest.mark.parametrize("name", list(DG_SHAPES))
def test_stride2_data_gradient_matches_fp64(stif, name):
    n, H, W = DG_SHAPES[name]
    Ho, Wo = out_size(H), out_size(W)
    gen = torch.Generator().manual_seed(sorted(DG_SHAPES).index(name) + 300)
    w = torch.randn(64, 64, 3, 3, generator=gen) * 0.05
    if name == "strided":
        gy = torch.randn(2 * n + 1, Ho, Wo, 64, generator=gen).cuda()[1::2]
        assert gy.stride(0) == 2 * Ho * Wo * 64
    else:
        gy = torch.randn(n, Ho, Wo, 64, generator=gen).cuda()
    assert stif._lib.lib().stif_conv3x3s2_dgrad_workspace_size(n, H, W) == 0
    gx = torch.full((n, H, W, 64), float("nan"), device="cuda")
    dgrad_into(stif, gy, w.cuda(), gx)
    assert bool(torch.isfinite(gx).all())                       # every element was overwritten
    ref = torch.nn.grad.conv2d_input((n, 64, H, W), w.double(), nchw64(gy), stride=2, padding=1)
    err = relmax(gx.permute(0, 3, 1, 2), ref)
    print(f"dgrad s2 {name}: {err:.3e} of max|ref|")
    assert err < RTOL, (name, err)
    assert torch.equal(stif.ops.conv3x3s2_dgrad(gy, w.cuda(), H, W), gx)


@pytest.mark.parametrize("hw", [(6, 8), (5, 7)])
def test_stride2_data_gradient_of_the_last_output_pixel(stif, hw):
    """gy one-hot at the last output pixel, for H = 2 Ho and H = 2 Ho - 1: gx is the weight's taps that land inside
    the map, everything else exactly zero."""
    H, W = hw
    Ho, Wo, co = out_size(H), out_size(W), 21
    w = torch.randn(64, 64, 3, 3, generator=torch.Generator().manual_seed(5))
    gy = torch.zeros(1, Ho, Wo, 64)
    gy[0, Ho - 1, Wo - 1, co] = 1.0
    gx = stif.ops.conv3x3s2_dgrad(gy.cuda(), w.cuda(), H, W).cpu()
    want = torch.zeros(1, H, W, 64)
    seen = 0
    for kh in range(3):
        for kw in range(3):
            y, x = 2 * (Ho - 1) + kh - 1, 2 * (Wo - 1) + kw - 1
            if y < H and x < W:
                want[0, y, x] = w[co, :, kh, kw]
                seen += 1
    assert seen == (9 if H % 2 == 0 else 4)
    assert torch.equal(gx, want)


# ---- conv_first weight gradient ----

@functools.lru_cache(maxsize=None)
def cf_case(name):
    n, h, w = CF_SHAPES[name]
    g = torch.Generator().manual_seed(sorted(CF_SHAPES).index(name) + 400)
    frames = torch.rand(n, 3, h, w, generator=g)
    gy = torch.randn(n, h, w, 64, generator=g)
    gw = torch.nn.grad.conv2d_weight(frames.double(), (64, 3, 3, 3), nchw64(gy), padding=1)
    return frames.cuda(), gy.cuda(), gw, nchw64(gy).sum((0, 2, 3))


@pytest.mark.parametrize("name", list(CF_SHAPES))
def test_conv_first_weight_gradient_matches_fp64(stif, name):
    ops = stif.ops
    frames, gy, gw_ref, gb_ref = cf_case(name)
    poison_workspace(ops)
    gw, gb = ops.conv_first_wgrad(frames, gy)
    assert tuple(gw.shape) == (64, 3, 3, 3) and tuple(gb.shape) == (64,)
    ew, eb = relmax(gw, gw_ref), relmax(gb, gb_ref)
    print(f"conv_first wgrad {name}: gw {ew:.3e} gb {eb:.3e} of max|ref|")
    assert ew < RTOL and eb < RTOL, (name, ew, eb)


def test_conv_first_weight_gradient_takes_strided_items(stif):
    frames, gy, gw_ref, gb_ref = cf_case("2x5x7")
    wide = torch.zeros(5, 5, 7, 64, device="cuda")
    wide[1::2] = gy
    gw, gb = stif.ops.conv_first_wgrad(frames, wide[1::2])
    assert relmax(gw, gw_ref) < RTOL and relmax(gb, gb_ref) < RTOL


def test_the_three_reductions_are_deterministic(stif):
    ops = stif.ops
    x, gy, _, _ = s2_case("many-tiles")
    a = ops.conv3x3s2_wgrad(x, gy)
    ops.conv3x3s2_wgrad(*s2_case("2x5x7")[:2])                   # another shape in between, same workspace
    b = ops.conv3x3s2_wgrad(x, gy)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    frames, g1, _, _ = cf_case("2x192x192")
    a = ops.conv_first_wgrad(frames, g1)
    ops.conv_first_wgrad(*cf_case("2x5x7")[:2])
    b = ops.conv_first_wgrad(frames, g1)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    x1 = torch.randn(2, 192, 192, 64, generator=torch.Generator().manual_seed(9)).cuda()
    a = ops.conv3x3_wgrad(x1, x)                                 # stride 1 shares the workspace with the new two
    ops.conv3x3s2_wgrad(x, gy)
    b = ops.conv3x3_wgrad(x1, x)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    w = torch.randn(64, 64, 3, 3, generator=torch.Generator().manual_seed(10)).cuda()
    a = ops.conv3x3s2_dgrad(gy, w, 192, 192)                     # no reduction, no atomics: trivially repeatable
    ops.conv3x3s2_dgrad(s2_case("2x5x7")[1], w, 5, 7)
    assert torch.equal(a, ops.conv3x3s2_dgrad(gy, w, 192, 192))


# ---- PLAIN device packer ----

@pytest.mark.parametrize("which", ["random", "fea_L2_conv1"])
def test_plain_device_packer_writes_the_host_packers_bytes(stif, sd, which):
    L, ops = stif._lib, stif.ops
    if which == "random":
        rng = np.random.default_rng(8)
        w = (rng.standard_normal((64, 64, 3, 3)) * 0.05).astype(np.float32)
        b = rng.standard_normal(64).astype(np.float32)
    else:
        w, b = np.asarray(sd["fea_L2_conv1.weight"]), np.asarray(sd["fea_L2_conv1.bias"])
    host = ops.pack_conv(w, b, L.PACK_PLAIN)
    dev = ops.pack_conv_plain_dev(torch.from_numpy(w).cuda(), torch.from_numpy(b).cuda())
    assert dev.mode == L.PACK_PLAIN and (dev.cout, dev.cin, dev.ks) == (64, 64, 3)
    for a, h in ((dev.w, host.w), (dev.b, host.b)):
        assert a.shape == h.shape and torch.equal(a.view(torch.int32), h.view(torch.int32))


# ---- modules ----

def away_from_zero(pre, rng, margin=1e-3):
    """A per-channel bias (float32 values) that keeps every pre-activation pre[n, c, y, x] + b[c] at least ``margin``
    from zero: the first of 200 random candidates per channel that does."""
    b = np.zeros(pre.shape[1], np.float32)
    for c in range(pre.shape[1]):
        for cand in (rng.standard_normal(200) * 0.1).astype(np.float32):
            if float((pre[:, c] + float(cand)).abs().min()) > margin:
                b[c] = cand
                break
        else:
            raise AssertionError(f"no bias keeps channel {c} away from zero")
    return torch.from_numpy(b)


def lrelu(t):
    return F.leaky_relu(t, 0.1)


@pytest.mark.parametrize("layout", ["channels_last", "contiguous"])
@pytest.mark.parametrize("shape", [(2, 64, 11, 13), (2, 64, 12, 20)])
@pytest.mark.parametrize("act", [None, "lrelu"])
def test_conv_down_module_matches_fp64(stif, act, shape, layout):
    T = stif.train
    rng = np.random.default_rng(51)
    gen = torch.Generator().manual_seed(51)
    n, _, H, W = shape
    x = torch.randn(*shape, generator=gen)
    w = torch.randn(64, 64, 3, 3, generator=gen) * 0.05
    go = torch.randn(n, 64, out_size(H), out_size(W), generator=gen)
    b = away_from_zero(F.conv2d(x.double(), w.double(), None, stride=2, padding=1), rng)
    ref = nn.Conv2d(64, 64, 3, 2, 1, dtype=torch.float64)
    with torch.no_grad():
        ref.weight.copy_(w)
        ref.bias.copy_(b)
    xr = x.double().requires_grad_(True)
    pre = ref(xr)
    assert float(pre.detach().abs().min()) > 1e-4                         # the mask is decided on both sides alike
    out_ref = lrelu(pre) if act else pre
    out_ref.backward(go.double())

    m = T.ConvDown(act=act).cuda()
    with torch.no_grad():
        m.weight.copy_(w)
        m.bias.copy_(b)
    xg = x.cuda()
    if layout == "channels_last":
        xg = xg.contiguous(memory_format=torch.channels_last)
        ptr = xg.data_ptr()
    xg.requires_grad_(True)
    out = m(xg)
    assert out.shape == out_ref.shape and out.is_contiguous(memory_format=torch.channels_last)
    out.backward(go.cuda())
    if layout == "channels_last":
        assert xg.data_ptr() == ptr
    errs = dict(out=relmax(out, out_ref), gx=relmax(xg.grad, xr.grad), gw=relmax(m.weight.grad, ref.weight.grad),
                gb=relmax(m.bias.grad, ref.bias.grad))
    print(f"ConvDown act={act} {shape} {layout}: " + " ".join(f"{k} {v:.3e}" for k, v in errs.items()))
    assert max(errs.values()) < RTOL, errs

    m.zero_grad()                      # requires_grad=False on the input: no data gradient, the same weight gradient
    x2 = x.cuda()
    m(x2).backward(go.cuda())
    assert x2.grad is None
    assert relmax(m.weight.grad, ref.weight.grad) < RTOL and relmax(m.bias.grad, ref.bias.grad) < RTOL


def test_conv_first_module_matches_fp64(stif):
    T = stif.train
    rng = np.random.default_rng(52)
    gen = torch.Generator().manual_seed(52)
    frames = torch.rand(2, 3, 11, 13, generator=gen)
    w = torch.randn(64, 3, 3, 3, generator=gen) * 0.2
    go = torch.randn(2, 64, 11, 13, generator=gen)
    b = away_from_zero(F.conv2d(frames.double(), w.double(), None, padding=1), rng)
    ref = nn.Conv2d(3, 64, 3, 1, 1, dtype=torch.float64)
    with torch.no_grad():
        ref.weight.copy_(w)
        ref.bias.copy_(b)
    pre = ref(frames.double())
    assert float(pre.detach().abs().min()) > 1e-4
    out_ref = lrelu(pre)
    out_ref.backward(go.double())
    m = T.ConvFirst().cuda()
    with torch.no_grad():
        m.weight.copy_(w)
        m.bias.copy_(b)
    out = m(frames.cuda())
    assert out.shape == out_ref.shape and out.is_contiguous(memory_format=torch.channels_last)
    out.backward(go.cuda())
    errs = dict(out=relmax(out, out_ref), gw=relmax(m.weight.grad, ref.weight.grad),
                gb=relmax(m.bias.grad, ref.bias.grad))
    print("ConvFirst: " + " ".join(f"{k} {v:.3e}" for k, v in errs.items()))
    assert max(errs.values()) < RTOL, errs
    with pytest.raises(NotImplementedError, match="not built"):
        m(frames.cuda().requires_grad_(True))


class RefBlock(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv2d(64, 64, 3, 1, 1, dtype=torch.float64)
        self.conv2 = nn.Conv2d(64, 64, 3, 1, 1, dtype=torch.float64)

    def forward(self, x):
        self.pre = self.conv1(x)
        return x + self.conv2(F.relu(self.pre))


class RefEncoder(nn.Module):
    """Sakuya_arch_test.py:282-287, :318-325 from nn.Conv2d in float64, the reference's parameter names"""

    def __init__(self, front_RBs):
        super().__init__()
        self.conv_first = nn.Conv2d(3, 64, 3, 1, 1, dtype=torch.float64)
        self.feature_extraction = nn.Sequential(*[RefBlock() for _ in range(front_RBs)])
        self.fea_L2_conv1 = nn.Conv2d(64, 64, 3, 2, 1, dtype=torch.float64)
        self.fea_L2_conv2 = nn.Conv2d(64, 64, 3, 1, 1, dtype=torch.float64)
        self.fea_L3_conv1 = nn.Conv2d(64, 64, 3, 2, 1, dtype=torch.float64)
        self.fea_L3_conv2 = nn.Conv2d(64, 64, 3, 1, 1, dtype=torch.float64)

    def forward(self, x):
        self.pres = []

        def act(conv, t):
            self.pres.append(conv(t))
            return lrelu(self.pres[-1])

        L1 = self.feature_extraction(act(self.conv_first, x))
        self.pres += [b.pre for b in self.feature_extraction]
        L2 = act(self.fea_L2_conv2, act(self.fea_L2_conv1, L1))
        L3 = act(self.fea_L3_conv2, act(self.fea_L3_conv1, L2))
        return L1, L2, L3


ENC_SHAPES = [(2, 3, 11, 13), (2, 3, 12, 20)]
ENC_OPTS = dict(lr_G=2e-5, beta1=0.9, beta2=0.99, weight_decay_G=0, lr_scheme="CosineAnnealingLR_Restart",
                T_period=[3, 3], restarts=[3], restart_weights=[0.5], eta_min=1e-7)


@functools.lru_cache(maxsize=None)
def encoder_reference(shape):
    """The fp64 side, once per frame shape: the reference slices of sd (float32 values; the bias of every activated
    conv moved so that no activation argument starts within 1e-3 of zero), frames, the loss weights r, the three
    outputs and every parameter gradient of loss = sum(L1 r1) + sum(L2 r2) + sum(L3 r3)."""
    import stif_pkg
    sd = stif_pkg.load().weights.make_state_dict(seed=0)
    rng = np.random.default_rng(61 + shape[2])
    gen = torch.Generator().manual_seed(61 + shape[2])
    frames = torch.rand(*shape, generator=gen)
    net = RefEncoder(2)
    init = {k: torch.from_numpy(np.asarray(sd[k])).clone() for k in net.state_dict()}
    with torch.no_grad():
        def settle(name, t, stride=1):
            init[name + ".bias"] = away_from_zero(F.conv2d(t, init[name + ".weight"].double(), None, stride=stride,
                                                           padding=1), rng)
            return F.conv2d(t, init[name + ".weight"].double(), init[name + ".bias"].double(), stride=stride, padding=1)

        h = lrelu(settle("conv_first", frames.double()))
        for i in range(2):
            t = F.relu(settle(f"feature_extraction.{i}.conv1", h))
            h = h + F.conv2d(t, init[f"feature_extraction.{i}.conv2.weight"].double(),
                             init[f"feature_extraction.{i}.conv2.bias"].double(), padding=1)
        for name, stride in (("fea_L2_conv1", 2), ("fea_L2_conv2", 1), ("fea_L3_conv1", 2), ("fea_L3_conv2", 1)):
            h = lrelu(settle(name, h, stride))
    net.load_state_dict({k: v.double() for k, v in init.items()}, strict=True)
    outs = net(frames.double())
    assert min(float(p.detach().abs().min()) for p in net.pres) > 1e-4      # no mask hangs on rounding
    r = [torch.randn(o.shape, generator=gen) for o in outs]
    sum((o * ri.double()).sum() for o, ri in zip(outs, r)).backward()
    grads = {k: p.grad.detach().clone() for k, p in net.named_parameters()}
    return init, frames, r, [o.detach() for o in outs], grads


@pytest.mark.parametrize("shape", ENC_SHAPES)
@pytest.mark.parametrize("mfma", ["f32", "f16x3"])
def test_frame_features_matches_the_oracle_and_fp64_gradients(stif, mfma, shape):
    T = stif.train
    init, frames, r, outs_ref, grads_ref = encoder_reference(shape)
    sd_np = {k: v.numpy() for k, v in init.items()}
    oracle = O.frame_features(frames.numpy(), sd_np, front_RBs=2)
    net = T.FrameFeatures(front_RBs=2, mfma=mfma)
    net.load_state_dict(init, strict=True)
    net.cuda()
    T.range_status()
    outs = net(frames.cuda())
    for name, o, want, ref in zip(("L1", "L2", "L3"), outs, oracle, outs_ref):
        assert tuple(o.shape) == want.shape
        err = relmax(o, want)
        print(f"FrameFeatures {mfma} {shape} {name}: {err:.3e} of max|oracle|")
        assert err < RTOL, (name, err)
        assert relmax(ref, want) < 1e-12                                     # the restatement is the oracle's module
    sum((o * ri.cuda()).sum() for o, ri in zip(outs, r)).backward()
    for k, p in net.named_parameters():
        ref = grads_ref[k]
        err, tol = float((p.grad.double().cpu() - ref).abs().max()), 2e-5 * float(ref.abs().max())
        print(f"FrameFeatures {mfma} {shape} {k}: grad err {err / float(ref.abs().max()):.3e} of max|ref|")
        assert err <= tol, (k, err, tol)
    assert net.range_status() == 0


def test_frame_features_optimisation_step(stif):
    """One train.optimize_step (Charbonnier + Adam, the options of tests/test_gpu_train.py) with the three levels
    concatenated into one output and one target moves every parameter, and the loss matches the fp64 run of the
    same step to 1e-5 relative."""
    T = stif.train
    shape = ENC_SHAPES[0]
    init, frames, _, outs_ref, _ = encoder_reference(shape)
    rng = np.random.default_rng(71)

    class Flat(nn.Module):
        def __init__(self, enc):
            super().__init__()
            self.enc = enc

        def forward(self, x):
            return torch.cat([o.reshape(-1) for o in self.enc(x)])

    flat_ref = torch.cat([o.reshape(-1) for o in outs_ref])
    sign = torch.from_numpy(np.where(rng.random(flat_ref.shape) < 0.5, -1.0, 1.0))
    gt = (flat_ref + sign * (1.0 + torch.from_numpy(rng.random(flat_ref.shape)))).float()
    losses = {}
    for side in ("fp64", "gpu"):
        enc = RefEncoder(2) if side == "fp64" else T.FrameFeatures(front_RBs=2, mfma="f32")
        enc.load_state_dict({k: v.double() if side == "fp64" else v for k, v in init.items()}, strict=True)
        net = Flat(enc)
        if side == "gpu":
            net.cuda()
        before = {k: p.detach().clone() for k, p in net.named_parameters()}
        opt, sch = T.make_optimizer(net, ENC_OPTS)
        T.update_learning_rate([sch], [opt], 1)
        x, g = (frames.double(), gt.double()) if side == "fp64" else (frames.cuda(), gt.cuda())
        losses[side] = T.optimize_step(net, opt, T.CharbonnierLoss(), [x], g)
        for k, p in net.named_parameters():
            assert float((p.detach() - before[k]).abs().max()) > 0, (side, k)     # every parameter moved
    assert abs(losses["gpu"] - losses["fp64"]) <= 1e-5 * abs(losses["fp64"]), losses
    assert T.range_status() == 0
