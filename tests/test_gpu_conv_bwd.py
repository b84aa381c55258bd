"""3x3 / 64 -> 64 conv backward on the GPU: stif_conv3x3_wgrad, stif_pack_conv_weight_dev, the data gradient through
stif_conv3x3_wino with the STIF_PACK_DGRAD packing, and the trainable modules of stif_amd.train on top.

Reference everywhere: torch on the CPU in float64 (F.conv2d under autograd, torch.nn.grad.conv2d_weight /
conv2d_input).  RTOL = 1e-5 of max |ref| is the bar of the fp32-MFMA convs against fp64 (tests/test_gpu_wino.py,
both operand modes), applied to the gradients unchanged; the module tests use the bounds of tests/test_gpu_train.py.

Weight-gradient shapes, from the kernel's tile (TH = 2 rows x TW = 32 columns) and grid (G = min(tiles, 2 per CU)):
1x1x1 (only the centre tap is non-zero), 2x5x7 (below one tile, odd), 1x(TH+1)x(TW+1) (partial tiles on both edges),
3x33x70, items through a strided view (t[0::2]), and 2x192x192 = 1152 tiles, more than the 512 workgroups of a
256-CU device, so that workgroups take two or three tiles.  Every other shape has fewer tiles than a full grid; all of
them run with the cached workspace filled with NaN first (stale contents must not matter)."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

pytestmark = pytest.mark.gpu

RTOL = 1e-5
TH, TW = 2, 32
SHAPES = {"1x1x1": (1, 1, 1), "2x5x7": (2, 5, 7), "tile+1": (1, TH + 1, TW + 1), "3x33x70": (3, 33, 70),
          "strided": (2, 5, 7), "many-tiles": (2, 192, 192)}


def relmax(got, ref):
    ref = torch.as_tensor(ref, dtype=torch.float64)
    return float((got.detach().double().cpu() - ref).abs().max() / ref.abs().max())


def nchw64(t):
    return t.detach().double().cpu().permute(0, 3, 1, 2).contiguous()


@functools.lru_cache(maxsize=None)
def wgrad_case(name):
    """(x, gy) NHWC float32 on the GPU and the fp64 (gw, gb), computed once per shape and never modified."""
    n, H, W = SHAPES[name]
    g = torch.Generator().manual_seed(sorted(SHAPES).index(name) + 100)
    if name == "strided":
        x = torch.randn(2 * n, H, W, 64, generator=g).cuda()[0::2]
        gy = torch.randn(2 * n + 1, H, W, 64, generator=g).cuda()[1::2]
        assert not x.is_contiguous() and x.stride(0) == 2 * H * W * 64
    else:
        x = torch.randn(n, H, W, 64, generator=g).cuda()
        gy = torch.randn(n, H, W, 64, generator=g).cuda()
    gw = torch.nn.grad.conv2d_weight(nchw64(x), (64, 64, 3, 3), nchw64(gy), padding=1)
    return x, gy, gw, nchw64(gy).sum((0, 2, 3))


def poison_workspace(ops, x, gy):
    """Fill the cached weight-gradient workspace with NaN (allocating it by one call if this is the first)."""
    if not ops._WGRAD_WS:
        ops.conv3x3_wgrad(x, gy)
    for ws in ops._WGRAD_WS.values():
        ws.fill_(float("nan"))


@pytest.mark.parametrize("name", list(SHAPES))
def test_weight_and_bias_gradient_match_fp64(stif, name):
    ops = stif.ops
    x, gy, gw_ref, gb_ref = wgrad_case(name)
    poison_workspace(ops, x, gy)
    gw, gb = ops.conv3x3_wgrad(x, gy)
    assert tuple(gw.shape) == (64, 64, 3, 3) and tuple(gb.shape) == (64,)
    ew, eb = relmax(gw, gw_ref), relmax(gb, gb_ref)
    print(f"wgrad {name}: gw {ew:.3e} gb {eb:.3e} of max|ref|")
    assert ew < RTOL and eb < RTOL, (name, ew, eb)
    if name == "1x1x1":
        off_centre = gw.clone()
        off_centre[:, :, 1, 1] = 0
        assert float(off_centre.abs().max()) == 0.0            # every other tap reads padding only


def test_many_tiles_shape_has_more_tiles_than_workgroups(stif):
    n, H, W = SHAPES["many-tiles"]
    part = (64 * 64 * 9 + 64) * 4
    G = stif._lib.lib().stif_conv3x3_wgrad_workspace_size(n, H, W, 64, 64) // part
    tiles = n * -(-H // TH) * -(-W // TW)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert G == min(tiles, 2 * cus) and G < tiles, (G, tiles, cus)


@pytest.mark.parametrize("corner", [(0, 0), (0, 34), (4, 0), (4, 34)])
def test_taps_against_padding(stif, corner):
    """x all ones, gy a single one at a corner pixel: gw is exactly the 0 / 1 pattern of the taps inside the map."""
    H, W, co = 5, 35, 37
    y, xc = corner
    x = torch.ones(1, H, W, 64, device="cuda")
    gy = torch.zeros(1, H, W, 64, device="cuda")
    gy[0, y, xc, co] = 1.0
    gw, gb = stif.ops.conv3x3_wgrad(x, gy)
    want = torch.zeros(64, 64, 3, 3)
    for kh in range(3):
        for kw in range(3):
            if 0 <= y + kh - 1 < H and 0 <= xc + kw - 1 < W:
                want[co, :, kh, kw] = 1.0
    assert 0 < int(want[co, 0].sum()) == 4                       # a corner sees four taps
    assert torch.equal(gw.cpu(), want)
    assert torch.equal(gb.cpu(), torch.eye(64)[co])


def test_weight_gradient_is_deterministic(stif):
    x, gy, _, _ = wgrad_case("many-tiles")
    a = stif.ops.conv3x3_wgrad(x, gy)
    stif.ops.conv3x3_wgrad(*wgrad_case("2x5x7")[:2])             # another shape in between, same workspace
    b = stif.ops.conv3x3_wgrad(x, gy)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---- device packer ----

def same_bytes(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def pack_weights(sd):
    rng = np.random.default_rng(7)
    return {"random": ((rng.standard_normal((64, 64, 3, 3)) * 0.05).astype(np.float32),
                       rng.standard_normal(64).astype(np.float32)),
            "recon_trunk.0.conv1": (sd["recon_trunk.0.conv1.weight"], sd["recon_trunk.0.conv1.bias"])}


@pytest.mark.parametrize("f16", [False, True])
@pytest.mark.parametrize("which", ["random", "recon_trunk.0.conv1"])
def test_device_packer_writes_the_host_packers_bytes(stif, sd, which, f16):
    L, ops = stif._lib, stif.ops
    mode = L.PACK_WINO | (L.PACK_F16X3 if f16 else 0)
    w, b = pack_weights(sd)[which]
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    wd, bd = torch.from_numpy(w).cuda(), torch.from_numpy(b).cuda()
    host = ops.pack_conv(w, b, mode, range_fallback=False)
    dev = ops.pack_conv_dev(wd, bd, mode, status=status)
    assert dev.mode == mode and same_bytes(dev.w, host.w) and same_bytes(dev.b, host.b)
    wt = np.ascontiguousarray(np.flip(w.transpose(1, 0, 2, 3), (2, 3)))
    host_t = ops.pack_conv(wt, np.zeros(64, np.float32), mode, range_fallback=False)
    dev_t = ops.pack_conv_dev(wd, None, mode, dgrad=True, status=status)
    assert same_bytes(dev_t.w, host_t.w) and same_bytes(dev_t.b, host_t.b)
    assert int(status.item()) == 0


def test_device_packer_reports_the_f16x3_range(stif):
    L, ops = stif._lib, stif.ops
    w = torch.full((64, 64, 3, 3), 100.0, device="cuda")
    b = torch.zeros(64, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    ops.pack_conv_dev(w, b, L.PACK_WINO, status=status)
    ops.pack_conv_dev(w, b, L.PACK_WINO)                         # fp32 mode needs no status word
    assert int(status.item()) == 0
    with pytest.raises(L.StifError):                              # the host packer's answer to the same weight
        ops.pack_conv(w.cpu().numpy(), b.cpu().numpy(), L.PACK_WINO | L.PACK_F16X3, range_fallback=False)
    ops.pack_conv_dev(w, b, L.PACK_WINO | L.PACK_F16X3, status=status)
    assert int(status.item()) == L.STATUS_PACK_RANGE
    one = w.clone() * 1e-3
    one[5, 9, 0, 0] = 70.0                                        # one corner tap (U = g there) past 65504 / 1024
    status.zero_()
    ops.pack_conv_dev(one, b, L.PACK_WINO | L.PACK_F16X3, dgrad=True, status=status)
    assert int(status.item()) == L.STATUS_PACK_RANGE


# ---- data gradient: stif_conv3x3_wino with the dgrad packing ----

@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("shape", [(2, 5, 7), (3, 33, 70)])
@pytest.mark.parametrize("f16", [False, True])
def test_data_gradient_through_the_winograd_conv(stif, f16, shape, res):
    L, ops = stif._lib, stif.ops
    n, H, W = shape
    gen = torch.Generator().manual_seed(11)
    w = torch.randn(64, 64, 3, 3, generator=gen) * 0.05
    g = torch.randn(n, H, W, 64, generator=gen)
    r = torch.randn(n, H, W, 64, generator=gen)
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    lay = ops.pack_conv_dev(w.cuda(), None, L.PACK_WINO | (L.PACK_F16X3 if f16 else 0), dgrad=True, status=status)
    out = torch.empty(n, H, W, 64, device="cuda")
    ops.conv2d([dict(layer=lay, in0=g.cuda(), out=out, res=r.cuda() if res else None)],
               epi=L.EPI_RES if res else L.EPI_NONE, status=status)
    ref = torch.nn.grad.conv2d_input((n, 64, H, W), w.double(), nchw64(g), padding=1)
    if res:
        ref = ref + nchw64(r)
    err = relmax(out.permute(0, 3, 1, 2), ref)
    print(f"dgrad f16={f16} {shape} res={res}: {err:.3e} of max|ref|")
    assert err < RTOL, err
    assert int(status.item()) == 0


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


class RefConv(nn.Module):
    """the fp64 side of Conv3x3: nn.Conv2d + the activation"""

    def __init__(self, act):
        super().__init__()
        self.conv = nn.Conv2d(64, 64, 3, 1, 1, dtype=torch.float64)
        self.act = act

    def forward(self, x):
        self.pre = self.conv(x)
        return {None: lambda t: t, "relu": F.relu, "lrelu": lambda t: F.leaky_relu(t, 0.1)}[self.act](self.pre)


@pytest.mark.parametrize("layout", ["channels_last", "contiguous"])
@pytest.mark.parametrize("mfma", ["f32", "f16x3"])
@pytest.mark.parametrize("act", [None, "relu", "lrelu"])
def test_conv3x3_module_matches_fp64(stif, act, mfma, layout):
    T = stif.train
    rng = np.random.default_rng(31)
    gen = torch.Generator().manual_seed(31)
    n, H, W = 2, 7, 37
    x = torch.randn(n, 64, H, W, generator=gen)
    w = torch.randn(64, 64, 3, 3, generator=gen) * 0.05
    go = torch.randn(n, 64, H, W, generator=gen)
    b = away_from_zero(F.conv2d(x.double(), w.double(), None, padding=1), rng)
    ref = RefConv(act)
    with torch.no_grad():
        ref.conv.weight.copy_(w)
        ref.conv.bias.copy_(b)
    xr = x.double().requires_grad_(True)
    out_ref = ref(xr)
    assert float(ref.pre.detach().abs().min()) > 1e-4                    # the mask is decided on both sides alike
    out_ref.backward(go.double())

    m = T.Conv3x3(act=act, mfma=mfma).cuda()
    with torch.no_grad():
        m.weight.copy_(w)
        m.bias.copy_(b)
    xg = x.cuda()
    if layout == "channels_last":
        xg = xg.contiguous(memory_format=torch.channels_last)
        ptr = xg.data_ptr()
    xg.requires_grad_(True)
    T.range_status()
    out = m(xg)
    assert out.shape == (n, 64, H, W) and out.is_contiguous(memory_format=torch.channels_last)
    out.backward(go.cuda())
    if layout == "channels_last":
        assert xg.data_ptr() == ptr
    errs = dict(out=relmax(out, out_ref), gx=relmax(xg.grad, xr.grad), gw=relmax(m.weight.grad, ref.conv.weight.grad),
                gb=relmax(m.bias.grad, ref.conv.bias.grad))
    print(f"Conv3x3 act={act} {mfma} {layout}: " + " ".join(f"{k} {v:.3e}" for k, v in errs.items()))
    assert max(errs.values()) < RTOL, errs
    assert m.range_status() == 0

    # requires_grad=False on the input: no data gradient, the same weight gradient
    m.zero_grad()
    x2 = x.cuda()
    m(x2).backward(go.cuda())
    assert x2.grad is None
    assert relmax(m.weight.grad, ref.conv.weight.grad) < RTOL and relmax(m.bias.grad, ref.conv.bias.grad) < RTOL


class RefBlock(nn.Module):
    """module_util.py:34-52 from nn.Conv2d in float64"""

    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv2d(64, 64, 3, 1, 1, dtype=torch.float64)
        self.conv2 = nn.Conv2d(64, 64, 3, 1, 1, dtype=torch.float64)

    def forward(self, x):
        self.pre = self.conv1(x)
        return x + self.conv2(F.relu(self.pre))


# One step: 420 pixels, partial tiles on both edges.  The six-iteration loop: 30 pixels and a wider starting margin.
# Adam moves every weight by ~lr per step whatever its gradient, so a weight whose gradient's sign hangs on rounding
# ends 2 lr away from the reference's, and the ReLU arguments it feeds drift ~1e-5 apart between the two runs; with
# few pixels and arguments that start 1e-2 from zero none comes near enough for its mask to flip (asserted below on
# the fp64 side: every argument stays 1e-4 away in every iteration).
TRUNK_CASES = {(1, 1): ((2, 64, 6, 35), 1e-3), (2, 1): ((2, 64, 6, 35), 1e-3), (2, 6): ((2, 64, 3, 5), 1e-2)}
TRUNK_OPTS = dict(lr_G=2e-5, beta1=0.9, beta2=0.99, weight_decay_G=0, lr_scheme="CosineAnnealingLR_Restart",
                  T_period=[3, 3], restarts=[3], restart_weights=[0.5], eta_min=1e-7)


@functools.lru_cache(maxsize=None)
def trunk_reference(n_blocks, iters):
    """The fp64 run on the CPU, once per (blocks, iterations): initial state dict (float32 values; recon_trunk's
    weights, conv1 biases moved so that no ReLU argument starts within the case's margin of zero), input, target, and per
    iteration the loss, the learning rate, the gradients and the smallest |ReLU argument|."""
    import stif_pkg
    stif = stif_pkg.load()
    T = stif.train
    sd = stif.weights.make_state_dict(seed=0)
    shape, margin = TRUNK_CASES[n_blocks, iters]
    rng = np.random.default_rng(41 + n_blocks)
    gen = torch.Generator().manual_seed(41 + n_blocks)
    x = torch.randn(*shape, generator=gen)
    net = nn.Sequential(*[RefBlock() for _ in range(n_blocks)])
    init = {}
    with torch.no_grad():
        h = x.double()
        for i, blk in enumerate(net):
            for name in ("conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias"):
                init[f"{i}.{name}"] = torch.from_numpy(np.asarray(sd[f"recon_trunk.{i}.{name}"])).clone()
            init[f"{i}.conv1.bias"] = away_from_zero(F.conv2d(h, init[f"{i}.conv1.weight"].double(), None, padding=1), rng,
                                                       margin)
            blk.load_state_dict({k[len(f"{i}."):]: v.double() for k, v in init.items() if k.startswith(f"{i}.")})
            h = blk(h)
        # the target sits 1-2 away from the output everywhere (tests/test_gpu_train.py: the Charbonnier gradient is
        # then ~sign(d) and well conditioned)
        sign = torch.from_numpy(np.where(rng.random(h.shape) < 0.5, -1.0, 1.0))
        gt = (h + sign * (1.0 + torch.from_numpy(rng.random(h.shape)))).float()
    opt, sch = T.make_optimizer(net, TRUNK_OPTS)
    crit = T.CharbonnierLoss()
    steps = []
    for it in range(1, iters + 1):
        T.update_learning_rate([sch], [opt], it)
        lr = opt.param_groups[0]["lr"]
        loss = T.optimize_step(net, opt, crit, [x.double()], gt.double())
        steps.append(dict(loss=loss, lr=lr, grads={k: v.grad.detach().clone() for k, v in net.named_parameters()},
                          min_pre=min(float(b.pre.detach().abs().min()) for b in net)))
    return init, x, gt, steps, {k: v.detach().clone() for k, v in net.named_parameters()}


@pytest.mark.parametrize("mfma", ["f32", "f16x3"])
@pytest.mark.parametrize("n_blocks,iters", [(1, 1), (2, 1), (2, 6)])
def test_residual_trunk_trains_like_the_fp64_modules(stif, n_blocks, iters, mfma):
    """One step of a ResidualBlock_noBN and of a two-block make_trunk, and the six-iteration restart-schedule loop of
    tests/test_gpu_train.py (update_learning_rate, then optimize_step: Charbonnier + Adam), against the same modules
    built from nn.Conv2d in float64 on the CPU, with that test's bounds: loss 1e-5 relative, gradients 2e-5 of
    max |ref|, firm-gradient parameters within 1e-6 per step, range_status() == 0 throughout."""
    T = stif.train
    init, x, gt, steps, p_ref = trunk_reference(n_blocks, iters)
    assert min(s["min_pre"] for s in steps) > 1e-4, [s["min_pre"] for s in steps]   # no ReLU mask hangs on rounding
    net = T.make_trunk(n_blocks, mfma=mfma) if n_blocks > 1 else nn.Sequential(T.ResidualBlock_noBN(mfma=mfma))
    net.load_state_dict(init, strict=True)
    net.cuda()
    opt, sch = T.make_optimizer(net, TRUNK_OPTS)
    crit = T.CharbonnierLoss()
    xg, gg = x.cuda().contiguous(memory_format=torch.channels_last), gt.cuda()
    T.range_status()
    firm = {k: torch.ones_like(v, dtype=torch.bool) for k, v in p_ref.items()}
    for it, ref in enumerate(steps, 1):
        T.update_learning_rate([sch], [opt], it)
        assert opt.param_groups[0]["lr"] == ref["lr"]
        loss = T.optimize_step(net, opt, crit, [xg], gg)
        assert abs(loss - ref["loss"]) <= 1e-5 * abs(ref["loss"]), (it, loss, ref["loss"])
        for k, p in net.named_parameters():
            r = ref["grads"][k]
            err, tol = float((p.grad.double().cpu() - r).abs().max()), 2e-5 * float(r.abs().max())
            print(f"trunk {n_blocks} blocks {mfma} it {it} {k}: grad err {err / float(r.abs().max()):.3e} of max|ref|")
            assert err <= tol, (it, k, err, tol)
            firm[k] &= r.abs() > 1e-3 * r.abs().max()
        assert net[0].range_status() == 0
    # Adam normalises each update, so only entries whose gradient sign rounding could flip may differ, by at most
    # one lr-sized step per iteration
    for k, p in net.named_parameters():
        d = (p.detach().double().cpu() - p_ref[k]).abs()
        assert float(d[firm[k]].max()) <= 1e-6 * iters, (k, float(d[firm[k]].max()))
        assert float(d.max()) <= iters * 2 * 2e-5 + 1e-6, (k, float(d.max()))
