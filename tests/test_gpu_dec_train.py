"""The trainable SIREN decoder on the GPU: stif_siren_fwd / _bwd, the input builders stif_dec_x{1,2,3}_fwd and their
adjoints, and train.Decoder / train.LunaTokis on top of them.

Reference everywhere: torch on the CPU in float64 (tests/dec_torch_ref.py, pinned to the numpy oracle by
tests/test_dec_train_host.py).  Tolerance, the rule of tests/test_gpu_pcd_train.py and tests/test_gpu_lstm_train.py:
1e-5 of max |ref| for the kernels that only move memory (builders, adjoints); max(2e-5, 4 e32) of max |ref| per tensor
for anything with a SIREN chain in it, e32 being the error of the same torch reference run in float32 on the CPU against
its float64 run, computed here.  Every observed error is printed.  Outputs and workspaces are pre-filled with NaN.

Row counts of the MLP kernels follow their row tile T = 64: 1, T - 1, T + 1, 2 T + 1, and one feat_imnet case with more
row tiles than any layer's weight pass launches workgroups (``big_rows``).  Builder sizes: 1x1 -> 3x2, 5x7 -> 11x13
(a non-integer scale), 4x4 -> 16x16 and 2 items of 8x12 -> 16x24."""
import functools
import math

import numpy as np
import pytest
import torch

import dec_torch_ref as R

pytestmark = pytest.mark.gpu

RTOL, RTOL_CHAIN = 1e-5, 2e-5
NAN = float("nan")
NETS = {"feat_imnet": (201, (64, 64, 256), 64), "flow_imnet": (263, (64, 64, 256), 4),
        "encode_imnet": (525, (64, 64, 256, 256), 3)}
T_ROWS = 64
SIZES = {"1x1-3x2": (1, 1, 1, 3, 2), "5x7-11x13": (1, 5, 7, 11, 13), "4x4-16x16": (1, 4, 4, 16, 16),
         "2x8x12-16x24": (2, 8, 12, 16, 24)}


def relmax(got, ref):
    ref = torch.as_tensor(ref, dtype=torch.float64).detach()
    return float((got.detach().double().cpu() - ref).abs().max() / ref.abs().max())


def check(name, got, ref, tol):
    e = relmax(got, ref)
    print(f"  {name}: {e:.3e} of max|ref| (tol {tol:.1e})")
    assert e <= tol, (name, e, tol)


def chain_tol(ref64, ref32):
    return max(RTOL_CHAIN, 4 * relmax(ref32, ref64))


def same_bytes(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def nan_like(shape):
    return torch.full(tuple(shape), NAN, device="cuda")


# ---- the MLP kernels ----

def big_rows(stif):
    """More row tiles than any layer of feat_imnet launches workgroups in the weight pass.  The launch rule
    (stif_siren_wgrad_grid): min(row tiles, max(1, 2 CUs / 64 x 64 blocks of the layer)) workgroups per block, so the
    largest grid any layer can get is that of a one-block layer (64 -> 64); T (that + 1) + 1 rows exceed it by a full
    tile and a part-filled one."""
    cin, hidden, cout = NETS["feat_imnet"]
    dims = (cin,) + hidden + (cout,)
    cap = max(stif._lib.lib().stif_siren_wgrad_grid(10 ** 8, dims[l + 1], dims[l]) for l in range(len(dims) - 1))
    return T_ROWS * (cap + 1) + 1


@functools.lru_cache(maxsize=None)
def mlp_case(net, n):
    """float32 parameters, X [n, kp] with zero pads and g_Y, and the float64 / float32 CPU autograd results."""
    cin, hidden, cout = NETS[net]
    g = torch.Generator().manual_seed(100 + sorted(NETS).index(net))
    dims = (cin,) + hidden + (cout,)
    ws, bs = [], []
    for l in range(len(dims) - 1):
        bound = 1.0 / dims[l] if l == 0 else math.sqrt(6.0 / dims[l]) / 30.0
        ws.append((torch.rand(dims[l + 1], dims[l], generator=g) * 2 - 1) * bound)
        bs.append((torch.rand(dims[l + 1], generator=g) * 2 - 1) / math.sqrt(dims[l]))
    ws[0] = ws[0] * 16           # |30 z_0| into the hundreds: the argument reduction of sin and cos is exercised
    kp = (cin + 7) // 8 * 8
    x = torch.zeros(n, kp)
    x[:, :cin] = torch.randn(n, cin, generator=g) * 2
    gy = torch.randn(n, cout, generator=g)
    out = {}
    for dt in (torch.float64, torch.float32):
        xr = x[:, :cin].to(dt).clone().requires_grad_(True)
        P = [w.to(dt).clone().requires_grad_(True) for w in ws] + [b.to(dt).clone().requires_grad_(True) for b in bs]
        nl = len(ws)
        a = xr
        zmax = 0.0
        for l in range(nl - 1):
            z = torch.nn.functional.linear(a, P[l], P[nl + l])
            zmax = max(zmax, float(z.detach().abs().max()))
            a = torch.sin(30.0 * z)
        y = torch.nn.functional.linear(a, P[nl - 1], P[2 * nl - 1])
        (y * gy.to(dt)).sum().backward()
        out[dt] = dict(y=y.detach(), g_x=xr.grad, g_w=[p.grad for p in P[:nl]], g_b=[p.grad for p in P[nl:]], zmax=zmax)
    return ws, bs, x, gy, out[torch.float64], out[torch.float32]


def run_mlp(stif, net, n, strided=False, need_x=True, poison=NAN):
    ops = stif.ops
    ws, bs, x, gy, r64, r32 = mlp_case(net, n)
    cin, hidden, cout = NETS[net]
    kp, zw = x.shape[1], sum(hidden)
    if strided:
        wide = torch.full((n, kp + 8), NAN)
        wide[:, :kp] = x
        xd = wide.cuda()[:, :kp]
        gx = nan_like((n, kp + 16))[:, :kp]
        assert xd.stride(0) == kp + 8 and gx.stride(0) == kp + 16
    else:
        xd, gx = x.cuda(), nan_like((n, kp))
    wd, bd = [w.cuda() for w in ws], [b.cuda() for b in bs]
    y, z = ops.siren_fwd(xd, wd, bd, y=nan_like((n, cout)), z=nan_like((n, zw)))
    nbytes = stif._lib.lib().stif_siren_bwd_workspace_size(n, len(hidden))
    wsb = torch.full((nbytes // 4,), poison, device="cuda")
    gp = ([nan_like(w.shape) for w in ws], [nan_like(b.shape) for b in bs])
    g_x, g_ws, g_bs = ops.siren_bwd(xd, z, wd, bd, gy.cuda(), need_x=need_x, g_x=gx if need_x else None, workspace=wsb,
                                    g_params=gp)
    return y, z, g_x, g_ws, g_bs, gx


def check_mlp(stif, net, n, strided=False):
    cin = NETS[net][0]
    ws, bs, x, gy, r64, r32 = mlp_case(net, n)
    print(f"{net} n={n} strided={strided}: max|z| {r64['zmax']:.2f} (|30 z| {30 * r64['zmax']:.0f})")
    y, z, g_x, g_ws, g_bs, gx_buf = run_mlp(stif, net, n, strided)
    assert bool(torch.isfinite(z).all())
    check("y", y, r64["y"], chain_tol(r64["y"], r32["y"]))
    check("g_x", g_x[:, :cin], r64["g_x"], chain_tol(r64["g_x"], r32["g_x"]))
    assert bool((g_x[:, cin:] == 0).all()), "the pad columns of g_x must be exactly zero"
    if strided:     # nothing is written between the rows
        assert bool(torch.isnan(gx_buf._base[:, gx_buf.shape[1]:]).all())
    for l, (gw, gb) in enumerate(zip(g_ws, g_bs)):
        check(f"g_w[{l}]", gw, r64["g_w"][l], chain_tol(r64["g_w"][l], r32["g_w"][l]))
        check(f"g_b[{l}]", gb, r64["g_b"][l], chain_tol(r64["g_b"][l], r32["g_b"][l]))
    return g_ws, g_bs


@pytest.mark.parametrize("n", [1, T_ROWS - 1, T_ROWS + 1, 2 * T_ROWS + 1])
@pytest.mark.parametrize("net", sorted(NETS))
def test_siren_kernels_match_fp64(stif, net, n):
    assert stif._lib.SIREN_ROW_TILE == T_ROWS
    check_mlp(stif, net, n)


def test_siren_more_row_tiles_than_weight_pass_workgroups(stif):
    """``big_rows``: every layer's weight pass walks several row tiles per workgroup."""
    n = big_rows(stif)
    lib = stif._lib.lib()
    assert (n + T_ROWS - 1) // T_ROWS > max(lib.stif_siren_wgrad_grid(n, co, ci) for co, ci in
                                            ((64, 201), (64, 64), (256, 64), (64, 256)))
    check_mlp(stif, "feat_imnet", n)


@pytest.mark.parametrize("net", sorted(NETS))
def test_siren_strided_rows_with_nan_between_them(stif, net):
    check_mlp(stif, net, 2 * T_ROWS + 1, strided=True)


@pytest.mark.parametrize("net", sorted(NETS))
def test_siren_weight_gradients_are_bit_identical_and_g_x_is_optional(stif, net):
    n = 2 * T_ROWS + 1
    a = run_mlp(stif, net, n, poison=NAN)
    b = run_mlp(stif, net, n, poison=1e30)
    c = run_mlp(stif, net, n, need_x=False, poison=-7.0)
    assert c[2] is None
    for other in (b, c):
        for l in range(len(a[3])):
            assert same_bytes(a[3][l], other[3][l]) and same_bytes(a[4][l], other[4][l]), (net, l)
    assert same_bytes(a[0], b[0]) and same_bytes(a[2], b[2])
    r64, r32 = mlp_case(net, n)[4:]
    for l, gw in enumerate(c[3]):
        check(f"g_w[{l}] without g_x", gw, r64["g_w"][l], chain_tol(r64["g_w"][l], r32["g_w"][l]))


# ---- the builders and their adjoints ----

MARGIN = 0.05


def sample_margins(ux, uy, H, W, HH, WW):
    """The least distance to an integer of every warped sample coordinate, un-normalised on the LR and on the HR
    lattice, per pixel: ux / uy [B, Q, 2] unclamped float64 grids -> [B, Q]."""
    gx, gy = ux.clamp(R.LO, R.HI), uy.clamp(R.LO, R.HI)
    m = [R.integer_margin(R.unnormalise(gx, n)) for n in (W, WW)] + [R.integer_margin(R.unnormalise(gy, n)) for n in (H, HH)]
    return torch.stack(m, 0).amin(dim=(0, 3))


def clamp_margins(ux, uy):
    """The least distance of every unclamped grid coordinate to a clamp bound, per pixel."""
    d = [(u - b).abs() for u in (ux, uy) for b in (R.LO, R.HI)]
    return torch.stack(d, 0).amin(dim=(0, 3))


def draw_flow(B, H, W, HH, WW, g):
    """A float32 flow [B, Q, 4] (HR pixels) drawn per pixel by rejection: a few pixels of motion, about a tenth of the
    pixels pushed past each side of each axis (clamped there), and every sample coordinate at least MARGIN from an
    integer on both lattices and 1e-3 from a clamp bound."""
    Q = HH * WW
    flow = torch.zeros(B, Q, 4)
    todo = torch.ones(B, Q, dtype=torch.bool)
    for _ in range(400):
        if not bool(todo.any()):
            break
        cand = torch.randn(B, Q, 4, generator=g) * 1.5
        side = torch.rand(B, Q, generator=g)
        which = torch.randint(0, 2, (B, Q), generator=g)       # which of the two grids is pushed out
        for k, (lo, comp, size) in enumerate(((0.0, 0, WW), (0.1, 0, WW), (0.2, 1, HH), (0.3, 1, HH))):
            pick = (side >= lo) & (side < lo + 0.1)
            sign = -1.0 if k % 2 == 0 else 1.0
            for grid in range(2):
                sel = pick & (which == grid)
                cand[..., 2 * grid + comp] = torch.where(sel, sign * (size + 1.5 + cand[..., 2 * grid + comp].abs()),
                                                         cand[..., 2 * grid + comp])
        ux, uy = R.warp_grids(cand.double(), HH, WW, torch.float64)
        ok = (sample_margins(ux, uy, H, W, HH, WW) >= MARGIN) & (clamp_margins(ux, uy) >= 1e-3)
        take = todo & ok
        flow[take] = cand[take]
        todo &= ~ok
    assert not bool(todo.any()), "rejection sampling did not place every pixel"
    return flow


@functools.lru_cache(maxsize=None)
def builder_case(name):
    B, H, W, HH, WW = SIZES[name]
    g = torch.Generator().manual_seed(300 + sorted(SIZES).index(name))
    Q = HH * WW
    feat = torch.randn(B, 3, 64, H, W, generator=g)
    inp = torch.rand(B, 2, 3, H, W, generator=g)
    t = torch.rand(B, generator=g)
    hrfeat = torch.randn(B, Q, 64, generator=g)
    flow = draw_flow(B, H, W, HH, WW, g)
    gx1, gx2, gx3 = (torch.randn(B, Q, w, generator=g) for w in (208, 264, 528))
    f64 = feat.double().requires_grad_(True)
    x1, tail = R.stage1_inputs(f64, inp, t, HH, WW)
    (x1 * gx1[..., :201].double()).sum().backward()
    g_feat1, f64.grad = f64.grad, None
    (tail * gx2[..., 64:263].double()).sum().backward()
    g_feat2, f64.grad = f64.grad, None
    hr64, fl64 = hrfeat.double().requires_grad_(True), flow.double().requires_grad_(True)
    x3, ux, uy = R.stage2_inputs(f64, inp, hr64, fl64, t, HH, WW)
    (x3 * gx3[..., :525].double()).sum().backward()
    # the margins hold on the float64 reference before anything is compared
    assert float(sample_margins(ux.detach(), uy.detach(), H, W, HH, WW).min()) >= MARGIN
    assert float(clamp_margins(ux.detach(), uy.detach()).min()) >= 1e-3
    clamped = torch.stack([(ux < R.LO) | (ux > R.HI), (uy < R.LO) | (uy > R.HI)], -1).detach()   # [B, Q, grid, (x, y)]
    ref = dict(x1=x1.detach(), tail=tail.detach(), x3=x3.detach(), g_feat1=g_feat1, g_feat2=g_feat2, g_feat3=f64.grad,
               g_hr3=hr64.grad, g_flow=fl64.grad, clamped=clamped.reshape(B, Q, 4), ux=ux.detach(), uy=uy.detach())
    return feat, inp, t, hrfeat, flow, (gx1, gx2, gx3), ref


def nhwc_lat(t5):
    """[B, 3, 64, H, W] -> the NHWC latent [B, H, W, 192]"""
    B, _, _, H, W = t5.shape
    return t5.reshape(B, 192, H, W).permute(0, 2, 3, 1).contiguous()


def make_geom(stif, name):
    B, H, W, HH, WW = SIZES[name]
    feat, inp, t = builder_case(name)[:3]
    return stif.ops.DecTrainGeom(nhwc_lat(feat).cuda(), inp.reshape(B, 6, H, W).cuda(), t.cuda(), HH, WW)


@pytest.mark.parametrize("name", sorted(SIZES))
def test_x1_and_x2_builders_and_adjoints(stif, name):
    ops = stif.ops
    B, H, W, HH, WW = SIZES[name]
    N = B * HH * WW
    feat, inp, t, hrfeat, flow, (gx1, gx2, gx3), ref = builder_case(name)
    geom = make_geom(stif, name)
    print(f"{name}:")
    x1 = ops.dec_x1_fwd(geom, nan_like((N, 208)))
    check("x1", x1[:, :201], ref["x1"].reshape(N, 201), RTOL)
    assert bool((x1[:, 201:] == 0).all())
    g1 = gx1.reshape(N, 208).cuda()
    g_feat = ops.dec_x1_bwd(geom, g1, nan_like((B, H, W, 192)))
    check("x1_bwd g_feat", g_feat, nhwc_lat(ref["g_feat1"]), RTOL)
    assert same_bytes(g_feat, ops.dec_x1_bwd(geom, g1, nan_like((B, H, W, 192))))
    hr = hrfeat.reshape(N, 64).cuda()
    x2 = ops.dec_x2_fwd(geom, hr, nan_like((N, 264)))
    assert same_bytes(x2[:, :64], hr)
    check("x2", x2[:, 64:263], ref["tail"].reshape(N, 199), RTOL)
    assert bool((x2[:, 263:] == 0).all())
    g2 = gx2.reshape(N, 264).cuda()
    g_hr, g_feat = ops.dec_x2_bwd(geom, g2, nan_like((N, 64)), nan_like((B, H, W, 192)))
    assert same_bytes(g_hr, g2[:, :64])
    check("x2_bwd g_feat", g_feat, nhwc_lat(ref["g_feat2"]), RTOL)
    again = ops.dec_x2_bwd(geom, g2, nan_like((N, 64)), nan_like((B, H, W, 192)))
    assert same_bytes(g_hr, again[0]) and same_bytes(g_feat, again[1])


@pytest.mark.parametrize("name", sorted(SIZES))
def test_x3_builder_and_adjoint(stif, name):
    ops = stif.ops
    B, H, W, HH, WW = SIZES[name]
    N = B * HH * WW
    feat, inp, t, hrfeat, flow, (gx1, gx2, gx3), ref = builder_case(name)
    geom = make_geom(stif, name)
    cl = ref["clamped"]
    # a deliberate share of the pixels is clamped on each side of each axis, so some corners fall outside the map
    sides = [int(((u < R.LO) if lo else (u > R.HI)).sum()) for u in (ref["ux"], ref["uy"]) for lo in (True, False)]
    print(f"{name}: clamped low/high x, low/high y: {sides} of {2 * N} samples")
    assert all(s > 0 for s in sides) and int((~cl).sum()) > 0
    hr, fl = hrfeat.reshape(N, 64).cuda(), flow.reshape(N, 4).cuda()
    x3 = ops.dec_x3_fwd(geom, hr, fl, nan_like((N, 528)))
    check("x3", x3[:, :525], ref["x3"].reshape(N, 525), RTOL)
    assert bool((x3[:, 525:] == 0).all())
    g_flow, g_hr, g_feat = ops.dec_x3_bwd(geom, hr, fl, gx3.reshape(N, 528).cuda(), nan_like((N, 4)))
    check("x3_bwd g_flow", g_flow, ref["g_flow"].reshape(N, 4), RTOL)
    assert bool((g_flow.cpu()[cl.reshape(N, 4)] == 0).all()), "g_flow must be exactly zero where the clamp is active"
    assert bool((ref["g_flow"].reshape(N, 4)[cl.reshape(N, 4)] == 0).all())
    check("x3_bwd g_hrfeat", g_hr, ref["g_hr3"].reshape(N, 64), RTOL)
    check("x3_bwd g_feat", g_feat, nhwc_lat(ref["g_feat3"]), RTOL)


# ---- train.Decoder ----

DEC_SIZES = [(1, 5, 7, 11, 13), (2, 8, 12, 16, 24)]
DEC_TIMES = [0.5, 0.3]
PIX = 1e-4      # over ten times the float32 coordinate error at these sizes (24 * 2^-24 * a few operations)


def decoder_params(seed):
    """Reference-initialised SIREN parameters as float32 tensors under the state-dict names."""
    g = torch.Generator().manual_seed(seed)
    P = {}
    for net, (cin, hidden, cout) in NETS.items():
        dims = (cin,) + hidden + (cout,)
        for l in range(len(dims) - 1):
            bound = 1.0 / dims[l] if l == 0 else math.sqrt(6.0 / dims[l]) / 30.0
            name = f"{net}.net.{l}.linear." if l < len(hidden) else f"{net}.net.{l}."
            P[name + "weight"] = (torch.rand(dims[l + 1], dims[l], generator=g) * 2 - 1) * bound
            P[name + "bias"] = (torch.rand(dims[l + 1], generator=g) * 2 - 1) / math.sqrt(dims[l])
    return P


def decoder_run(P, feat, inp, G, HH, WW, dtype):
    """The reference forward and every gradient of sum_i (pred_i * G_i) in ``dtype`` on the CPU."""
    Pd = {k: v.to(dtype).clone().requires_grad_(True) for k, v in P.items()}
    fd = feat.to(dtype).clone().requires_grad_(True)
    B = feat.shape[0]
    preds, mids = [], []
    for t in DEC_TIMES:
        tb = torch.full((B,), t, dtype=dtype)
        s1 = R.decode_stage1(fd, inp, tb, Pd, HH, WW, dtype)
        s2 = R.decode_stage2(fd, inp, s1["hrfeat"], s1["flow"], tb, Pd, HH, WW, dtype)
        preds.append(s2["pred"])
        mids.append({**s1, **s2})
    sum((p * g.to(dtype)).sum() for p, g in zip(preds, G)).backward()
    return preds, mids, {k: v.grad for k, v in Pd.items()}, fd.grad


def decoder_case_for_seed(B, H, W, HH, WW, seed):
    g = torch.Generator().manual_seed(1000 + seed)
    feat = torch.randn(B, 3, 64, H, W, generator=g) * 0.5
    inp = torch.rand(B, 2, 3, H, W, generator=g)
    G = [torch.randn(B, 3, HH, WW, generator=g) for _ in DEC_TIMES]
    P = decoder_params(2000 + seed)
    # flow_imnet's last layer scaled so that the float64 flow reaches 0.75 HR pixel (it is linear in that layer)
    with torch.no_grad():
        P64 = {k: v.double() for k, v in P.items()}
        m = max(float(R.decode_stage1(feat, inp, torch.full((B,), t, dtype=torch.float64), P64, HH, WW)["flow"].abs().max())
                for t in DEC_TIMES)
    for k in ("flow_imnet.net.3.weight", "flow_imnet.net.3.bias"):
        P[k] = P[k] * (0.75 / m)
    return feat, inp, G, P


def decoder_margins(mids, H, W, HH, WW):
    """(least distance of a warped sample coordinate to an integer, in pixels of its lattice; least distance of an
    unclamped grid coordinate to a clamp bound, in HR pixels; max |flow|) of the float64 reference."""
    ints, bounds, fl = [], [], []
    for m in mids:
        ux, uy = m["ux"].detach(), m["uy"].detach()
        ints.append(float(sample_margins(ux, uy, H, W, HH, WW).min()))
        bounds.append(min(float(((ux - b).abs() * WW / 2).min()) for b in (R.LO, R.HI)))
        bounds.append(min(float(((uy - b).abs() * HH / 2).min()) for b in (R.LO, R.HI)))
        fl.append(float(m["flow"].detach().abs().max()))
    return min(ints), min(bounds), max(fl)


@functools.lru_cache(maxsize=None)
def decoder_case(B, H, W, HH, WW):
    """The first seed in 0..31 whose float64 reference keeps every warped sample coordinate PIX from an integer and
    from the clamp bound; fails loudly if there is none.  The cap on excluded pixels is zero."""
    for seed in range(32):
        feat, inp, G, P = decoder_case_for_seed(B, H, W, HH, WW, seed)
        r64 = decoder_run(P, feat, inp, G, HH, WW, torch.float64)
        near_int, near_bound, flow_max = decoder_margins(r64[1], H, W, HH, WW)
        if near_int >= PIX and near_bound >= PIX:
            assert flow_max >= 0.5, flow_max
            print(f"decoder case {B}x{H}x{W}->{HH}x{WW}: seed {seed}, integer margin {near_int:.2e}, bound margin "
                  f"{near_bound:.2e}, max|flow| {flow_max:.3f} px")
            return feat, inp, G, P, r64, decoder_run(P, feat, inp, G, HH, WW, torch.float32)
    raise AssertionError(f"no seed in 0..31 keeps the warped samples {PIX} px from the lattice at {B}x{H}x{W}")


@pytest.mark.parametrize("B,H,W,HH,WW", DEC_SIZES)
def test_decoder_forward_and_every_gradient(stif, B, H, W, HH, WW):
    feat, inp, G, P, r64, r32 = decoder_case(B, H, W, HH, WW)
    dec = stif.train.Decoder()
    dec.load_state_dict(P, strict=True)
    dec = dec.cuda()
    fd = feat.cuda().requires_grad_(True)
    times = [torch.full((B, 1), DEC_TIMES[0]), DEC_TIMES[1]]           # the reference's [B, 1] tensor, and a float
    outs = dec(fd, inp.cuda(), times, (HH, WW))
    sum((o * g.cuda()).sum() for o, g in zip(outs, G)).backward()
    for i, o in enumerate(outs):
        assert tuple(o.shape) == (B, 3, HH, WW)
        check(f"pred[{i}]", o, r64[0][i], chain_tol(r64[0][i], r32[0][i]))
    check("g_feat", fd.grad, r64[3], chain_tol(r64[3], r32[3]))
    named = dict(dec.named_parameters())
    assert len(named) == 26
    for k in sorted(named):
        check("g " + k, named[k].grad, r64[2][k], chain_tol(r64[2][k], r32[2][k]))
    assert inp.requires_grad is False


def close(a, b, rtol=1e-4, atol=1e-6):
    """(ok, max |a - b|, worst ratio of |a - b| to its elementwise bound): the inference engine's yardstick"""
    a, b = a.detach().cpu().numpy().astype(np.float64), np.asarray(b, np.float64)
    d, lim = np.abs(a - b), rtol * np.abs(b) + atol
    return bool((d <= lim).all()), float(d.max()), float((d / lim).max())


def test_decoder_matches_the_reference_fixture(stif, sd, golden):
    gm = golden["model_16x20"]
    dec = stif.train.Decoder()
    dec.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in sd.items() if "imnet" in k}, strict=True)
    dec = dec.cuda()
    seen = {}

    def first(name):
        def hook(_m, _i, out):
            seen.setdefault(name, out)
        return hook

    dec.feat_imnet.register_forward_hook(first("hrfeat"))
    dec.flow_imnet.register_forward_hook(first("flow"))
    feat, x = torch.from_numpy(gm["feat"])[None].cuda(), torch.from_numpy(gm["x"]).cuda()
    with torch.no_grad():
        first = dec(feat, x, [0.5])[0]
        outs = dec(feat, x, [torch.tensor([[float(t)]]) for t in gm["times"]])
        out25 = dec(feat, x, [0.5], (torch.tensor([40]), torch.tensor([50])))[0]
    assert float(gm["times"][0]) != 0.5 or same_bytes(first, outs[0])
    pairs = [("hrfeat_t05", seen["hrfeat"], gm["hrfeat_t05"]), ("flow_t05", seen["flow"], gm["flow_t05"]),
             ("out_scale_40x50", out25[0], gm["out_scale_40x50"])]
    pairs += [(f"out[{i}]", o[0], gm["out"][i]) for i, o in enumerate(outs)]
    results = {name: close(got, want) for name, got, want in pairs}
    for name, (ok, err, ratio) in results.items():
        print(f"  {name}: max err {err:.3e}, worst ratio to the elementwise bound {ratio:.3f}")
    assert all(ok for ok, _, _ in results.values()), results


# ---- train.LunaTokis ----

@pytest.mark.parametrize("mfma", ["f16x3", "f32"])
def test_lunatokis_loads_the_442_keys_and_matches_the_fixture(stif, sd, golden, mfma):
    gm = golden["model_16x20"]
    net = stif.train.LunaTokis(5, 40, mfma)
    net.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in sd.items()}, strict=True)
    assert len(net.state_dict()) == 442
    net = net.cuda()
    with torch.no_grad():
        outs = net(torch.from_numpy(gm["x"]).cuda(), [torch.tensor([[float(t)]]) for t in gm["times"]])
    for i, o in enumerate(outs):
        ok, err, ratio = close(o[0], gm["out"][i])
        print(f"  {mfma} out[{i}]: max err {err:.3e}, worst ratio to the elementwise bound {ratio:.3f}")
        assert tuple(o.shape) == (1, 3, 64, 80) and ok, (i, err, ratio)
    assert net.range_status() == 0


def test_lunatokis_takes_an_optimiser_step(stif, sd):
    TR = stif.train
    net = TR.LunaTokis(5, 40)
    net.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in sd.items()}, strict=True)
    net = net.cuda()
    before = {k: v.detach().clone() for k, v in net.named_parameters()}
    g = torch.Generator().manual_seed(11)
    x = torch.rand(1, 2, 3, 8, 12, generator=g).cuda()
    times = [torch.tensor([[0.25]]), torch.tensor([[0.75]])]
    gt = torch.rand(1, 2, 3, 16, 24, generator=g).cuda()
    opt, _ = TR.make_optimizer(net, dict(lr_G=1e-4, beta1=0.9, beta2=0.99, lr_scheme="MultiStepLR", lr_steps=[10],
                                         lr_gamma=0.5))
    loss = TR.optimize_step(net, opt, TR.TimesLoss(TR.CharbonnierLoss()), (x, times, (16, 24)), gt)
    assert math.isfinite(loss) and loss > 0
    unused = ("upconv1.", "upconv2.", "HRconv.", "conv_last.")
    trained = 0
    for k, p in net.named_parameters():
        if k.startswith(unused):
            assert p.grad is None and torch.equal(p.detach(), before[k]), k
            continue
        trained += 1
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
        assert bool(torch.isfinite(p).all()) and not torch.equal(p.detach(), before[k]), k
    assert trained == 434 and len(before) == 442
    assert net.range_status() == 0
