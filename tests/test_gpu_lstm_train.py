"""The trainable BiDeformableConvLSTM and gen_feat on the GPU: stif_lstm_gates_nhwc / _bwd_nhwc, stif_conv1x1_wgrad,
stif_pack_conv1x1_dev, the (2, 256, 256) block weight gradient and the [256, 128] block packs, and train.Conv1x1Cat /
ConvLSTMCell / Easy_PCD / BiDeformableConvLSTM / GenFeat on top of them.

Reference everywhere: torch on the CPU in float64 (tests/lstm_torch_ref.py, pinned to the numpy oracle by
tests/test_lstm_train_host.py).  RTOL = 1e-5 of max |ref| for kernels and single conv modules; every module with a DCN
in it is a cascade here, held to max(2e-5, 4 e32) of max |ref| per tensor, e32 being the error of the same torch
reference run in float32 on the CPU against its float64 run, computed here (the rule of
tests/test_gpu_pcd_train.py).  Every DCN call of every step follows the taming recipe (offsets 0.5 +- 0.3), asserted on
the float64 reference before anything is compared.  GenFeat is also held to the reference's own fixture (tests/golden/model_16x20.npz) with the inference
engine's elementwise bound.

Pixel sets, from the gate kernels' 16 threads per pixel, the 1x1 weight gradient's chunks of 64 pixels and the 3x3
kernel's tile of 2 x 32: 1x1x1, 2x5x7 (one part-filled chunk per item), 1x3x33 (a second chunk), 3x33x70 (111 chunks,
153 tiles), strided items with NaN in the gaps.  Outputs are pre-filled with NaN, the shared workspace too."""
import functools
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lstm_torch_ref as T

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL, RTOL_CASCADE = 1e-5, 2e-5
SHAPES = {"1x1x1": (1, 1, 1), "2x5x7": (2, 5, 7), "1x3x33": (1, 3, 33), "3x33x70": (3, 33, 70), "strided": (2, 5, 7)}
MODES = ["f16x3", "f32"]
MOD_SHAPES = [(1, 5, 7), (2, 12, 20)]
shape_id = lambda s: "x".join(map(str, s))
NAN = float("nan")


def relmax(got, ref):
    ref = torch.as_tensor(ref, dtype=torch.float64).detach()
    return float((got.detach().double().cpu() - ref).abs().max() / ref.abs().max())


def nchw64(t):
    return t.detach().double().cpu().permute(0, 3, 1, 2).contiguous()


def leaf(t):
    return t.detach().clone().requires_grad_(True)


def gpu_leaf(t):
    return t.detach().float().cuda().requires_grad_(True)


def check(name, got, ref, tol):
    e = relmax(got, ref)
    print(f"  {name}: {e:.3e} of max|ref| (tol {tol:.1e})")
    assert e <= tol, (name, e, tol)


def items(t, strided):
    """``t`` [n, ...] on the GPU; strided: every other item of a buffer whose gaps hold NaN."""
    if not strided:
        return t.cuda()
    wide = torch.full((2 * t.shape[0] + 1,) + tuple(t.shape[1:]), NAN)
    wide[1::2] = t
    v = wide.cuda()[1::2]
    assert v.stride(0) == 2 * t[0].numel()
    return v


def nan_out(n, H, W, c, strided):
    return items(torch.full((n, H, W, c), NAN), strided)


def poison_workspace(ops):
    if not ops._WGRAD_WS:
        ops.conv3x3_wgrad(torch.zeros(1, 2, 2, 64, device="cuda"), torch.zeros(1, 2, 2, 64, device="cuda"))
    for ws in ops._WGRAD_WS.values():
        ws.fill_(NAN)


def same_bytes(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---- the gate kernels ----

@functools.lru_cache(maxsize=None)
def gates_case(name, scale=1.0):
    """NHWC float32 inputs and the float64 autograd results: h, c, and per (g_c_next given?) the input gradients."""
    n, H, W = SHAPES[name]
    g = torch.Generator().manual_seed(sorted(SHAPES).index(name) + 40)
    pre, c = torch.randn(n, H, W, 256, generator=g) * scale, torch.randn(n, H, W, 64, generator=g)
    if scale != 1.0:                      # saturated gates: exactly +-30 and +-100 on a quarter of the elements each
        sign = torch.where(pre >= 0, 1.0, -1.0)
        pick = torch.rand(pre.shape, generator=g)
        pre = torch.where(pick < 0.25, 30.0 * sign, torch.where(pick < 0.5, 100.0 * sign, pre))
    gh, gc = torch.randn(n, H, W, 64, generator=g), torch.randn(n, H, W, 64, generator=g)
    ref = {}
    for with_gc in (True, False):
        pr, cr = leaf(nchw64(pre)), leaf(nchw64(c))
        h, cn = T.lstm_gates(pr, cr)
        loss = (h * nchw64(gh)).sum() + ((cn * nchw64(gc)).sum() if with_gc else 0)
        loss.backward()
        ref[with_gc] = (pr.grad, cr.grad)
    ref["h"], ref["c"] = h.detach(), cn.detach()
    return pre, c, gh, gc, ref


def run_gates(ops, name, scale=1.0):
    n, H, W = SHAPES[name]
    st = name == "strided"
    pre, c, gh, gc, ref = gates_case(name, scale)
    pre_d, c_d, gh_d, gc_d = (items(t, st) for t in (pre, c, gh, gc))
    h, cn = ops.lstm_gates(pre_d, c_d, nan_out(n, H, W, 64, st), nan_out(n, H, W, 64, st))
    assert bool(torch.isfinite(h).all()) and bool(torch.isfinite(cn).all())
    check(f"gates {name} h_next", nchw64(h), ref["h"], RTOL)
    check(f"gates {name} c_next", nchw64(cn), ref["c"], RTOL)
    h2, c2 = ops.lstm_gates(pre_d, c_d)                      # fresh outputs: the same bits
    assert torch.equal(h2, h) and torch.equal(c2, cn)
    for with_gc in (True, False):
        g_pre, g_cc = ops.lstm_gates_bwd(pre_d, c_d, gh_d, gc_d if with_gc else None, g_pre=nan_out(n, H, W, 256, st),
                                         g_c_cur=nan_out(n, H, W, 64, st))
        assert bool(torch.isfinite(g_pre).all()) and bool(torch.isfinite(g_cc).all())
        check(f"gates {name} g_pre (g_c_next {with_gc})", nchw64(g_pre), ref[with_gc][0], RTOL)
        check(f"gates {name} g_c_cur (g_c_next {with_gc})", nchw64(g_cc), ref[with_gc][1], RTOL)
        only, none = ops.lstm_gates_bwd(pre_d, c_d, gh_d, gc_d if with_gc else None, need_c=False)
        assert none is None and torch.equal(only, g_pre)     # g_c_cur null: g_pre unchanged
    # g_h null: the gradient of c_next alone
    pr, cr = leaf(nchw64(pre)), leaf(nchw64(c))
    (T.lstm_gates(pr, cr)[1] * nchw64(gc)).sum().backward()
    g_pre, g_cc = ops.lstm_gates_bwd(pre_d, c_d, None, gc_d)
    check(f"gates {name} g_pre (g_h null)", nchw64(g_pre), pr.grad, RTOL)
    check(f"gates {name} g_c_cur (g_h null)", nchw64(g_cc), cr.grad, RTOL)
    o_rows = g_pre[..., 128:192]
    assert float(o_rows.abs().max()) == 0.0                  # the o gate sees g_h only
    with pytest.raises(ValueError, match="both None"):
        ops.lstm_gates_bwd(pre_d, c_d, None, None)


@pytest.mark.parametrize("name", list(SHAPES))
def test_lstm_gates_forward_and_backward_match_autograd(stif, name):
    run_gates(stif.ops, name)


def test_lstm_gates_are_finite_and_right_when_saturated(stif):
    pre = gates_case("3x33x70", 3.0)[0]
    assert float(pre.abs().max()) == 100.0 and int((pre.abs() == 30.0).sum()) > 1000
    run_gates(stif.ops, "3x33x70", 3.0)


@pytest.mark.parametrize("mfma", MODES)
def test_conv_and_gates_against_the_fused_lstm_conv(stif, mfma):
    """EPI_NONE conv + lstm_gates against the inference engine's fused STIF_EPI_LSTM conv on the same weights: RTOL is
    asserted, whether the bits agree is printed."""
    ops, L = stif.ops, stif._lib
    n, H, W = 2, 12, 20
    g = torch.Generator().manual_seed(77)
    x, h, c = (torch.randn(n, H, W, 64, generator=g) for _ in range(3))
    w, b = torch.randn(256, 128, 3, 3, generator=g) / 34, torch.randn(256, generator=g) * 0.1
    f16 = L.PACK_F16X3 if mfma == "f16x3" else 0
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    lay = ops.pack_conv_blocks_dev(w.cuda(), b.cuda(), L.PACK_WINO | f16, status=status)
    pre = torch.full((n, H, W, 256), NAN, device="cuda")
    ops.conv2d([dict(layer=lay, in0=x.cuda(), in1=h.cuda(), out=pre)], in1_mode=1, status=status)
    hn, cn = ops.lstm_gates(pre, c.cuda())
    ref_pre = F.conv2d(torch.cat([nchw64(x), nchw64(h)], 1), w.double(), b.double(), padding=1)
    rh, rc = T.lstm_gates(ref_pre, nchw64(c))
    check(f"pre {mfma}", nchw64(pre), ref_pre, RTOL)
    check(f"h_next {mfma}", nchw64(hn), rh, RTOL)
    check(f"c_next {mfma}", nchw64(cn), rc, RTOL)
    fused = ops.pack_conv(w.numpy(), b.numpy(), L.PACK_WINO_LSTM | f16, device="cuda", range_fallback=False)
    fh, fc = torch.empty(n, H, W, 64, device="cuda"), torch.empty(n, H, W, 64, device="cuda")
    ops.conv2d([dict(layer=fused, in0=x.cuda(), in1=h.cuda(), res=c.cuda(), out=fh, out2=fc)], epi=L.EPI_LSTM,
               in1_mode=1, status=status)
    check(f"fused h_next {mfma}", nchw64(fh), rh, RTOL)
    print(f"  {mfma}: h_next bits equal the fused conv's: {torch.equal(fh, hn)}, c_next: {torch.equal(fc, cn)}; "
          f"max |diff| h {float((fh - hn).abs().max()):.2e} c {float((fc - cn).abs().max()):.2e}")
    assert int(status.item()) == 0


# ---- the 1x1 weight gradient ----

@functools.lru_cache(maxsize=None)
def c1_case(nx, name):
    n, H, W = SHAPES[name]
    g = torch.Generator().manual_seed(sorted(SHAPES).index(name) * 2 + nx + 500)
    xs = [torch.randn(n, H, W, 64, generator=g) for _ in range(nx)]
    gy = torch.randn(n, H, W, 64, generator=g)
    gw = torch.einsum("nhwo,nhwi->oi", gy.double(), torch.cat(xs, 3).double())
    st = name == "strided"
    return [items(x, st) for x in xs], items(gy, st), gw.reshape(64, 64 * nx, 1, 1), gy.double().sum((0, 1, 2))


@pytest.mark.parametrize("name", list(SHAPES))
@pytest.mark.parametrize("nx", [1, 2])
def test_conv1x1_wgrad_matches_fp64(stif, nx, name):
    ops = stif.ops
    xs, gy, gw_ref, gb_ref = c1_case(nx, name)
    poison_workspace(ops)
    gw, gb = ops.conv1x1_wgrad(xs, gy)
    assert tuple(gw.shape) == (64, 64 * nx, 1, 1) and tuple(gb.shape) == (64,)
    assert bool(torch.isfinite(gw).all()) and bool(torch.isfinite(gb).all())
    ew, eb = relmax(gw, gw_ref), relmax(gb, gb_ref)
    print(f"conv1x1_wgrad nx {nx} {name}: gw {ew:.3e} gb {eb:.3e} of max|ref|")
    assert ew <= RTOL and eb <= RTOL, (nx, name, ew, eb)


@pytest.mark.parametrize("nx", [1, 2])
def test_conv1x1_wgrad_integer_inputs_give_the_fp64_bits(stif, nx):
    gen = torch.Generator().manual_seed(79)
    n, H, W = 2, 33, 70
    ints = lambda *s: torch.randint(-3, 4, s, generator=gen).float()
    xs, gy = [ints(n, H, W, 64) for _ in range(nx)], ints(n, H, W, 64)
    gw, gb = stif.ops.conv1x1_wgrad([x.cuda() for x in xs], gy.cuda())
    ref = torch.einsum("nhwo,nhwi->oi", gy.double(), torch.cat(xs, 3).double())
    assert float(ref.abs().max()) < 2 ** 24
    assert torch.equal(gw.double().cpu().reshape(64, 64 * nx), ref)
    assert torch.equal(gb.double().cpu(), gy.double().sum((0, 1, 2)))


@pytest.mark.parametrize("nx", [1, 2])
def test_conv1x1_wgrad_repeats_are_bit_identical(stif, nx):
    ops = stif.ops
    xs, gy, _, _ = c1_case(nx, "3x33x70")
    first = ops.conv1x1_wgrad(xs, gy)
    other = c1_case(3 - nx, "2x5x7")
    ops.conv1x1_wgrad(other[0], other[1])                     # another shape in between
    poison_workspace(ops)
    again = ops.conv1x1_wgrad(xs, gy)
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])


# ---- the 1x1 packer ----

def c1_weights(sd, kind):
    if kind == "state-dict":
        return torch.from_numpy(sd["fusion.weight"]), torch.from_numpy(sd["fusion.bias"])
    g = torch.Generator().manual_seed(192)
    return torch.randn(64, 128, 1, 1, generator=g), torch.randn(64, generator=g)


@pytest.mark.parametrize("kind", ["random", "state-dict"])
@pytest.mark.parametrize("mfma", MODES)
def test_conv1x1_packs_are_the_host_packers_bytes(stif, sd, mfma, kind):
    ops, L = stif.ops, stif._lib
    mode = L.PACK_PLAIN | (L.PACK_F16X3 if mfma == "f16x3" else 0)
    w, b = c1_weights(sd, kind)
    assert tuple(w.shape) == (64, 128, 1, 1)
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    lay = ops.pack_conv1x1_dev(w.cuda(), b.cuda(), mode, status=status)
    host = ops.pack_conv(w.numpy(), b.numpy(), mode, device="cuda", range_fallback=False)
    assert lay.w.numel() == L.lib().stif_conv_weight_floats(64, 128, 1, mode)
    assert same_bytes(lay.w, host.w) and same_bytes(lay.b, host.b)
    assert (lay.cout, lay.cin, lay.ks, lay.mode) == (64, 128, 1, mode) and int(status.item()) == 0
    for half in (0, 1):     # the DGRAD halves: the host pack of the transposed slice, zero bias
        d = ops.pack_conv1x1_dev(w.cuda(), None, L.PACK_PLAIN, dgrad=True, half=half)
        wt = w[:, 64 * half:64 * half + 64, 0, 0].t().contiguous().reshape(64, 64, 1, 1)
        ht = ops.pack_conv(wt.numpy(), np.zeros(64, np.float32), L.PACK_PLAIN, device="cuda")
        assert (d.cout, d.cin, d.ks, d.mode) == (64, 64, 1, L.PACK_PLAIN)
        assert same_bytes(d.w, ht.w) and same_bytes(d.b, ht.b), half
    with pytest.raises(ValueError, match="no form"):
        ops.pack_conv1x1_dev(w.cuda(), None, L.PACK_PLAIN, dgrad=True)
    with pytest.raises(ValueError, match="no form"):
        ops.pack_conv1x1_dev(w.cuda(), b.cuda(), L.PACK_PLAIN, half=1)


def test_conv1x1_packer_reports_a_weight_outside_the_split_range(stif):
    ops, L = stif.ops, stif._lib
    w = torch.zeros(64, 128, 1, 1)
    w[40, 100] = 100.0
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    ops.pack_conv1x1_dev(w.cuda(), torch.zeros(64).cuda(), L.PACK_PLAIN | L.PACK_F16X3, status=status)
    assert int(status.item()) == L.STATUS_PACK_RANGE
    with pytest.raises(stif._lib.StifError):                  # where the host packer returns STIF_E_RANGE
        ops.pack_conv(w.numpy(), np.zeros(64, np.float32), L.PACK_PLAIN | L.PACK_F16X3, range_fallback=False)
    status.zero_()
    ops.pack_conv1x1_dev(w.cuda(), torch.zeros(64).cuda(), L.PACK_PLAIN, status=status)          # fp32: no range
    ops.pack_conv1x1_dev(w.cuda(), None, L.PACK_PLAIN, dgrad=True, half=1, status=status)
    w[40, 100] = 63.0
    ops.pack_conv1x1_dev(w.cuda(), torch.zeros(64).cuda(), L.PACK_PLAIN | L.PACK_F16X3, status=status)
    assert int(status.item()) == 0


# ---- the (2, 256, 256) weight gradient and the [256, 128] block packs ----

@functools.lru_cache(maxsize=None)
def cell_wg_case(name):
    n, H, W = SHAPES[name]
    g = torch.Generator().manual_seed(sorted(SHAPES).index(name) + 700)
    xs = [torch.randn(n, H, W, 64, generator=g) for _ in range(2)]
    gy = torch.randn(n, H, W, 256, generator=g)
    gw = torch.nn.grad.conv2d_weight(torch.cat([nchw64(x) for x in xs], 1), (256, 128, 3, 3), nchw64(gy), padding=1)
    st = name == "strided"
    return [items(x, st) for x in xs], items(gy, st), gw, gy.double().sum((0, 1, 2))


@pytest.mark.parametrize("name", list(SHAPES))
def test_cell_wgrad_matches_fp64_and_the_64_to_64_kernel(stif, name):
    ops = stif.ops
    xs, gy, gw_ref, gb_ref = cell_wg_case(name)
    poison_workspace(ops)
    gw, gb = ops.conv3x3_wgrad_cat(xs, gy, 256)
    assert tuple(gw.shape) == (256, 128, 3, 3) and tuple(gb.shape) == (256,)
    assert bool(torch.isfinite(gw).all()) and bool(torch.isfinite(gb).all())
    ew, eb = relmax(gw, gw_ref), relmax(gb, gb_ref)
    print(f"wgrad_cat cell {name}: gw {ew:.3e} gb {eb:.3e} of max|ref|")
    assert ew <= RTOL and eb <= RTOL, (name, ew, eb)
    for s in range(4):      # block for block the bits of the 64 -> 64 kernel on the contiguous slices
        gs = gy[..., 64 * s:64 * s + 64].contiguous()
        for i, x in enumerate(xs):
            bw, bb = ops.conv3x3_wgrad(x, gs)
            assert torch.equal(gw[64 * s:64 * s + 64, 64 * i:64 * i + 64], bw), (name, s, i)
            assert torch.equal(gb[64 * s:64 * s + 64], bb), (name, s, i)
    again = ops.conv3x3_wgrad_cat(xs, gy, 256)
    assert torch.equal(again[0], gw) and torch.equal(again[1], gb)


@pytest.mark.parametrize("kind", ["random", "state-dict"])
@pytest.mark.parametrize("mfma", MODES)
def test_cell_block_packs_are_the_host_packers_bytes(stif, sd, mfma, kind):
    ops, L = stif.ops, stif._lib
    mode = L.PACK_WINO | (L.PACK_F16X3 if mfma == "f16x3" else 0)
    if kind == "state-dict":
        name = "ConvBLSTM.forward_net.cell_list.0.conv"
        w, b = torch.from_numpy(sd[name + ".weight"]), torch.from_numpy(sd[name + ".bias"])
    else:
        g = torch.Generator().manual_seed(384)
        w, b = torch.randn(256, 128, 3, 3, generator=g), torch.randn(256, generator=g)
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    lay = ops.pack_conv_blocks_dev(w.cuda(), b.cuda(), mode, status=status)
    host = ops.pack_conv(w.numpy(), b.numpy(), mode, device="cuda", range_fallback=False)
    assert lay.w.numel() == L.lib().stif_conv_weight_floats(256, 128, 3, mode)
    assert same_bytes(lay.w, host.w) and same_bytes(lay.b, host.b)
    assert (lay.cout, lay.cin, lay.ks, lay.mode) == (256, 128, 3, mode)
    per = lay.w.numel() // 8
    for half in (0, 1):     # dgrad: four DGRAD packs of the contiguous 64 x 64 slices, end to end
        d = ops.pack_conv_blocks_dev(w.cuda(), None, mode, dgrad=True, half=half, status=status)
        assert (d.cout, d.cin) == (64, 256) and d.w.numel() == 4 * per and float(d.b.abs().max()) == 0.0
        for s in range(4):
            one = ops.pack_conv_dev(w[64 * s:64 * s + 64, 64 * half:64 * half + 64].contiguous().cuda(), None, mode,
                                    dgrad=True, status=status)
            assert same_bytes(d.w[s * per:(s + 1) * per], one.w), (half, s)
    assert int(status.item()) == 0
    with pytest.raises(ValueError, match="no block form"):
        ops.pack_conv_blocks_dev(w.cuda(), None, mode, dgrad=True)
    with pytest.raises(ValueError, match="no block form"):
        ops.pack_conv_blocks_dev(w.cuda(), b.cuda(), mode, half=0)


# ---- the single modules ----

@pytest.mark.parametrize("mfma", MODES)
@pytest.mark.parametrize("shape", MOD_SHAPES, ids=shape_id)
def test_conv1x1cat_module(stif, shape, mfma):
    n, h, w = shape
    g = torch.Generator().manual_seed(h * w + 1)
    rnd = lambda *s: torch.randn(*s, generator=g).double()
    a, b, gout = rnd(n, 64, h, w), rnd(n, 64, h, w), rnd(n, 64, h, w)
    torch.manual_seed(1)
    m = stif.train.Conv1x1Cat(mfma)
    ar, br, wr, biasr = leaf(a), leaf(b), leaf(m.weight.double()), leaf(m.bias.double())
    ref = F.conv2d(torch.cat([ar, br], 1), wr, biasr)
    ref.backward(gout)
    m = m.cuda()
    ag, bg = gpu_leaf(a), gpu_leaf(b)
    out = m(ag, bg)
    out.backward(gout.float().cuda())
    assert tuple(out.shape) == (n, 64, h, w)
    check("out", out, ref, RTOL)
    for name, got, want in (("ga", ag.grad, ar.grad), ("gb", bg.grad, br.grad), ("gw", m.weight.grad, wr.grad),
                            ("gbias", m.bias.grad, biasr.grad)):
        check(name, got, want, RTOL)
    assert m.range_status() == 0
    # only the gradients that are asked for are computed
    bg2 = gpu_leaf(b)
    m.zero_grad()
    m.weight.requires_grad_(False)
    m(a.float().cuda(), bg2).backward(gout.float().cuda())
    assert m.weight.grad is None and torch.equal(bg2.grad, bg.grad) and m.bias.grad is not None


@pytest.mark.parametrize("mfma", MODES)
@pytest.mark.parametrize("shape", MOD_SHAPES, ids=shape_id)
def test_convlstm_cell_module(stif, shape, mfma):
    n, hh, ww = shape
    g = torch.Generator().manual_seed(hh * ww + 2)
    rnd = lambda *s: torch.randn(*s, generator=g).double()
    x, h, c, g_h, g_c = (rnd(n, 64, hh, ww) for _ in range(5))
    torch.manual_seed(2)
    m = stif.train.ConvLSTMCell(mfma)
    with torch.no_grad():
        m.conv.weight.mul_(3.0)             # pre-activations of order 1: the gates leave their linear range
    P = {"conv.weight": leaf(m.conv.weight.double()), "conv.bias": leaf(m.conv.bias.double())}
    xr, hr, cr = leaf(x), leaf(h), leaf(c)
    rh, rc = T.conv_lstm_cell(P, "", xr, hr, cr)
    ((rh * g_h).sum() + (rc * g_c).sum()).backward()
    m = m.cuda()
    xg, hg, cg = gpu_leaf(x), gpu_leaf(h), gpu_leaf(c)
    oh, oc = m(xg, (hg, cg))
    torch.autograd.backward([oh, oc], [g_h.float().cuda(), g_c.float().cuda()])
    assert tuple(oh.shape) == (n, 64, hh, ww) and tuple(oc.shape) == (n, 64, hh, ww)
    check("h_next", oh, rh, RTOL)
    check("c_next", oc, rc, RTOL)
    for name, got, want in (("gx", xg.grad, xr.grad), ("gh", hg.grad, hr.grad), ("gc", cg.grad, cr.grad),
                            ("gw", m.conv.weight.grad, P["conv.weight"].grad),
                            ("gbias", m.conv.bias.grad, P["conv.bias"].grad)):
        check(name, got, want, RTOL)
    assert m.range_status() == 0
    # c_next without a consumer (the last step), and only the gradients that are asked for
    P2 = {k: leaf(v) for k, v in P.items()}
    hr2 = leaf(h)
    (T.conv_lstm_cell(P2, "", x, hr2, c)[0] * g_h).sum().backward()
    hg2 = gpu_leaf(h)
    m.zero_grad()
    m.conv.weight.requires_grad_(False)
    m(x.float().cuda(), (hg2, c.float().cuda()))[0].backward(g_h.float().cuda())
    assert m.conv.weight.grad is None
    check("gh (h_next only)", hg2.grad, hr2.grad, RTOL)
    check("gbias (h_next only)", m.conv.bias.grad, P2["conv.bias"].grad, RTOL)


# ---- the cascades ----

def cascade(tag, got, ref, e32, kinds):
    assert sorted(got) == sorted(ref), sorted(set(got) ^ set(ref))
    ratios = {}
    for k in ref:
        assert got[k] is not None, k
        tol = max(RTOL_CASCADE, 4 * e32[k])
        e = relmax(got[k], ref[k])
        ratios[k] = (e / tol, e, e32[k])
    for kind in kinds:
        ks = [k for k in ratios if kind in k]
        k = max(ks, key=lambda q: ratios[q][0])
        print(f"  {tag} worst {kind}: {k} err {ratios[k][1]:.3e} e32 {ratios[k][2]:.3e} ratio {ratios[k][0]:.3f}")
    bad = {k: v for k, v in ratios.items() if v[0] > 1.0}
    assert not bad, bad


def both_precisions(P, inputs, fn, gout):
    """The float64 results of ``fn(P, *inputs)`` with every gradient, and e32 per tensor (float32 against float64)."""
    res = {}
    for dt in (torch.float64, torch.float32):
        Pl = {k: leaf(v.to(dt)) for k, v in P.items()}
        ins = [leaf(t.to(dt)) for t in inputs]
        out = fn(Pl, *ins)
        out.backward(gout.to(dt))
        q = {"out": out.detach()}
        q.update({"g_" + k: v.grad for k, v in Pl.items()})
        q.update({f"g_in{i}": t.grad for i, t in enumerate(ins)})
        res[dt] = q
    ref = res[torch.float64]
    return ref, {k: relmax(res[torch.float32][k], ref[k]) for k in ref}


@functools.lru_cache(maxsize=None)
def easy_pcd_case(shape):
    B, H, W = shape
    g = torch.Generator().manual_seed(B * H + W + 60)
    f1, f2 = (torch.randn(B, 64, H, W, generator=g, dtype=torch.float64) for _ in range(2))
    gout = torch.randn(B, 64, H, W, generator=g, dtype=torch.float64)
    P = T.random_params(T.easy_pcd_shapes(), B + H + 60)
    run = lambda calls: T.easy_pcd(P, "", f1, f2, calls)
    T.tame_recurrence(P, run)
    T.assert_all_tame(P, run)
    ref, e32 = both_precisions(P, (f1, f2), lambda Pl, a, b: T.easy_pcd(Pl, "", a, b), gout)
    return f1, f2, P, gout, ref, e32


KINDS = ("out", "g_in", "conv_offset_mask.weight", "conv_offset_mask.bias", "dcnpack", "offset_conv", "fea_conv",
         "fea_L", "fusion")


@pytest.mark.parametrize("mfma", MODES)
@pytest.mark.parametrize("shape", [(1, 8, 12), (2, 12, 20)], ids=shape_id)
def test_easy_pcd_output_and_every_gradient(stif, shape, mfma):
    f1, f2, P, gout, ref, e32 = easy_pcd_case(shape)
    net = stif.train.Easy_PCD(mfma)
    net.load_state_dict({k: v.float() for k, v in P.items()}, strict=True)
    net = net.cuda()
    a, b = gpu_leaf(f1), gpu_leaf(f2)
    out = net(a, b)
    assert tuple(out.shape) == (shape[0], 64, shape[1], shape[2])
    out.backward(gout.float().cuda())
    got = {"out": out, "g_in0": a.grad, "g_in1": b.grad}
    got.update({"g_" + k: p.grad for k, p in net.named_parameters()})
    assert len(ref) == 1 + 74 + 2
    cascade(f"easy_pcd {shape_id(shape)} {mfma}", got, ref, e32, KINDS)
    assert net.range_status() == 0


@functools.lru_cache(maxsize=None)
def bilstm_case(shape):
    B, Tn, H, W = shape
    g = torch.Generator().manual_seed(B * Tn + H + W + 80)
    x = torch.randn(B, Tn, 64, H, W, generator=g, dtype=torch.float64)
    gout = torch.randn(B, Tn, 64, H, W, generator=g, dtype=torch.float64)
    P = T.random_params(T.bilstm_shapes(""), B + Tn + 80)
    fn = lambda Pl, xs, calls=None: torch.stack(T.bi_convlstm(Pl, list(xs.unbind(1)), calls, p=""), 1)
    run = lambda calls: fn(P, x, calls)
    T.tame_recurrence(P, run)
    calls = T.assert_all_tame(P, run)
    assert len(calls) == 12 and all(len(v) == 2 * Tn for v in calls.values())
    ref, e32 = both_precisions(P, (x,), fn, gout)
    return x, P, gout, ref, e32


@pytest.mark.parametrize("mfma", MODES)
@pytest.mark.parametrize("shape", [(1, 2, 8, 12), (2, 3, 8, 12)], ids=shape_id)
def test_bilstm_output_and_every_gradient(stif, shape, mfma):
    x, P, gout, ref, e32 = bilstm_case(shape)
    spec = json.load(open(os.path.join(REPO, "tests", "golden", "state_dict_spec.json")))
    assert sorted(P) == sorted(k[len("ConvBLSTM."):] for k, _ in spec if k.startswith("ConvBLSTM."))
    assert len(P) == 2 * 74 + 4 and len(ref) == len(P) + 2
    net = stif.train.BiDeformableConvLSTM(mfma)
    net.load_state_dict({k: v.float() for k, v in P.items()}, strict=True)
    net = net.cuda()
    xg = gpu_leaf(x)
    out = net(xg)
    assert tuple(out.shape) == tuple(x.shape)
    out.backward(gout.float().cuda())
    got = {"out": out, "g_in0": xg.grad}
    got.update({"g_" + k: p.grad for k, p in net.named_parameters()})
    cascade(f"bilstm {shape_id(shape)} {mfma}", got, ref, e32, KINDS + ("cell_list", "conv_1x1"))
    assert net.range_status() == 0


# ---- against the reference's own fixture ----

def close(a, b, rtol=1e-4, atol=1e-6):
    """(ok, max |a - b|, worst ratio of |a - b| to its elementwise bound): the inference engine's yardstick"""
    a, b = a.detach().cpu().numpy().astype(np.float64), np.asarray(b, np.float64)
    d, lim = np.abs(a - b), rtol * np.abs(b) + atol
    return bool((d <= lim).all()), float(d.max()), float((d / lim).max())


def test_gen_feat_matches_the_reference_fixture(stif, sd, golden):
    TR = stif.train
    gm = golden["model_16x20"]
    net = TR.GenFeat(5, 40)
    net.load_state_dict(TR.gen_feat_state_dict(sd), strict=True)
    net = net.cuda()
    seen = {}

    def first(name):
        def hook(_m, _i, out):
            seen.setdefault(name, out)
        return hook

    net.ConvBLSTM.forward_net.pcd_h.register_forward_hook(first("pcd_h_t0"))
    net.ConvBLSTM.forward_net.cell_list[0].register_forward_hook(first("cell_t0"))
    net.ConvBLSTM.register_forward_hook(first("bilstm"))
    net.fusion.register_forward_hook(first("fusion"))
    with torch.no_grad():
        feat = net(torch.from_numpy(gm["x"]).cuda())
    assert tuple(feat.shape) == (1, 3, 64, 16, 20)
    pairs = [("pcd_h_t0", seen["pcd_h_t0"][0], gm["pcd_h_t0"]), ("cell_h_t0", seen["cell_t0"][0][0], gm["cell_h_t0"]),
             ("cell_c_t0", seen["cell_t0"][1][0], gm["cell_c_t0"]), ("bilstm", seen["bilstm"][0], gm["bilstm"]),
             ("fusion", seen["fusion"][0], gm["fusion"]), ("feat", feat[0], gm["feat"])]
    results = {name: close(got, want) for name, got, want in pairs}
    for name, (ok, err, ratio) in results.items():
        print(f"  {name}: max err {err:.3e}, worst ratio to the elementwise bound {ratio:.3f}")
    assert all(ok for ok, _, _ in results.values()), results
    assert net.range_status() == 0


# ---- one optimiser step ----

def test_one_optimiser_step_through_gen_feat(stif):
    TR = stif.train
    torch.manual_seed(5)
    net = TR.GenFeat(front_RBs=1, back_RBs=1).cuda()
    with torch.no_grad():        # the zero-initialised offset convs would leave their inputs without a gradient
        for m in net.modules():
            if isinstance(m, TR.DCN_sep):
                m.conv_offset_mask.weight.normal_(0, 0.01)
    g = torch.Generator().manual_seed(6)
    x, gt = torch.rand(1, 2, 3, 16, 24, generator=g).cuda(), torch.rand(1, 3, 64, 16, 24, generator=g).cuda()
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    crit = TR.CharbonnierLoss()
    first = TR.optimize_step(net, opt, crit, (x,), gt)
    grads = {k: p.grad for k, p in net.named_parameters()}
    assert len(grads) == len(T.gen_feat_shapes(1, 1))
    assert all(v is not None and bool(torch.isfinite(v).all()) for v in grads.values())
    for k in ("ConvBLSTM.forward_net.cell_list.0.conv.weight", "ConvBLSTM.conv_1x1.weight",
              "ConvBLSTM.forward_net.pcd_c.fusion.weight", "fusion.weight", "conv_first.weight"):
        assert float(grads[k].abs().max()) > 0, k
    with torch.no_grad():
        second = float(crit(net(x), gt))
    print(f"  loss {first:.4f} -> {second:.4f}")
    assert second < first
    assert net.range_status() == 0
