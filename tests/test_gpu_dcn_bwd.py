"""The native NHWC backward of the deformable conv on the GPU: stif_dcn_bwd_nhwc (k_dcn_bwd_data, k_dcn_bwd_w),
stif_dcn_offmask_nhwc, ops.dcn_bwd / ops.dcn_offmask and the rewired train.DCN_sep.

References: the deformable conv of tests/pcd_torch_ref.py in float64 under autograd (pinned to the numpy oracle by
tests/test_pcd_train_host.py), with g_om assembled from its grad_offset / grad_mask; and, for offsets that land on
and around integers, where bilinear sampling has no unique gradient, the drop-in ops.dcn_v2_backward on the same
tensors (pinned to the oracle by tests/test_gpu_ops.py), which computes every position as the same fp32 sum and takes
its corners from the same header, so both branch alike.  RTOL_DCN = 2e-5 of max |ref|.

Shapes, from the kernels' tiles -- 4 x 32 pixels for the data kernel, 2 x 32 for the weight kernel, whose persistent
grid is G = min(tiles, 2 per CU): 1x1x1; 2x5x7 (inside one data tile, three weight tiles per item); 1x3x33 and 3x33x70
(partial tiles on both axes, several items); 2x5x7 with every map's item stride larger than dense; 2x192x192 (1152
weight tiles, more than workgroups), compared with the drop-in only.  The exactness runs use inputs whose every
reference value is a small dyadic rational, so that fp32 sums are exact in any order and torch.equal is the check, with
the workspace, g_in and g_om filled with NaN first."""
import ctypes as C
import functools

import pytest
import torch

import pcd_torch_ref as R

pytestmark = pytest.mark.gpu

RTOL_DCN = 2e-5
NAN = float("nan")
GEOM = (3, 3, 1, 1, 1, 1, 1, 1, 8)
SMALL = {"1x1x1": (1, 1, 1), "2x5x7": (2, 5, 7), "1x3x33": (1, 3, 33), "3x33x70": (3, 33, 70), "strided": (2, 5, 7)}
PAD = {"strided": 36}     # floats between items beyond the dense size (a multiple of 4), on every map
OUTS = ("g_in", "g_om", "g_w", "g_b")


def relmax(got, ref):
    ref = ref.detach().double().cpu()
    return float((got.detach().double().cpu() - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


def same_bytes(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def to_offmask(offset, mask):
    """offset [n, 144, H, W] + mask [n, 72, H, W] (reference row order) -> [n, H, W, 216] = [group][tap][dy, dx, m]"""
    n, _, H, W = offset.shape
    om = torch.cat([offset.reshape(n, 8, 9, 2, H, W), mask.reshape(n, 8, 9, 1, H, W)], 3)
    return om.permute(0, 4, 5, 1, 2, 3).reshape(n, H, W, 216).contiguous()


def to_g_om(g_offset, g_mask, mask):
    """[grad_offset | grad_mask * m (1 - m) | 0] as NHWC [n, H, W, 256]"""
    n, _, H, W = g_offset.shape
    pad = torch.zeros(n, 40, H, W, dtype=g_offset.dtype, device=g_offset.device)
    return nhwc(torch.cat([g_offset, g_mask * mask * (1.0 - mask), pad], 1))


def reference(inp, offset, mask, weight, gout, lrelu):
    """float64 autograd through pcd_torch_ref.dcn: (out, {g_in, g_om, g_w, g_b}) in the kernel's layouts"""
    leaves = [t.double().clone().requires_grad_(True) for t in (inp, offset, mask, weight)]
    bias = torch.zeros(64, dtype=torch.float64, requires_grad=True)
    out = R.dcn(*leaves, bias)
    if lrelu:
        out = R.lrelu(out)
    out.backward(gout.double())
    gi, go, gm, gw = (t.grad for t in leaves)
    return out.detach(), {"g_in": nhwc(gi), "g_om": to_g_om(go, gm, mask.double()), "g_w": gw, "g_b": bias.grad}


def exact_inputs(shape, seed):
    n, H, W = shape
    g = torch.Generator().manual_seed(seed)
    ints = lambda *s: torch.randint(-3, 4, s, generator=g).double()
    inp, weight, gout = ints(n, 64, H, W), ints(64, 64, 3, 3), ints(n, 64, H, W)
    # multiples of 0.5 in [-2.5, 2.5]: zero (the fresh module's offsets) and other integers included; border pixels
    # reach the bands (-1, 0) and (H - 1, H) with them
    offset = torch.randint(-5, 6, (n, 144, H, W), generator=g).double() * 0.5
    far = torch.rand(n, 144, H, W, generator=g)
    offset[far < 0.03] = 1e4
    offset[far > 0.97] = -1e4
    mask = torch.randint(0, 5, (n, 72, H, W), generator=g).double() * 0.25
    return inp, offset, mask, weight, gout


@functools.lru_cache(maxsize=None)
def exact_case(name):
    t = exact_inputs(SMALL[name], 11 + len(name))
    inp, offset, mask, weight, gout = t
    H, W = inp.shape[2:]
    pos = offset.reshape(-1, 8, 9, 2, H, W)[:, :, :, 0] + torch.arange(H).view(1, 1, 1, H, 1)
    assert float(offset.abs().min()) == 0.0 and float(offset.abs().max()) == 1e4
    if H > 1:   # every band of rows is sampled: (-1, 0), on the grid, (H - 1, H)
        rows = pos - 1 + (torch.arange(9) // 3).view(1, 1, 9, 1, 1)
        assert bool(((rows > -1) & (rows < 0)).any()) and bool(((rows > H - 1) & (rows < H)).any())
        assert bool((rows == rows.round()).any())
    _, ref = reference(*t, lrelu=False)
    return t, ref


class Maps:
    """The NHWC device tensors of one call, each item `pad` floats past dense, and NaN-filled outputs."""

    def __init__(self, inp, offset, mask, weight, gout, out=None, pad=0):
        self.n, _, self.H, self.W = inp.shape
        self.pad = pad
        self.inp, self.in_item = self.place(nhwc(inp.float()))
        self.offmask, self.om_item = self.place(to_offmask(offset.float(), mask.float()))
        self.gout, self.gout_item = self.place(nhwc(gout.float()))
        self.out, self.out_item = self.place(nhwc(out.float())) if out is not None else (None, 0)
        self.weight = weight.float().cuda().contiguous()

    def place(self, t):
        n, H, W, c = t.shape
        full = torch.full((n, H * W * c + self.pad), NAN, device="cuda")
        view = full[:, :H * W * c].view(n, H, W, c)
        view.copy_(t)
        return view, H * W * c + self.pad

    def empty(self, c):
        return self.place(torch.full((self.n, self.H, self.W, c), NAN))


def call(stif, m, need=(True, True, True), lrelu=False, with_gb=True):
    """stif_dcn_bwd_nhwc through the C ABI on NaN-filled (and, with m.pad, strided) outputs; the workspace is the
    shared one, filled with NaN first.  Returns {name: tensor or None} and the workspace."""
    L, ops = stif._lib, stif.ops
    a = L.DcnBwdArgs()
    a.inp, a.offmask, a.w, a.gout = m.inp.data_ptr(), m.offmask.data_ptr(), m.weight.data_ptr(), m.gout.data_ptr()
    a.in_item, a.om_item, a.gout_item = m.in_item, m.om_item, m.gout_item
    if lrelu:
        a.out, a.out_item, a.epi = m.out.data_ptr(), m.out_item, L.EPI_LRELU
    got = dict.fromkeys(OUTS)
    if need[0]:
        got["g_in"], a.gin_item = m.empty(64)
        a.g_in = got["g_in"].data_ptr()
    if need[1]:
        got["g_om"], a.gom_item = m.empty(256)
        a.g_om = got["g_om"].data_ptr()
    ws, stream = ops._wgrad_workspace(m.inp.device, L.lib().stif_dcn_bwd_workspace_size(m.n, m.H, m.W))
    ws.fill_(NAN)
    if need[2]:
        got["g_w"] = torch.full((64, 64, 3, 3), NAN, device="cuda")
        a.g_w, a.workspace, a.workspace_bytes = got["g_w"].data_ptr(), ws.data_ptr(), ws.numel() * 4
        if with_gb:
            got["g_b"] = torch.full((64,), NAN, device="cuda")
            a.g_b = got["g_b"].data_ptr()
    a.n, a.H, a.W = m.n, m.H, m.W
    L.check(L.lib().stif_dcn_bwd_nhwc(C.byref(a), stream), "stif_dcn_bwd_nhwc")
    torch.cuda.synchronize()
    return got, ws


# ---- exactness ----

@pytest.mark.parametrize("name", list(SMALL))
def test_exact_inputs_give_the_reference_bit_for_bit(stif, name):
    t, ref = exact_case(name)
    for k in OUTS:   # an input bug, not a tolerance case
        assert torch.equal(ref[k].float().double(), ref[k]), k
        assert float(ref[k].abs().max()) > 0, k
    got, _ = call(stif, Maps(*t, pad=PAD.get(name, 0)))
    for k in OUTS:
        assert torch.equal(got[k].cpu().double(), ref[k]), (k, relmax(got[k], ref[k]))


# ---- real inputs ----

@functools.lru_cache(maxsize=None)
def tame_case(name):
    n, H, W = SMALL[name]
    g = torch.Generator().manual_seed(5 + n * H + W)
    rnd = lambda *s: torch.randn(*s, generator=g).double()
    inp, fea, gout, weight = rnd(n, 64, H, W), rnd(n, 64, H, W), rnd(n, 64, H, W), rnd(64, 64, 3, 3) / 24
    w_om, b_om = rnd(216, 64, 3, 3) / 24, rnd(216) * 0.1
    R.tame_dcn(w_om, b_om, fea)
    offset, mask = R.offset_mask(fea, w_om, b_om)
    R.assert_offsets_tame(offset)
    t = (inp, offset, mask, weight, gout)
    return t, {lrelu: reference(*t, lrelu=lrelu) for lrelu in (False, True)}


@pytest.mark.parametrize("lrelu", [False, True], ids=["none", "lrelu"])
@pytest.mark.parametrize("name", list(SMALL))
def test_tamed_inputs_against_float64(stif, name, lrelu):
    t, refs = tame_case(name)
    out, ref = refs[lrelu]
    got, _ = call(stif, Maps(*t, out=out if lrelu else None, pad=PAD.get(name, 0)), lrelu=lrelu)
    errs = {k: relmax(got[k], ref[k]) for k in OUTS}
    print(name, lrelu, errs)
    for k in OUTS:
        assert errs[k] <= RTOL_DCN, (k, errs)
    assert float(got["g_om"][..., 216:].abs().max()) == 0.0


def wild_inputs(shape, seed):
    n, H, W = shape
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g)
    inp, gout, weight = rnd(n, 64, H, W), rnd(n, 64, H, W), rnd(64, 64, 3, 3) / 24
    offset = rnd(n, 144, H, W) * 3
    pick = torch.rand(n, 144, H, W, generator=g)
    offset = torch.where(pick < 0.05, offset.round(), offset)                       # exactly on the grid
    offset = torch.where(pick > 0.97, offset + torch.sign(offset) * (H + W), offset)   # beyond the frame
    mask = torch.sigmoid(rnd(n, 72, H, W))
    return inp, offset, mask, weight, gout


@pytest.mark.parametrize("shape", [(3, 33, 70), (2, 192, 192)], ids=["3x33x70", "2x192x192"])
def test_wild_offsets_against_the_drop_in(stif, shape):
    ops = stif.ops
    inp, offset, mask, weight, gout = (t.cuda() for t in wild_inputs(shape, 3 + shape[1]))
    bias = torch.zeros(64, device="cuda")
    gi, go, gm, gw, gb = ops.dcn_v2_backward(inp, weight, bias, offset, mask, gout, *GEOM)
    ref = {"g_in": nhwc(gi), "g_om": to_g_om(go, gm, mask), "g_w": gw, "g_b": gb}
    got = dict(zip(OUTS, ops.dcn_bwd(nhwc(inp), to_offmask(offset, mask), weight, nhwc(gout))))
    errs = {k: relmax(got[k], ref[k]) for k in OUTS}
    print(shape, errs)
    for k in OUTS:
        assert errs[k] <= RTOL_DCN, (k, errs)


def test_repeated_calls_give_identical_bits_except_g_in(stif):
    t, refs = tame_case("3x33x70")
    m = Maps(*t)
    first, _ = call(stif, m)
    second, _ = call(stif, m)
    for k in ("g_om", "g_w", "g_b"):
        assert same_bytes(first[k], second[k]), k
    assert relmax(second["g_in"], refs[False][1]["g_in"]) <= RTOL_DCN


NEEDS = [(i, o, w) for i in (True, False) for o in (True, False) for w in (True, False) if i or o or w]


@pytest.mark.parametrize("need", NEEDS, ids=lambda n: "".join("iow"[k] if v else "-" for k, v in enumerate(n)))
def test_null_outputs_skip_their_work(stif, need):
    t, refs = tame_case("1x3x33")
    out, ref = refs[True]
    m = Maps(*t, out=out)
    full, _ = call(stif, m, lrelu=True)
    got, ws = call(stif, m, need=need, lrelu=True)
    for k, wanted in zip(OUTS, (need[0], need[1], need[2], need[2])):
        if not wanted:
            assert got[k] is None
        elif k == "g_in":
            assert relmax(got[k], ref[k]) <= RTOL_DCN
        else:
            assert same_bytes(got[k], full[k]), k
    if not need[2]:                 # no weight kernel: the workspace keeps its NaN
        assert bool(torch.isnan(ws).all())
    else:                           # g_b is optional beside g_w
        alone, _ = call(stif, m, need=need, lrelu=True, with_gb=False)
        assert alone["g_b"] is None and same_bytes(alone["g_w"], full["g_w"])
    py = stif.ops.dcn_bwd(m.inp, m.offmask, m.weight, m.gout, out=m.out, epi=stif._lib.EPI_LRELU, need=need)
    for k, v, wanted in zip(OUTS, py, (need[0], need[1], need[2], need[2])):
        assert (v is not None) == wanted, k
        if wanted and k != "g_in":
            assert same_bytes(v, full[k]), k


# ---- the bridge and the forward ----

@pytest.mark.parametrize("name", list(SMALL) + ["2x192x192"])
def test_dcn_offmask(stif, name):
    n, H, W = SMALL.get(name, (2, 192, 192))
    pad = PAD.get(name, 0)
    g = torch.Generator().manual_seed(n + H + W)
    om = torch.randn(n, H, W, 256, generator=g) * 4
    om[..., 216:] = NAN                                     # never read
    src = torch.full((n, H * W * 256 + pad), NAN, device="cuda")
    src_v = src[:, :H * W * 256].view(n, H, W, 256)
    src_v.copy_(om)
    dst = torch.full((n, H * W * 216 + pad), NAN, device="cuda")
    dst_v = dst[:, :H * W * 216].view(n, H, W, 216)
    assert stif.ops.dcn_offmask(src_v, out=dst_v) is dst_v
    got = dst_v.cpu().view(n, H, W, 8, 9, 3)
    off = om[..., :144].reshape(n, H, W, 8, 9, 2)
    assert same_bytes(got[..., :2], off)
    ref = torch.sigmoid(om[..., 144:216].double()).reshape(n, H, W, 8, 9)
    assert float((got[..., 2].double() - ref).abs().max()) <= 1e-5
    if pad:
        assert bool(torch.isnan(dst[:, H * W * 216:]).all())
    fresh = stif.ops.dcn_offmask(src_v)
    assert same_bytes(fresh.cpu(), dst_v.cpu())


@pytest.mark.parametrize("shape", [(2, 5, 7), (3, 33, 70)], ids=["2x5x7", "3x33x70"])
def test_forward_on_the_bridge_equals_the_drop_in(stif, shape):
    ops, L = stif.ops, stif._lib
    n, H, W = shape
    g = torch.Generator().manual_seed(H)
    inp, weight, bias = torch.randn(n, 64, H, W, generator=g), torch.randn(64, 64, 3, 3, generator=g) / 24, \
        torch.randn(64, generator=g)
    om = torch.randn(n, H, W, 256, generator=g).cuda()
    om[..., :144] *= 3
    offset = om[..., :144].permute(0, 3, 1, 2).contiguous()
    mask = torch.sigmoid(om[..., 144:216]).permute(0, 3, 1, 2).contiguous()
    ref = ops.dcn_v2_forward(inp.cuda(), weight.cuda(), bias.cuda(), offset, mask, *GEOM)
    out = torch.empty(n, H, W, 64, device="cuda")
    lay = ops.pack_conv_plain_dev(weight.cuda(), bias.cuda())
    ops.dcn([dict(layer=lay, inp=nhwc(inp).cuda(), offmask=ops.dcn_offmask(om), out=out)], epi=L.EPI_NONE)
    assert relmax(out.permute(0, 3, 1, 2), ref) <= 1e-5


# ---- the module ----

def module_run(stif, P, inp, fea, gout, off=()):
    m = stif.train.DCN_sep("lrelu", "f32")
    m.load_state_dict(P, strict=True)
    m = m.cuda()
    ig, fg = (t.float().cuda().requires_grad_("input" not in off) for t in (inp, fea))
    fg.requires_grad_(True)
    if "weight" in off:
        m.weight.requires_grad_(False)
        m.bias.requires_grad_(False)
    m(ig, fg).backward(gout.float().cuda())
    grads = {"input": ig.grad, "fea": fg.grad}
    grads.update({k: p.grad for k, p in m.named_parameters()})
    return grads


def test_module_computes_only_the_gradients_asked_for(stif):
    n, H, W = 2, 5, 7
    g = torch.Generator().manual_seed(21)
    rnd = lambda *s: torch.randn(*s, generator=g).double()
    inp, fea, gout = rnd(n, 64, H, W), rnd(n, 64, H, W), rnd(n, 64, H, W)
    P = {"weight": rnd(64, 64, 3, 3) / 24, "bias": rnd(64) * 0.1,
         "conv_offset_mask.weight": rnd(216, 64, 3, 3) / 24, "conv_offset_mask.bias": rnd(216) * 0.1}
    R.tame_dcn(P["conv_offset_mask.weight"], P["conv_offset_mask.bias"], fea)
    P = {k: v.float() for k, v in P.items()}
    full = module_run(stif, P, inp, fea, gout)
    assert all(v is not None for v in full.values())
    for off, none in ((("weight",), ("weight", "bias")), (("input",), ("input",))):
        part = module_run(stif, P, inp, fea, gout, off)
        for k, v in part.items():
            if k in none:
                assert v is None, (off, k)
            elif k == "input":
                assert relmax(v, full[k]) <= RTOL_DCN, (off, k)
            else:
                assert same_bytes(v, full[k]), (off, k)
