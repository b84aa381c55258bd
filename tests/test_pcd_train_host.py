"""The trainable PCD_Align, the host side (no GPU).  First the torch reference the GPU tests rest on
(tests/pcd_torch_ref.py) is pinned to the numpy oracle: its deformable conv forward against oracle.dcn_v2_forward, its
autograd gradients against oracle.dcn_v2_backward, its PCD_Align against oracle.pcd_align, all to 1e-10 of max |ref|.
Then the new symbols are declared, exported and bound; every new entry point rejects every invalid argument with its
reason before any launch (fake pointers that are never dereferenced, as tests/test_conv_bwd_host.py); and
train.PCD_Align loads the reference's three state-dict slices strictly and refuses what it cannot run."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import pcd_torch_ref as R
from oracle import stif_oracle as O

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = 4096
PART = 64 * 64 * 9 + 64
PIN = 1e-10
GEOM = (3, 3, 1, 1, 1, 1, 1, 1, 8)

SIGS = {"stif_conv3x3_wgrad_cat_workspace_size": ("size_t", 6), "stif_conv3x3_wgrad_cat": ("int", 2),
        "stif_upsample2x_bwd_nhwc": ("int", 10), "stif_pack_conv_block_dev": ("int", 12)}
CAT_FIELDS = ["x", "gy", "gw", "gb", "x_item", "gy_item", "n", "H", "W", "nx", "gy_channels", "cout", "workspace",
              "workspace_bytes"]
SUPPORTED = {(2, 64, 64): 2, (1, 256, 216): 4, (1, 64, 64): 1}     # (nx, gy_channels, cout): blocks


def rel(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(got - ref).max() / np.abs(ref).max())


def rejected(L, name, args, text, why):
    lib = L.lib()
    lib.stif_dec_blend4(None, None, None, 0, 0, 0, None)   # another text sits in the error slot first
    rc = getattr(lib, name)(*args)
    err = lib.stif_last_error().decode()
    assert rc == L.E_INVALID, (name, why, rc, err)         # anything else would have launched
    assert err.startswith(name + ": ") and text in err, (name, why, text, err)


# ---- the torch reference against the oracle ----

def dcn_case(seed=5, B=1, H=5, W=7):
    """The STIF shape (64 -> 64, 8 groups) on 1x5x7 maps; offsets = an integer in -2..2 (samples on both sides of every
    border) plus a fraction in [0.2, 0.8] on a 1/1024 grid."""
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    inp, weight, bias, gout = rnd(B, 64, H, W), rnd(64, 64, 3, 3) / 24, rnd(64), rnd(B, 64, H, W)
    offset = (torch.randint(-2, 3, (B, 144, H, W), generator=g)
              + torch.randint(205, 820, (B, 144, H, W), generator=g) / 1024.0).double()
    mask = torch.sigmoid(rnd(B, 72, H, W))
    return inp, offset, mask, weight, bias, gout


def test_reference_dcn_forward_matches_the_oracle():
    inp, offset, mask, weight, bias, _ = dcn_case()
    R.assert_offsets_tame(offset)
    got = R.dcn(inp, offset, mask, weight, bias)
    ref = O.dcn_v2_forward(inp.numpy(), weight.numpy(), bias.numpy(), offset.numpy(), mask.numpy(), *GEOM)
    assert rel(got, ref) < PIN, rel(got, ref)


def test_reference_dcn_gradients_match_the_oracle():
    inp, offset, mask, weight, bias, gout = dcn_case()
    leaves = [t.clone().requires_grad_(True) for t in (inp, offset, mask, weight, bias)]
    R.dcn(*leaves).backward(gout)
    ref = O.dcn_v2_backward(inp.numpy(), weight.numpy(), bias.numpy(), offset.numpy(), mask.numpy(), gout.numpy(),
                            *GEOM)
    for name, leaf, r in zip(("input", "offset", "mask", "weight", "bias"), leaves, ref):
        e = rel(leaf.grad, r)
        assert e < PIN, (name, e)


def test_reference_pcd_align_matches_the_oracle(stif, sd):
    pre = "pcd_align."
    P = {k[len(pre):]: torch.from_numpy(v).double().clone() for k, v in sd.items() if k.startswith(pre)}
    assert list(P) == list(R.pcd_param_shapes())
    assert all(tuple(P[k].shape) == s for k, s in R.pcd_param_shapes().items())
    fea1, fea2 = R.pyramid_inputs(11, 1, 8, 12)
    R.tame_offsets(P, fea1, fea2)
    R.assert_pcd_offsets_tame(P, fea1, fea2)
    got = R.pcd_align(P, fea1, fea2)
    sdn = {pre + k: v.numpy() for k, v in P.items()}
    ref = O.pcd_align([t.numpy() for t in fea1], [t.numpy() for t in fea2], sdn, pre, np.float64)
    assert tuple(got.shape) == (1, 128, 8, 12)
    assert rel(got, ref) < PIN, rel(got, ref)


def test_the_recipe_keeps_offsets_in_their_band():
    P = R.random_pcd_params(3)
    fea1, fea2 = R.pyramid_inputs(4, 2, 12, 20)
    feas = R.tame_offsets(P, fea1, fea2)
    assert sorted(feas) == sorted(f"L{l}_dcnpack_{s}" for l in (1, 2, 3) for s in (1, 2))
    for name, fea in feas.items():
        offset, mask = R.offset_mask(fea, P[name + ".conv_offset_mask.weight"], P[name + ".conv_offset_mask.bias"])
        assert float((offset - 0.5).abs().max()) <= 0.3 and float((offset - 0.5).abs().max()) > 0.29
        assert 0.0 < float(mask.min()) < 0.45 and 0.55 < float(mask.max()) < 1.0      # the mask rows stay random
    with pytest.raises(AssertionError):
        R.assert_offsets_tame(torch.tensor([0.5, 1.05]))


# ---- the C ABI ----

def test_the_symbols_are_declared_exported_and_bound(stif):
    L = stif._lib
    hdr = open(os.path.join(REPO, "include", "stif.h")).read()
    for name, (ret, nargs) in SIGS.items():
        m = re.search(r"^\s*%s\s+%s\s*\(([^;]*)\);" % (ret, name), hdr, re.M)
        assert m, name
        assert len(m.group(1).split(",")) == nargs, (name, m.group(1))
        assert hasattr(L.lib(), name), name
        res, args = L.EXPORTS[name]
        assert res is (C.c_int if ret == "int" else C.c_size_t) and len(args) == nargs, name
    assert [f for f, _ in L.ConvWgradCatArgs._fields_] == CAT_FIELDS
    body = re.search(r"typedef struct \{([^}]*)\} stif_conv_wgrad_cat_args;", hdr).group(1)
    body = re.sub(r"\[\d+\]", "", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert re.findall(r"(\w+)\s*[,;]", body) == CAT_FIELDS
    a = L.ConvWgradCatArgs()                                # zero-initialisable: nothing set, everything null
    assert not a.x[0] and not a.x[1] and a.nx == 0 and a.workspace_bytes == 0
    for name in ("conv3x3_wgrad_cat", "upsample2x_bwd", "pack_conv_blocks_dev"):
        assert callable(getattr(stif.ops, name)), name
    for name in ("Upsample2x", "Conv3x3Cat", "DCN_sep", "PCD_Align"):
        assert callable(getattr(stif.train, name)), name


def test_workspace_size_is_blocks_times_the_64_to_64_size(stif):
    lib = stif._lib.lib()
    cat, one = lib.stif_conv3x3_wgrad_cat_workspace_size, lib.stif_conv3x3_wgrad_workspace_size
    for n, H, W in ((1, 1, 1), (2, 5, 7), (1, 3, 33), (3, 33, 70), (6, 128, 128)):
        base = one(n, H, W, 64, 64)
        assert base > 0 and base % (PART * 4) == 0
        for shape, blocks in SUPPORTED.items():
            assert cat(n, H, W, *shape) == blocks * base, (n, H, W, shape)
    assert cat(2, 5, 7, 1, 256, 216) == 4 * 6 * PART * 4          # 2 items x 3 x 1 tiles of 2 x 32 pixels
    for bad in ((2, 64, 216), (2, 256, 216), (1, 64, 216), (1, 256, 64), (1, 256, 256), (3, 64, 64), (0, 64, 64),
                (1, 128, 128), (1, 216, 216)):
        assert cat(2, 5, 7, *bad) == 0, bad
    for bad in ((0, 5, 7), (2, 0, 7), (2, 5, -1)):
        assert cat(*bad, 2, 64, 64) == 0, bad


def cat_args(L, **changed):
    a = L.ConvWgradCatArgs()
    a.x[0], a.x[1], a.gy, a.gw, a.gb = A, A, A, A, A
    a.x_item[0], a.x_item[1], a.gy_item = 5 * 7 * 64, 5 * 7 * 64, 5 * 7 * 64
    a.n, a.H, a.W, a.nx, a.gy_channels, a.cout = 2, 5, 7, 2, 64, 64
    a.workspace, a.workspace_bytes = A, 2 * 6 * PART * 4      # 2 blocks x 6 tiles
    for k, v in changed.items():
        if isinstance(k, str) and k[-1] in "01" and k[:-1] in ("x", "x_item"):
            getattr(a, k[:-1])[int(k[-1])] = v
        else:
            setattr(a, k, v)
    return a


def test_wgrad_cat_validates_before_launching(stif):
    L = stif._lib
    name = "stif_conv3x3_wgrad_cat"
    rej = lambda text, **ch: rejected(L, name, (C.byref(cat_args(L, **ch)), None), text, ch)
    om = dict(nx=1, gy_channels=256, cout=216, gy_item=5 * 7 * 256, workspace_bytes=4 * 6 * PART * 4)
    rejected(L, name, (None, None), "null args", "args")
    for p in ("x0", "gy", "gw"):
        rej("null pointer", **{p: None})
    rej("null pointer (x[1]", x1=None)
    for k in ("n", "H", "W"):
        for v in (0, -1):
            rej("must be >= 1", **{k: v})
    for ch in (dict(nx=2, gy_channels=256, cout=216), dict(nx=1, gy_channels=64, cout=216), dict(cout=128),
               dict(nx=0), dict(nx=3), dict(gy_channels=128), dict(nx=1, gy_channels=256, cout=256),
               dict(nx=1, gy_channels=216, cout=216)):
        rej("unsupported channel counts", **ch)
    rej("negative item stride", x_item0=-64)
    rej("negative item stride", x_item1=-64)
    rej("negative item stride", gy_item=-64)
    rej("16-byte aligned", x0=A + 4)
    rej("16-byte aligned", x1=A + 8)
    rej("16-byte aligned", gy=A + 4)
    rej("16-byte aligned", x_item1=5 * 7 * 64 + 2)
    rej("16-byte aligned", gy_item=5 * 7 * 64 + 1)
    rej("item larger than 2 GB", H=2900, W=2900, workspace_bytes=1 << 40)
    rej("item larger than 2 GB", **dict(om, H=1450, W=1450, workspace_bytes=1 << 40))    # 2 GB with the real pitch
    rej("workspace too small", workspace=None)
    rej("workspace too small", workspace_bytes=2 * 6 * PART * 4 - 1)
    rej("workspace too small", workspace_bytes=0)
    rej("workspace too small", **dict(om, workspace_bytes=4 * 6 * PART * 4 - 1))
    rej("workspace too small", **dict(om, workspace_bytes=2 * 6 * PART * 4))           # the cat form's size
    rej("workspace not 16-byte aligned", workspace=A + 4)
    rej("workspace not 16-byte aligned", **dict(om, workspace=A + 8))
    # with one map x[1] and its stride are not looked at
    a = cat_args(L, nx=1, x1=None, x_item1=-3, gy=None)
    rejected(L, name, (C.byref(a), None), "null pointer (x[0], gy, gw)", "nx = 1")


UPB = ["gy", "gx", "n", "h1", "w1", "c", "scale", "gy_item", "gx_item", "stream"]


def test_upsample_backward_validates_before_launching(stif):
    L = stif._lib
    base = dict(gy=A, gx=A, n=2, h1=3, w1=5, c=64, scale=1.0, gy_item=4 * 3 * 5 * 64, gx_item=3 * 5 * 64, stream=None)

    def rej(text, **ch):
        assert set(ch) <= set(base)
        rejected(L, "stif_upsample2x_bwd_nhwc", [dict(base, **ch)[k] for k in UPB], text, ch)

    for p in ("gy", "gx"):
        rej("null pointer", **{p: None})
    for k in ("n", "h1", "w1"):
        for v in (0, -1):
            rej("must be >= 1", **{k: v})
    for c in (0, 2, 6, -4):
        rej("multiple of 4", c=c)
    rej("negative item stride", gy_item=-64)
    rej("negative item stride", gx_item=-64)
    rej("16-byte aligned", gy=A + 4)
    rej("16-byte aligned", gx=A + 8)
    rej("16-byte aligned", gy_item=4 * 3 * 5 * 64 + 2)
    rej("16-byte aligned", gx_item=3 * 5 * 64 + 1)
    rej("gx items overlap", gx_item=3 * 5 * 64 - 4)
    rej("too large", n=1, h1=70000)


BLK = ["w_oihw", "b", "cout", "cin", "co0", "ci0", "mode", "flags", "w_dst", "b_dst", "status", "stream"]


def test_block_packer_validates_before_launching(stif):
    L = stif._lib
    base = dict(w_oihw=A, b=A, cout=216, cin=64, co0=64, ci0=0, mode=L.PACK_WINO | L.PACK_F16X3, flags=0, w_dst=A,
                b_dst=A, status=A, stream=None)

    def rej(text, **ch):
        assert set(ch) <= set(base)
        rejected(L, "stif_pack_conv_block_dev", [dict(base, **ch)[k] for k in BLK], text, ch)

    for p in ("w_oihw", "w_dst", "b_dst"):
        rej("null pointer", **{p: None})
    for mode in (L.PACK_PLAIN, L.PACK_WINO_OFFMASK, L.PACK_WINO_LSTM | L.PACK_F16X3, L.PACK_PLAIN | L.PACK_F16X3):
        rej("unsupported mode", mode=mode)
    for ch in (dict(cout=256), dict(cout=128), dict(cin=256), dict(cin=32), dict(cout=0), dict(cin=0)):
        rej("unsupported channel counts", **ch)
    for ch in (dict(co0=256), dict(co0=216), dict(co0=32), dict(co0=-64), dict(ci0=64), dict(ci0=-64),
               dict(cin=128, ci0=128), dict(cin=128, ci0=32), dict(cout=64, co0=64)):
        rej("multiples of 64 inside the weight", **ch)
    rej("unknown flags", flags=2)
    rej("null bias", b=None)
    rej("status word", status=None)


def test_the_existing_entry_points_still_refuse_the_wider_shapes(stif):
    L = stif._lib
    for cin, cout in ((128, 64), (64, 216)):
        a = L.ConvWgradArgs()
        a.x, a.gy, a.gw = A, A, A
        a.n, a.H, a.W, a.cin, a.cout = 1, 4, 4, cin, cout
        a.workspace, a.workspace_bytes = A, 1 << 30
        rejected(L, "stif_conv3x3_wgrad", (C.byref(a), None), "unsupported channel counts", (cin, cout))
        assert L.lib().stif_conv3x3_wgrad_workspace_size(1, 4, 4, cin, cout) == 0
        rejected(L, "stif_pack_conv_weight_dev", (A, A, cout, cin, 3, L.PACK_WINO, 0, A, A, A, None),
                 "unsupported channel counts", (cin, cout))
    with pytest.raises(ValueError, match="64 -> 64"):
        stif.train.Conv3x3(nf=128)


# ---- the modules ----

@pytest.mark.parametrize("prefix", ["pcd_align.", "ConvBLSTM.forward_net.pcd_h.pcd_align.",
                                    "ConvBLSTM.forward_net.pcd_c.pcd_align."])
def test_pcd_align_loads_the_reference_slices_strictly(stif, sd, prefix):
    net = stif.train.PCD_Align()
    part = {k[len(prefix):]: torch.from_numpy(v) for k, v in sd.items() if k.startswith(prefix)}
    assert len(part) == 64
    net.load_state_dict(part, strict=True)
    assert list(net.state_dict()) == list(part)                 # the reference's registration order
    assert list(net.state_dict()) == list(R.pcd_param_shapes())
    for k, v in net.state_dict().items():
        assert tuple(v.shape) == R.pcd_param_shapes()[k], k
        assert torch.equal(v, part[k]), k
    assert [n for n, _ in net.named_children()][:13] == [
        "L3_offset_conv1_1", "L3_offset_conv2_1", "L3_dcnpack_1", "L2_offset_conv1_1", "L2_offset_conv2_1",
        "L2_offset_conv3_1", "L2_dcnpack_1", "L2_fea_conv_1", "L1_offset_conv1_1", "L1_offset_conv2_1",
        "L1_offset_conv3_1", "L1_dcnpack_1", "L1_fea_conv_1"]


def test_parameter_names_shapes_and_initial_values(stif):
    T = stif.train
    torch.manual_seed(0)
    d = T.DCN_sep()
    assert [(k, tuple(v.shape)) for k, v in d.state_dict().items()] == [
        ("weight", (64, 64, 3, 3)), ("bias", (64,)), ("conv_offset_mask.weight", (216, 64, 3, 3)),
        ("conv_offset_mask.bias", (216,))]
    stdv = 1.0 / (64 * 9) ** 0.5
    w = d.weight.detach()
    assert 0.99 * stdv < float(w.abs().max()) <= stdv                       # uniform(-stdv, stdv), dcn_v2.py:69-75
    assert float(w.std()) == pytest.approx(stdv / 3 ** 0.5, rel=0.02) and abs(float(w.mean())) < 0.03 * stdv
    assert float(d.bias.detach().abs().max()) == 0.0
    assert all(float(p.detach().abs().max()) == 0.0 for p in d.conv_offset_mask.parameters())
    assert all(p.requires_grad for p in d.parameters())
    c = T.Conv3x3Cat()
    ref = torch.nn.Conv2d(128, 64, 3, 1, 1)
    assert [(k, tuple(v.shape)) for k, v in c.state_dict().items()] == [
        (k, tuple(v.shape)) for k, v in ref.state_dict().items()]
    c.load_state_dict(ref.state_dict(), strict=True)
    bound = 1.0 / (128 * 9) ** 0.5             # nn.Conv2d's default, kaiming_uniform(a = sqrt 5): 1 / sqrt(fan_in)
    fresh = T.Conv3x3Cat()
    assert 0.99 * bound < float(fresh.weight.detach().abs().max()) <= bound
    assert float(fresh.bias.detach().abs().max()) <= bound
    assert list(T.Upsample2x(2.0).state_dict()) == [] and T.Upsample2x(2.0).scale == 2.0


def test_modules_refuse_cpu_tensors_bad_sizes_and_bad_choices(stif):
    T, ops = stif.train, stif.ops
    z = lambda *s: torch.zeros(*s)
    with pytest.raises(RuntimeError, match="need a CUDA tensor"):
        T.Upsample2x()(z(1, 64, 4, 5))
    with pytest.raises(RuntimeError, match="need a CUDA tensor"):
        T.Conv3x3Cat()(z(1, 64, 4, 5), z(1, 64, 4, 5))
    with pytest.raises(RuntimeError, match="need a CUDA tensor"):
        T.DCN_sep()(z(1, 64, 4, 5), z(1, 64, 4, 5))
    pyr = lambda H, W: [z(1, 64, H >> l, W >> l) for l in range(3)]
    with pytest.raises(RuntimeError, match="need a CUDA tensor"):
        T.PCD_Align()(pyr(8, 12), pyr(8, 12))
    for H, W in ((6, 12), (8, 10), (9, 12)):
        with pytest.raises(ValueError, match="multiples of 4"):
            T.PCD_Align()([z(1, 64, H, W), z(1, 64, H // 2, W // 2), z(1, 64, H // 4, W // 4)], pyr(8, 12))
    with pytest.raises(ValueError, match="level L2"):
        T.PCD_Align()([z(1, 64, 8, 12), z(1, 64, 4, 5), z(1, 64, 2, 3)], pyr(8, 12))
    with pytest.raises(ValueError, match="act must be"):
        T.Conv3x3Cat(act="gelu")
    with pytest.raises(ValueError, match="act must be"):
        T.DCN_sep(act="relu")
    for mk in (T.Conv3x3Cat, T.DCN_sep, T.PCD_Align):
        with pytest.raises(ValueError, match="mfma must be"):
            mk(mfma="bf16")
    with pytest.raises(ValueError, match="CUDA"):
        ops.conv3x3_wgrad_cat([z(1, 4, 5, 64), z(1, 4, 5, 64)], z(1, 4, 5, 64), 64)
    with pytest.raises(ValueError, match="unsupported channel counts"):
        ops.conv3x3_wgrad_cat([z(1, 4, 5, 64), z(1, 4, 5, 64)], z(1, 4, 5, 256), 216)
    with pytest.raises(ValueError, match="CUDA"):
        ops.upsample2x_bwd(z(1, 4, 6, 64))
    with pytest.raises(ValueError, match="2h, 2w"):
        ops.upsample2x_bwd(z(1, 3, 6, 64))
    with pytest.raises(ValueError, match="CUDA"):
        ops.pack_conv_blocks_dev(z(64, 128, 3, 3), z(64))
