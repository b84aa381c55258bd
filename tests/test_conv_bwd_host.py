"""3x3 conv backward, the host side (no GPU): the three new symbols are declared, exported and bound with their
signatures; stif_conv3x3_wgrad and stif_pack_conv_weight_dev reject every invalid argument with its reason before any
launch -- fake pointers (4096) that are never dereferenced, in the manner of tests/test_points_ensemble_host.py; the
training modules load the reference's state-dict slices strictly and refuse CPU tensors with a clear error."""
import ctypes as C
import os
import re

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = 4096
PART = 64 * 64 * 9 + 64          # floats of one workgroup's partial sum (conv_bwd.hip)
TH, TW = 2, 32                   # the weight-gradient kernel's tile (conv_bwd.hip)


def wgrad_args(L, **changed):
    a = L.ConvWgradArgs()
    a.x, a.gy, a.gw, a.gb = A, A, A, A
    a.x_item = a.gy_item = 5 * 7 * 64
    a.n, a.H, a.W, a.cin, a.cout = 2, 5, 7, 64, 64
    a.workspace, a.workspace_bytes = A, 6 * PART * 4      # 2 items x 3 x 1 tiles
    for k, v in changed.items():
        setattr(a, k, v)
    return a


def wgrad_rejected(L, text, **changed):
    lib = L.lib()
    lib.stif_dec_blend4(None, None, None, 0, 0, 0, None)   # another text sits in the error slot first
    rc = lib.stif_conv3x3_wgrad(C.byref(wgrad_args(L, **changed)), None)
    err = lib.stif_last_error().decode()
    assert rc == L.E_INVALID, (changed, rc, err)           # anything else would have launched
    assert err.startswith("stif_conv3x3_wgrad: ") and text in err, (changed, text, err)


PACK = ["w_oihw", "b", "cout", "cin", "ks", "mode", "flags", "w_dst", "b_dst", "status", "stream"]


def pack_rejected(L, text, **changed):
    lib = L.lib()
    a = dict(w_oihw=A, b=A, cout=64, cin=64, ks=3, mode=L.PACK_WINO, flags=0, w_dst=A, b_dst=A, status=A, stream=None)
    for k, v in changed.items():
        assert k in a, k
        a[k] = v
    lib.stif_dec_blend4(None, None, None, 0, 0, 0, None)
    rc = lib.stif_pack_conv_weight_dev(*[a[k] for k in PACK])
    err = lib.stif_last_error().decode()
    assert rc == L.E_INVALID, (changed, rc, err)
    assert err.startswith("stif_pack_conv_weight_dev: ") and text in err, (changed, text, err)


def test_the_symbols_are_declared_exported_and_bound(stif):
    L = stif._lib
    hdr = open(os.path.join(REPO, "include", "stif.h")).read()
    sigs = {"stif_conv3x3_wgrad": ("int", 2), "stif_conv3x3_wgrad_workspace_size": ("size_t", 5),
            "stif_pack_conv_weight_dev": ("int", 11)}
    for name, (ret, nargs) in sigs.items():
        m = re.search(r"^\s*%s\s+%s\s*\(([^;]*)\);" % (ret, name), hdr, re.M)
        assert m, name
        assert len(m.group(1).split(",")) == nargs, (name, m.group(1))
        assert hasattr(L.lib(), name), name
        res, args = L.EXPORTS[name]
        assert res is (C.c_int if ret == "int" else C.c_size_t) and len(args) == nargs, name
    fields = [f for f, _ in L.ConvWgradArgs._fields_]
    assert fields == ["x", "gy", "gw", "gb", "x_item", "gy_item", "n", "H", "W", "cin", "cout", "workspace",
                      "workspace_bytes"]
    body = re.search(r"typedef struct \{([^}]*)\} stif_conv_wgrad_args;", hdr).group(1)
    names = re.findall(r"(\w+)\s*[,;]", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert names == fields, names                                       # the binding's order is the header's
    assert "#define STIF_PACK_DGRAD 1" in hdr and L.PACK_DGRAD == 1
    assert "#define STIF_STATUS_PACK_RANGE 16" in hdr and L.STATUS_PACK_RANGE == 16
    for name in ("conv3x3_wgrad", "pack_conv_dev"):
        assert callable(getattr(stif.ops, name)), name
    for name in ("Conv3x3", "ResidualBlock_noBN", "make_trunk", "range_status"):
        assert callable(getattr(stif.train, name)), name


def test_wgrad_workspace_size(stif):
    """G partials' worth, G = min(tiles, 2 per CU): a function of the shape and the CU count (256 when no device
    answers, as here or on the MI355X); zero for anything the entry point refuses."""
    size = stif._lib.lib().stif_conv3x3_wgrad_workspace_size
    assert size(2, 5, 7, 64, 64) == 6 * PART * 4
    assert size(1, 1, 1, 64, 64) == PART * 4
    assert size(1, TH + 1, TW + 1, 64, 64) == 4 * PART * 4
    big = size(2, 192, 192, 64, 64)
    assert big % (PART * 4) == 0 and 0 < big // (PART * 4) < 2 * 96 * 6      # fewer workgroups than tiles
    for bad in ((0, 5, 7, 64, 64), (2, 0, 7, 64, 64), (2, 5, 0, 64, 64), (2, 5, 7, 128, 64), (2, 5, 7, 64, 216)):
        assert size(*bad) == 0, bad


def test_wgrad_validates_before_launching(stif):
    L = stif._lib
    L.lib().stif_dec_blend4(None, None, None, 0, 0, 0, None)
    assert L.lib().stif_conv3x3_wgrad(None, None) == L.E_INVALID
    assert "stif_conv3x3_wgrad: null args" in L.lib().stif_last_error().decode()
    for p in ("x", "gy", "gw"):
        wgrad_rejected(L, "null pointer", **{p: None})
    for k in ("n", "H", "W"):
        for v in (0, -1):
            wgrad_rejected(L, "must be >= 1", **{k: v})
    for ch in (dict(cin=128), dict(cout=216), dict(cin=32, cout=32), dict(cin=0)):
        wgrad_rejected(L, "unsupported channel counts", **ch)
    wgrad_rejected(L, "workspace too small", workspace=None)
    wgrad_rejected(L, "workspace too small", workspace_bytes=6 * PART * 4 - 1)
    wgrad_rejected(L, "workspace too small", workspace_bytes=0)
    wgrad_rejected(L, "workspace not 16-byte aligned", workspace=A + 4)
    wgrad_rejected(L, "negative item stride", x_item=-64)
    wgrad_rejected(L, "negative item stride", gy_item=-64)
    wgrad_rejected(L, "16-byte aligned", x=A + 4)
    wgrad_rejected(L, "16-byte aligned", gy_item=5 * 7 * 64 + 2)
    # 2900 x 2900 x 64 floats = 2.15e9 bytes: past the buffer-addressing limit the forward enforces
    wgrad_rejected(L, "item larger than 2 GB", H=2900, W=2900, workspace_bytes=1 << 40)
    L.lib().stif_dec_blend4(None, None, None, 0, 0, 0, None)
    cargs = L.ConvArgs()
    cargs.ngroups = cargs.nitems = 1
    cargs.H = cargs.W = cargs.Ho = cargs.Wo = 2900
    cargs.C0 = cargs.cout = 64
    cargs.ks, cargs.stride = 3, 1
    for i in ("in0", "w", "bias", "out"):
        getattr(cargs, i)[0] = A
    assert L.lib().stif_conv3x3_wino(C.byref(cargs), None) == L.E_INVALID       # the same limit, the same words
    assert "item larger than 2 GB" in L.lib().stif_last_error().decode()
    # gb alone may be null: nothing else is wrong with these arguments, so only a launch could follow -- not made here


def test_device_packer_validates_before_launching(stif):
    L = stif._lib
    for p in ("w_oihw", "w_dst", "b_dst"):
        pack_rejected(L, "null pointer", **{p: None})
    for mode in (L.PACK_PLAIN, L.PACK_WINO_OFFMASK, L.PACK_WINO_LSTM, L.PACK_PLAIN | L.PACK_F16X3,
                 L.PACK_DCNPAIR | L.PACK_F16X3, L.PACK_WINO | 32):
        pack_rejected(L, "unsupported mode", mode=mode)
    pack_rejected(L, "3x3 kernel", ks=1)
    for ch in (dict(cout=216), dict(cin=128), dict(cin=32, cout=32)):
        pack_rejected(L, "unsupported channel counts", **ch)
    pack_rejected(L, "unknown flags", flags=2)
    pack_rejected(L, "null bias", b=None)
    pack_rejected(L, "needs a status word", mode=L.PACK_WINO | L.PACK_F16X3, status=None)


def test_trunk_loads_the_reference_slices_strictly(stif, sd):
    T = stif.train
    for prefix in ("recon_trunk.", "feature_extraction."):
        trunk = T.make_trunk(2)
        part = {k[len(prefix):]: torch.from_numpy(v) for k, v in sd.items()
                if k.startswith(prefix + "0.") or k.startswith(prefix + "1.")}
        assert sorted(part) == sorted(f"{i}.conv{j}.{p}" for i in (0, 1) for j in (1, 2) for p in ("weight", "bias"))
        trunk.load_state_dict(part, strict=True)
        assert list(trunk.state_dict()) == [f"{i}.conv{j}.{p}" for i in (0, 1) for j in (1, 2)
                                            for p in ("weight", "bias")]
        assert torch.equal(trunk[1].conv2.weight.detach(), part["1.conv2.weight"])
    c = T.Conv3x3()
    assert tuple(c.weight.shape) == (64, 64, 3, 3) and tuple(c.bias.shape) == (64,)
    ref = torch.nn.Conv2d(64, 64, 3, 1, 1)
    c.load_state_dict(ref.state_dict(), strict=True)
    blk = T.ResidualBlock_noBN()
    with torch.no_grad():                                                     # the reference's 0.1-scaled init
        assert float(blk.conv1.bias.abs().max()) == 0.0 and float(blk.conv2.weight.std()) < 0.01


def test_modules_refuse_cpu_tensors_and_bad_choices(stif):
    T = stif.train
    x = torch.zeros(1, 64, 4, 5)
    for m in (T.Conv3x3(), T.Conv3x3(act="lrelu", mfma="f32"), T.ResidualBlock_noBN(), T.make_trunk(1)):
        with pytest.raises(RuntimeError, match="need a CUDA tensor"):
            m(x)
    with pytest.raises(ValueError, match="CUDA"):
        stif.ops.conv3x3_wgrad(torch.zeros(1, 4, 5, 64), torch.zeros(1, 4, 5, 64))
    with pytest.raises(ValueError, match="CUDA"):
        stif.ops.pack_conv_dev(torch.zeros(64, 64, 3, 3), torch.zeros(64))
    with pytest.raises(ValueError, match="64 -> 64"):
        T.Conv3x3(nf=128)
    with pytest.raises(ValueError, match="act must be"):
        T.Conv3x3(act="gelu")
    with pytest.raises(ValueError, match="mfma must be"):
        T.ResidualBlock_noBN(mfma="bf16")
