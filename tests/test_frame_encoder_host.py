"""The trainable frame encoder, the host side (no GPU): the new symbols are declared, exported and bound with matching
arities; every new entry point rejects every invalid argument with its reason before any launch -- fake pointers
(4096) that are never dereferenced, in the manner of tests/test_conv_bwd_host.py; train.FrameFeatures loads the
reference's state-dict slices strictly, and the modules refuse CPU tensors and an input that requires grad."""
import ctypes as C
import os
import re

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = 4096
PART = 64 * 64 * 9 + 64          # floats of one stride-2 workgroup's partial sum (conv_bwd.hip, as stride 1)
TH, TW = 2, 16                   # the stride-2 weight-gradient tile, in output pixels (conv_bwd.hip)
CF_PART, CF_WG_PX = 28 * 64, 512  # conv_first: floats per partial, pixels per workgroup chunk (conv_bwd.hip)

SIGS = {"stif_conv3x3s2_wgrad_workspace_size": ("size_t", 5), "stif_conv3x3s2_wgrad": ("int", 2),
        "stif_conv3x3s2_dgrad_workspace_size": ("size_t", 3), "stif_conv3x3s2_dgrad": ("int", 11),
        "stif_conv_first_wgrad_workspace_size": ("size_t", 3), "stif_conv_first_wgrad": ("int", 11),
        "stif_pack_conv_plain_dev": ("int", 8)}


def rejected(L, name, args, text, why):
    lib = L.lib()
    lib.stif_dec_blend4(None, None, None, 0, 0, 0, None)   # another text sits in the error slot first
    rc = getattr(lib, name)(*args)
    err = lib.stif_last_error().decode()
    assert rc == L.E_INVALID, (name, why, rc, err)         # anything else would have launched
    assert err.startswith(name + ": ") and text in err, (name, why, text, err)


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
    fields = [f for f, _ in L.ConvWgradArgs._fields_]
    assert len(fields) == 13 and fields == ["x", "gy", "gw", "gb", "x_item", "gy_item", "n", "H", "W", "cin", "cout",
                                            "workspace", "workspace_bytes"]
    body = re.search(r"typedef struct \{([^}]*)\} stif_conv_wgrad_args;", hdr).group(1)
    assert re.findall(r"(\w+)\s*[,;]", re.sub(r"/\*.*?\*/", "", body, flags=re.S)) == fields
    for name in ("conv3x3s2_wgrad", "conv3x3s2_dgrad", "conv_first_wgrad", "pack_conv_plain_dev"):
        assert callable(getattr(stif.ops, name)), name
    for name in ("ConvDown", "ConvFirst", "FrameFeatures"):
        assert callable(getattr(stif.train, name)), name


def test_workspace_sizes(stif):
    """Partials' worth of bytes: exact below one grid (256 CUs when no device answers, as on the MI355X), monotone in
    the shape, and zero for anything the entry points refuse."""
    lib = stif._lib.lib()
    s2, cf, dg = (lib.stif_conv3x3s2_wgrad_workspace_size, lib.stif_conv_first_wgrad_workspace_size,
                  lib.stif_conv3x3s2_dgrad_workspace_size)
    assert s2(2, 5, 7, 64, 64) == 2 * 2 * 1 * PART * 4                   # 3 x 4 outputs: 2 x 1 tiles per item
    assert s2(2, 6, 8, 64, 64) == 2 * 2 * 1 * PART * 4
    assert s2(1, 1, 1, 64, 64) == PART * 4
    assert s2(1, 2 * (TH + 1) - 1, 2 * (TW + 1), 64, 64) == 4 * PART * 4
    big = s2(2, 192, 192, 64, 64)
    assert big % (PART * 4) == 0 and 0 < big // (PART * 4) < 2 * 48 * 6      # fewer workgroups than tiles
    sizes = [s2(n, h, w, 64, 64) for n, h, w in ((1, 8, 8), (1, 16, 64), (2, 16, 64), (2, 64, 64), (4, 256, 256))]
    assert sizes == sorted(sizes) and sizes[0] > 0
    for bad in ((0, 5, 7, 64, 64), (2, 0, 7, 64, 64), (2, 5, -1, 64, 64), (2, 5, 7, 128, 64), (2, 5, 7, 64, 216)):
        assert s2(*bad) == 0, bad
    assert cf(1, 1, 1) == CF_PART * 4 and cf(2, 5, 7) == CF_PART * 4
    assert cf(1, 16, 33) == 2 * CF_PART * 4                                    # 528 pixels: two chunks
    assert cf(3, 33, 70) == -(-3 * 33 * 70 // CF_WG_PX) * CF_PART * 4
    sizes = [cf(n, h, w) for n, h, w in ((1, 8, 8), (1, 64, 64), (2, 64, 64), (2, 192, 192), (14, 256, 256))]
    assert sizes == sorted(sizes) and sizes[-1] < -(-14 * 256 * 256 // CF_WG_PX) * CF_PART * 4
    for bad in ((0, 5, 7), (2, 0, 7), (2, 5, -3)):
        assert cf(*bad) == 0 and dg(*bad) == 0, bad
    assert dg(2, 5, 7) == 0 and dg(14, 256, 256) == 0        # the weight is transposed by the kernel's own loads


def s2_args(L, **changed):
    a = L.ConvWgradArgs()
    a.x, a.gy, a.gw, a.gb = A, A, A, A
    a.x_item, a.gy_item = 5 * 7 * 64, 3 * 4 * 64
    a.n, a.H, a.W, a.cin, a.cout = 2, 5, 7, 64, 64
    a.workspace, a.workspace_bytes = A, 4 * PART * 4
    for k, v in changed.items():
        setattr(a, k, v)
    return a


def test_stride2_wgrad_validates_before_launching(stif):
    L = stif._lib
    name = "stif_conv3x3s2_wgrad"
    rej = lambda text, **ch: rejected(L, name, (C.byref(s2_args(L, **ch)), None), text, ch)
    rejected(L, name, (None, None), "null args", "args")
    for p in ("x", "gy", "gw"):
        rej("null pointer", **{p: None})
    for k in ("n", "H", "W"):
        for v in (0, -1):
            rej("must be >= 1", **{k: v})
    for ch in (dict(cin=128), dict(cout=216), dict(cin=32, cout=32), dict(cin=0)):
        rej("unsupported channel counts", **ch)
    rej("workspace too small", workspace=None)
    rej("workspace too small", workspace_bytes=4 * PART * 4 - 1)
    rej("workspace too small", workspace_bytes=0)
    rej("workspace not 16-byte aligned", workspace=A + 4)
    rej("negative item stride", x_item=-64)
    rej("negative item stride", gy_item=-64)
    rej("16-byte aligned", x=A + 4)
    rej("16-byte aligned", gy=A + 8)
    rej("16-byte aligned", gy_item=3 * 4 * 64 + 2)
    rej("item larger than 2 GB", H=2900, W=2900, workspace_bytes=1 << 40)


DGRAD = ["gy", "w_oihw", "gx", "gy_item", "gx_item", "n", "H", "W", "workspace", "workspace_bytes", "stream"]


def test_stride2_dgrad_validates_before_launching(stif):
    L = stif._lib
    base = dict(gy=A, w_oihw=A, gx=A, gy_item=3 * 4 * 64, gx_item=5 * 7 * 64, n=2, H=5, W=7, workspace=None,
                workspace_bytes=0, stream=None)

    def rej(text, **ch):
        assert set(ch) <= set(base)
        rejected(L, "stif_conv3x3s2_dgrad", [dict(base, **ch)[k] for k in DGRAD], text, ch)

    for p in ("gy", "w_oihw", "gx"):
        rej("null pointer", **{p: None})
    for k in ("n", "H", "W"):
        for v in (0, -1):
            rej("must be >= 1", **{k: v})
    rej("negative item stride", gy_item=-64)
    rej("negative item stride", gx_item=-64)
    rej("16-byte aligned", gy=A + 4)
    rej("16-byte aligned", gx=A + 4)
    rej("16-byte aligned", gy_item=3 * 4 * 64 + 2)
    rej("16-byte aligned", gx_item=5 * 7 * 64 + 1)
    rej("item larger than 2 GB", H=2900, W=2900)


CFW = ["x_nchw", "gy", "gw", "gb", "gy_item", "n", "h", "w", "workspace", "workspace_bytes", "stream"]


def test_conv_first_wgrad_validates_before_launching(stif):
    L = stif._lib
    base = dict(x_nchw=A, gy=A, gw=A, gb=A, gy_item=5 * 7 * 64, n=2, h=5, w=7, workspace=A,
                workspace_bytes=CF_PART * 4, stream=None)

    def rej(text, **ch):
        assert set(ch) <= set(base)
        rejected(L, "stif_conv_first_wgrad", [dict(base, **ch)[k] for k in CFW], text, ch)

    for p in ("x_nchw", "gy", "gw"):
        rej("null pointer", **{p: None})
    for k in ("n", "h", "w"):
        for v in (0, -1):
            rej("must be >= 1", **{k: v})
    rej("negative item stride", gy_item=-64)
    rej("16-byte aligned", gy=A + 4)
    rej("16-byte aligned", gy_item=5 * 7 * 64 + 2)
    rej("item larger than 2 GB", h=2900, w=2900, workspace_bytes=1 << 40)
    rej("workspace too small", workspace=None)
    rej("workspace too small", workspace_bytes=CF_PART * 4 - 1)
    rej("workspace too small", workspace_bytes=0)
    rej("workspace too small", h=16, w=33)                                     # two chunks need two partials
    rej("workspace not 16-byte aligned", workspace=A + 4)


PLAIN = ["w_oihw", "b", "cout", "cin", "ks", "w_dst", "b_dst", "stream"]


def test_plain_device_packer_validates_before_launching(stif):
    L = stif._lib
    base = dict(w_oihw=A, b=A, cout=64, cin=64, ks=3, w_dst=A, b_dst=A, stream=None)

    def rej(text, **ch):
        assert set(ch) <= set(base)
        rejected(L, "stif_pack_conv_plain_dev", [dict(base, **ch)[k] for k in PLAIN], text, ch)

    for p in ("w_oihw", "w_dst", "b_dst"):
        rej("null pointer", **{p: None})
    for ks in (1, 5, 0):
        rej("3x3 kernel", ks=ks)
    for ch in (dict(cout=216), dict(cin=128), dict(cin=32, cout=32), dict(cout=0)):
        rej("unsupported channel counts", **ch)


def test_the_existing_entry_points_still_refuse_other_shapes(stif):
    L = stif._lib
    a = L.ConvWgradArgs()
    a.x, a.gy, a.gw = A, A, A
    a.n, a.H, a.W, a.cin, a.cout = 1, 4, 4, 3, 64
    a.workspace, a.workspace_bytes = A, 1 << 30
    rejected(L, "stif_conv3x3_wgrad", (C.byref(a), None), "unsupported channel counts", "3 -> 64")
    rejected(L, "stif_pack_conv_weight_dev", (A, A, 64, 64, 3, L.PACK_PLAIN, 0, A, A, A, None), "unsupported mode",
             "PLAIN")
    with pytest.raises(ValueError, match="64 -> 64"):
        stif.train.Conv3x3(nf=128)
    with pytest.raises(ValueError, match="64 -> 64"):
        stif.train.ConvDown(nf=128)
    with pytest.raises(ValueError, match="act must be"):
        stif.train.ConvDown(act="relu")           # the stride-2 forward kernel has no ReLU epilogue
    with pytest.raises(ValueError, match="mfma must be"):
        stif.train.FrameFeatures(mfma="bf16")


def test_frame_features_loads_the_reference_slices_strictly(stif, sd):
    T = stif.train
    net = T.FrameFeatures(front_RBs=2)
    want = (["conv_first.weight", "conv_first.bias"]
            + [f"feature_extraction.{i}.conv{j}.{p}" for i in (0, 1) for j in (1, 2) for p in ("weight", "bias")]
            + [f"fea_L{l}_conv{j}.{p}" for l in (2, 3) for j in (1, 2) for p in ("weight", "bias")])
    part = {k: torch.from_numpy(sd[k]) for k in want}
    net.load_state_dict(part, strict=True)
    assert list(net.state_dict()) == want                  # the reference's registration order
    assert [k for k in sd if k in part] == want            # ... which is the state dict's own
    assert torch.equal(net.fea_L3_conv1.weight.detach(), part["fea_L3_conv1.weight"])
    assert tuple(net.conv_first.weight.shape) == (64, 3, 3, 3)
    ref = torch.nn.Conv2d(64, 64, 3, 2, 1)
    T.ConvDown().load_state_dict(ref.state_dict(), strict=True)
    T.ConvFirst().load_state_dict(torch.nn.Conv2d(3, 64, 3, 1, 1).state_dict(), strict=True)
    assert len(T.FrameFeatures().feature_extraction) == 5


def test_modules_refuse_cpu_tensors_and_frames_that_require_grad(stif):
    T = stif.train
    with pytest.raises(RuntimeError, match="need a CUDA tensor"):
        T.ConvDown()(torch.zeros(1, 64, 4, 5))
    with pytest.raises(RuntimeError, match="need a CUDA tensor"):
        T.ConvFirst()(torch.zeros(1, 3, 4, 5))
    with pytest.raises(RuntimeError, match="need a CUDA tensor"):
        T.FrameFeatures(front_RBs=1)(torch.zeros(1, 3, 4, 5))
    with pytest.raises(NotImplementedError, match="not built"):
        T.ConvFirst()(torch.zeros(1, 3, 4, 5, requires_grad=True))
    with pytest.raises(NotImplementedError, match="not built"):
        T.FrameFeatures(front_RBs=1)(torch.zeros(1, 3, 4, 5, requires_grad=True))
    ops = stif.ops
    with pytest.raises(ValueError, match="CUDA"):
        ops.conv3x3s2_wgrad(torch.zeros(1, 4, 5, 64), torch.zeros(1, 2, 3, 64))
    with pytest.raises(ValueError, match="CUDA"):
        ops.conv3x3s2_dgrad(torch.zeros(1, 2, 3, 64), torch.zeros(64, 64, 3, 3), 4, 5)
    with pytest.raises(ValueError, match="CUDA"):
        ops.conv_first_wgrad(torch.zeros(1, 3, 4, 5), torch.zeros(1, 4, 5, 64))
    with pytest.raises(ValueError, match="CUDA"):
        ops.pack_conv_plain_dev(torch.zeros(64, 64, 3, 3), torch.zeros(64))
