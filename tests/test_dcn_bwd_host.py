"""The native NHWC backward of the deformable conv, the host side (no GPU): stif_dcn_bwd_nhwc, its workspace size
and stif_dcn_offmask_nhwc are declared, exported and bound; the struct has the documented fields; the workspace is
stif_conv3x3_wgrad's (the weight kernel writes the same partials over the same 2 x 32 tiles with the same grid);
every invalid argument is rejected with its reason before any launch (fake pointers that are never dereferenced, one
changed argument at a time, as tests/test_pcd_train_host.py); and train.DCN_sep keeps its parameters."""
import ctypes as C
import os
import re

import pytest
import torch

import pcd_torch_ref as R  # noqa: F401  (the helper both DCN backward test files rest on)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = 4096
PART = 64 * 64 * 9 + 64

SIGS = {"stif_dcn_bwd_workspace_size": ("size_t", 3), "stif_dcn_bwd_nhwc": ("int", 2),
        "stif_dcn_offmask_nhwc": ("int", 8)}
HDR_FIELDS = ["in", "offmask", "w", "gout", "out", "g_in", "g_om", "g_w", "g_b", "in_item", "om_item", "gout_item",
              "out_item", "gin_item", "gom_item", "n", "H", "W", "epi", "workspace", "workspace_bytes"]


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
    body = re.search(r"typedef struct \{([^}]*)\} stif_dcn_bwd_args;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+)\s*[,;]", body) == HDR_FIELDS
    # the binding names the input `inp` (`in` is a Python keyword); order, count and types follow the header
    assert [f for f, _ in L.DcnBwdArgs._fields_] == ["inp"] + HDR_FIELDS[1:]
    types = [t for _, t in L.DcnBwdArgs._fields_]
    assert types == [C.c_void_p] * 9 + [C.c_longlong] * 6 + [C.c_int] * 4 + [C.c_void_p, C.c_size_t]
    a = L.DcnBwdArgs()                                       # zero-initialisable: nothing set, everything null
    assert not a.inp and not a.g_in and not a.g_b and a.n == 0 and a.epi == 0 and a.workspace_bytes == 0
    for name in ("dcn_offmask", "dcn_bwd"):
        assert callable(getattr(stif.ops, name)), name
    csrc = os.path.join(REPO, "stif-continuous-video-representation_amd", "csrc")
    assert os.path.exists(os.path.join(csrc, "dcn_bwd.hip"))
    nopk = re.search(r"^NOPK_SRC := (.*)$", open(os.path.join(REPO, "Makefile")).read(), re.M).group(1).split()
    assert "dcn_bwd" in nopk


def test_workspace_size_is_the_conv_weight_gradients(stif):
    lib = stif._lib.lib()
    size, conv = lib.stif_dcn_bwd_workspace_size, lib.stif_conv3x3_wgrad_workspace_size
    for n, H, W in ((1, 1, 1), (2, 5, 7), (1, 3, 33), (3, 33, 70), (2, 192, 192), (6, 128, 128)):
        assert size(n, H, W) == conv(n, H, W, 64, 64) > 0, (n, H, W)
        assert size(n, H, W) % (PART * 4) == 0
    assert size(2, 5, 7) == 6 * PART * 4              # 2 items x 3 x 1 tiles of 2 x 32 pixels, one partial each
    assert size(1, 1, 1) == PART * 4
    for bad in ((0, 5, 7), (2, 0, 7), (2, 5, 0), (-1, 5, 7), (2, -5, 7), (2, 5, -1)):
        assert size(*bad) == 0, bad


def bwd_args(L, **changed):
    """A valid call on fake pointers: 2 x 5 x 7, every output asked for, epi LRELU with its out."""
    a = L.DcnBwdArgs()
    a.inp, a.offmask, a.w, a.gout, a.out = A, A, A, A, A
    a.g_in, a.g_om, a.g_w, a.g_b = A, A, A, A
    a.in_item = a.gout_item = a.out_item = a.gin_item = 5 * 7 * 64
    a.om_item, a.gom_item = 5 * 7 * 216, 5 * 7 * 256
    a.n, a.H, a.W, a.epi = 2, 5, 7, L.EPI_LRELU
    a.workspace, a.workspace_bytes = A, 6 * PART * 4
    for k, v in changed.items():
        setattr(a, k, v)
    return a


def test_dcn_bwd_validates_before_launching(stif):
    L = stif._lib
    name = "stif_dcn_bwd_nhwc"
    rej = lambda text, **ch: rejected(L, name, (C.byref(bwd_args(L, **ch)), None), text, ch)
    rejected(L, name, (None, None), "null args", "args")
    for p in ("inp", "offmask", "w", "gout"):
        rej("null pointer (in, offmask, w, gout)", **{p: None})
    rej("null pointer (out with STIF_EPI_LRELU)", out=None)
    for epi in (L.EPI_RELU, L.EPI_RES, -1, 6):
        rej("epilogue must be NONE or LRELU", epi=epi)
    rej("nothing to compute", g_in=None, g_om=None, g_w=None, g_b=None)
    rej("g_b without g_w", g_w=None)
    for k in ("n", "H", "W"):
        for v in (0, -1):
            rej("must be >= 1", **{k: v})
    for k in ("in_item", "om_item", "gout_item", "out_item", "gin_item", "gom_item"):
        rej("negative item stride", **{k: -64})
    for p in ("inp", "offmask", "w", "gout", "out", "g_in", "g_om"):
        rej("16-byte aligned", **{p: A + 4})
    for k in ("in_item", "om_item", "gout_item", "out_item", "gin_item", "gom_item"):
        rej("16-byte aligned", **{k: 5 * 7 * 256 + 2})
    rej("items overlap", gin_item=5 * 7 * 64 - 4)
    rej("items overlap", gom_item=5 * 7 * 256 - 4)
    rej("items overlap", gin_item=0)
    rej("item larger than 2 GB", H=1450, W=1450, workspace_bytes=1 << 40)        # counted with the 256-float pitch
    rej("workspace too small (stif_dcn_bwd_workspace_size)", workspace=None)
    rej("workspace too small", workspace_bytes=6 * PART * 4 - 1)
    rej("workspace too small", workspace_bytes=0)
    rej("workspace not 16-byte aligned", workspace=A + 4)
    # what is not used is not looked at: out and its stride without the activation, the stride of a NULL g_in, the
    # workspace without g_w -- the call gets as far as the last check that still applies
    a = bwd_args(L, epi=L.EPI_NONE, out=None, out_item=-3, g_in=None, gin_item=-3, g_w=None, g_b=None, workspace=None,
                 workspace_bytes=0, gom_item=5 * 7 * 256 - 4)
    rejected(L, name, (C.byref(a), None), "items overlap", "unused arguments")


OMK = ["om", "offmask", "om_item", "offmask_item", "n", "H", "W", "stream"]


def test_dcn_offmask_validates_before_launching(stif):
    L = stif._lib
    base = dict(om=A, offmask=A, om_item=5 * 7 * 256, offmask_item=5 * 7 * 216, n=2, H=5, W=7, stream=None)

    def rej(text, **ch):
        assert set(ch) <= set(base)
        rejected(L, "stif_dcn_offmask_nhwc", [dict(base, **ch)[k] for k in OMK], text, ch)

    for p in ("om", "offmask"):
        rej("null pointer", **{p: None})
    for k in ("n", "H", "W"):
        for v in (0, -1):
            rej("must be >= 1", **{k: v})
    rej("negative item stride", om_item=-256)
    rej("negative item stride", offmask_item=-216)
    rej("16-byte aligned", om=A + 4)
    rej("16-byte aligned", offmask=A + 8)
    rej("16-byte aligned", om_item=5 * 7 * 256 + 2)
    rej("16-byte aligned", offmask_item=5 * 7 * 216 + 1)
    rej("items overlap", offmask_item=5 * 7 * 216 - 4)
    rej("item larger than 2 GB", H=1450, W=1450, om_item=1 << 40, offmask_item=1 << 40)


def test_ops_refuse_cpu_tensors_and_bad_shapes(stif):
    ops, L = stif.ops, stif._lib
    z = lambda *s: torch.zeros(*s)
    with pytest.raises(ValueError, match=r"\[n, H, W, 256\]"):
        ops.dcn_offmask(z(1, 4, 5, 216))
    with pytest.raises(ValueError, match="CUDA"):
        ops.dcn_offmask(z(1, 4, 5, 256), out=z(1, 4, 5, 216))
    with pytest.raises(ValueError, match="out shape"):
        ops.dcn_offmask(z(1, 4, 5, 256), out=z(1, 4, 5, 256))
    with pytest.raises(ValueError, match=r"\[n, H, W, 64\]"):
        ops.dcn_bwd(z(1, 4, 5, 64), z(1, 4, 5, 216), z(64, 64, 3, 3), z(1, 4, 6, 64))
    with pytest.raises(ValueError, match="offmask shape"):
        ops.dcn_bwd(z(1, 4, 5, 64), z(1, 4, 5, 256), z(64, 64, 3, 3), z(1, 4, 5, 64))
    with pytest.raises(ValueError, match="CUDA weight"):
        ops.dcn_bwd(z(1, 4, 5, 64), z(1, 4, 5, 216), z(64, 64, 3, 3), z(1, 4, 5, 64))


def test_dcn_sep_keeps_its_parameters_and_initialisation(stif):
    T = stif.train
    torch.manual_seed(0)
    d = T.DCN_sep("lrelu", "f32")
    assert [(k, tuple(v.shape)) for k, v in d.state_dict().items()] == [
        ("weight", (64, 64, 3, 3)), ("bias", (64,)), ("conv_offset_mask.weight", (216, 64, 3, 3)),
        ("conv_offset_mask.bias", (216,))]
    stdv = 1.0 / (64 * 9) ** 0.5
    w = d.weight.detach()
    assert 0.99 * stdv < float(w.abs().max()) <= stdv                       # uniform(-stdv, stdv), dcn_v2.py:69-75
    assert float(w.std()) == pytest.approx(stdv / 3 ** 0.5, rel=0.02)
    assert float(d.bias.detach().abs().max()) == 0.0
    assert all(float(p.detach().abs().max()) == 0.0 for p in d.conv_offset_mask.parameters())
    assert all(p.requires_grad for p in d.parameters())
    assert d.extra_repr() == "64, 64, kernel_size=(3, 3), padding=1, deformable_groups=8, act=lrelu, mfma=f32"
    with pytest.raises(RuntimeError, match="need a CUDA tensor"):
        d(torch.zeros(1, 64, 4, 5), torch.zeros(1, 64, 4, 5))
    with pytest.raises(ValueError, match="act must be"):
        T.DCN_sep(act="relu")
    # the node no longer goes through the NCHW drop-in or torch layout work
    src = open(os.path.join(REPO, "stif-continuous-video-representation_amd", "train.py")).read()
    node = src[src.index("class _DCNSepFn"):src.index("class _ConvParams")]
    for gone in ("dcn_v2_", ".contiguous()", "torch.sigmoid", "torch.zeros", "torch.where"):
        assert gone not in node, gone
