"""The trainable BiDeformableConvLSTM and gen_feat, the host side (no GPU).  First the torch reference the GPU tests
rest on (tests/lstm_torch_ref.py) is pinned to the numpy oracle (oracle.easy_pcd, conv_lstm_cell, deformable_conv_lstm,
bi_convlstm, gen_feat) to 1e-10 of max |ref|.  Then the new symbols are declared, exported and bound; every new entry
point rejects every invalid argument with its reason before any launch (fake pointers that are never dereferenced, as
tests/test_pcd_train_host.py); and the modules load the reference's state-dict slices strictly, carry nn.Conv2d's
names, shapes and initial statistics, and refuse what they cannot run."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

import lstm_torch_ref as T
from oracle import stif_oracle as O

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = 4096
PART = 64 * 64 * 9 + 64
PIN = 1e-10
H, W = 8, 12

SIGS = {"stif_lstm_gates_nhwc": ("int", 12), "stif_lstm_gates_bwd_nhwc": ("int", 16),
        "stif_conv1x1_wgrad_workspace_size": ("size_t", 4), "stif_conv1x1_wgrad": ("int", 2),
        "stif_pack_conv1x1_dev": ("int", 11)}


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

@pytest.fixture(scope="module")
def P64(sd):
    """The state dict in float64 with its recurrence tamed on the inputs below (the oracle reads the same values)."""
    P = {k: torch.from_numpy(np.asarray(v)).double().clone() for k, v in sd.items()}
    T.tame_recurrence(P, lambda calls: T.bi_convlstm(P, seq_inputs(), calls))
    return P


def seq_inputs(seed=21, B=1, n=2):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(B, 64, H, W, generator=g, dtype=torch.float64) for _ in range(n)]


def as_np(P):
    return {k: v.numpy() for k, v in P.items()}


def test_reference_easy_pcd_and_cell_match_the_oracle(P64):
    P64 = {k: v.clone() for k, v in P64.items()}                 # tamed again, on this test's own inputs
    f1, f2 = seq_inputs(5)
    p = "ConvBLSTM.forward_net.pcd_h."
    T.tame_recurrence(P64, lambda calls: T.easy_pcd(P64, p, f1, f2, calls))
    T.assert_all_tame(P64, lambda calls: T.easy_pcd(P64, p, f1, f2, calls))
    got = T.easy_pcd(P64, p, f1, f2)
    ref = O.easy_pcd(f1.numpy(), f2.numpy(), as_np(P64), p, np.float64)
    assert tuple(got.shape) == (1, 64, H, W) and rel(got, ref) < PIN, rel(got, ref)
    c = seq_inputs(6, n=1)[0]
    p = "ConvBLSTM.forward_net.cell_list.0."
    gh, gc = T.conv_lstm_cell(P64, p, f1, f2, c)
    rh, rc = O.conv_lstm_cell(f1.numpy(), f2.numpy(), c.numpy(), as_np(P64), p, np.float64)
    assert rel(gh, rh) < PIN and rel(gc, rc) < PIN, (rel(gh, rh), rel(gc, rc))


def test_reference_recurrence_matches_the_oracle(P64):
    xs = seq_inputs()
    calls = T.assert_all_tame(P64, lambda calls: T.bi_convlstm(P64, xs, calls))
    assert len(calls) == 12 and all(len(v) == 4 for v in calls.values())      # 2 Easy_PCD x 6 DCN; 2 steps x 2 ways
    sdn = as_np(P64)
    got = T.deformable_conv_lstm(P64, "ConvBLSTM.forward_net.", xs)
    ref = O.deformable_conv_lstm([x.numpy() for x in xs], sdn, "ConvBLSTM.forward_net.", np.float64)
    for g, r in zip(got, ref):
        assert rel(g, r) < PIN, rel(g, r)
    got = T.bi_convlstm(P64, xs)
    ref = O.bi_convlstm([x.numpy() for x in xs], sdn, np.float64)
    for g, r in zip(got, ref):
        assert rel(g, r) < PIN, rel(g, r)


def test_reference_gen_feat_matches_the_oracle(sd):
    P = {k: torch.from_numpy(np.asarray(v)).double().clone() for k, v in sd.items()}
    g = torch.Generator().manual_seed(9)
    x = torch.rand(1, 2, 3, H, W, generator=g, dtype=torch.float64)
    run = lambda calls: T.gen_feat(P, x, 1, 1, calls)
    T.tame_recurrence(P, run)
    calls = T.assert_all_tame(P, run)
    assert len(calls) == 18 and len(calls["pcd_align.L1_dcnpack_1"]) == 1
    got = T.gen_feat(P, x, 1, 1)
    ref = O.gen_feat(x.numpy(), as_np(P), 1, 1, np.float64)
    assert tuple(got.shape) == (1, 3, 64, H, W) and rel(got, ref) < PIN, rel(got, ref)


def test_the_recurrence_recipe_refuses_untamed_offsets():
    P = T.random_params(T.bilstm_shapes(), 3)
    xs = seq_inputs(4)
    with pytest.raises(AssertionError):
        T.assert_all_tame(P, lambda calls: T.bi_convlstm(P, xs, calls))
    T.tame_recurrence(P, lambda calls: T.bi_convlstm(P, xs, calls))
    T.assert_all_tame(P, lambda calls: T.bi_convlstm(P, xs, calls))


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
    for name in ("lstm_gates", "lstm_gates_bwd", "conv1x1_wgrad", "pack_conv1x1_dev"):
        assert callable(getattr(stif.ops, name)), name
    for name in ("Conv1x1Cat", "ConvLSTMCell", "Easy_PCD", "DeformableConvLSTM", "BiDeformableConvLSTM", "GenFeat",
                 "gen_feat_state_dict"):
        assert callable(getattr(stif.train, name)), name
    mk = open(os.path.join(REPO, "Makefile")).read()
    nopk = re.search(r"^NOPK_SRC := (.*)$", mk, re.M).group(1).split()
    assert "lstm" in nopk and "conv1x1_bwd" in nopk


def test_workspace_sizes_of_the_widened_and_new_forms(stif):
    lib = stif._lib.lib()
    cat, one, c1 = (lib.stif_conv3x3_wgrad_cat_workspace_size, lib.stif_conv3x3_wgrad_workspace_size,
                    lib.stif_conv1x1_wgrad_workspace_size)
    for n, h, w in ((1, 1, 1), (2, 5, 7), (1, 3, 33), (3, 33, 70), (6, 128, 128)):
        base = one(n, h, w, 64, 64)
        assert base > 0 and cat(n, h, w, 2, 256, 256) == 8 * base, (n, h, w)
        assert cat(n, h, w, 2, 64, 64) == 2 * base and cat(n, h, w, 1, 256, 216) == 4 * base
    for bad in ((1, 256, 256), (2, 256, 216), (2, 256, 64), (3, 256, 256), (2, 128, 256)):
        assert cat(2, 5, 7, *bad) == 0, bad
    # one partial [64][64 nx] + 64 per workgroup, one workgroup per 64 pixels of an item until the grid is full
    assert c1(2, 5, 7, 1) == 2 * (64 * 64 + 64) * 4 and c1(2, 5, 7, 2) == 2 * (64 * 128 + 64) * 4
    assert c1(1, 1, 1, 2) == (64 * 128 + 64) * 4
    big = c1(6, 128, 128, 2)
    assert big % ((64 * 128 + 64) * 4) == 0 and big == c1(12, 128, 128, 2)      # the grid is capped by the CU count
    for bad in ((0, 5, 7, 1), (2, 0, 7, 1), (2, 5, -1, 2), (2, 5, 7, 0), (2, 5, 7, 3)):
        assert c1(*bad) == 0, bad


GATES = ["pre", "c_cur", "h_next", "c_next", "n", "H", "W", "pre_item", "c_item", "h_item", "cn_item", "stream"]
GATES_BWD = ["pre", "c_cur", "g_h", "g_c_next", "g_pre", "g_c_cur", "n", "H", "W", "pre_item", "c_item", "gh_item",
             "gcn_item", "gpre_item", "gcc_item", "stream"]


def test_lstm_gates_validate_before_launching(stif):
    L = stif._lib
    px = 5 * 7
    base = dict(pre=A, c_cur=A, h_next=A, c_next=A, n=2, H=5, W=7, pre_item=px * 256, c_item=px * 64, h_item=px * 64,
                cn_item=px * 64, stream=None)

    def rej(text, **ch):
        assert set(ch) <= set(base)
        rejected(L, "stif_lstm_gates_nhwc", [dict(base, **ch)[k] for k in GATES], text, ch)

    for p in ("pre", "c_cur", "h_next", "c_next"):
        rej("null pointer", **{p: None})
        rej("16-byte aligned", **{p: A + 4})
    for k in ("n", "H", "W"):
        for v in (0, -1):
            rej("must be >= 1", **{k: v})
    for k in ("pre_item", "c_item", "h_item", "cn_item"):
        rej("negative item stride", **{k: -64})
        rej("16-byte aligned", **{k: base[k] + 2})
    rej("item larger than 2 GB", H=1450, W=1450)
    rej("output items overlap", h_item=px * 64 - 4)
    rej("output items overlap", cn_item=0)


def test_lstm_gates_backward_validates_before_launching(stif):
    L = stif._lib
    px = 5 * 7
    base = dict(pre=A, c_cur=A, g_h=A, g_c_next=A, g_pre=A, g_c_cur=A, n=2, H=5, W=7, pre_item=px * 256,
                c_item=px * 64, gh_item=px * 64, gcn_item=px * 64, gpre_item=px * 256, gcc_item=px * 64, stream=None)

    def rej(text, **ch):
        assert set(ch) <= set(base)
        rejected(L, "stif_lstm_gates_bwd_nhwc", [dict(base, **ch)[k] for k in GATES_BWD], text, ch)

    for p in ("pre", "c_cur", "g_pre"):
        rej("null pointer", **{p: None})
    rej("both null", g_h=None, g_c_next=None)
    for p in ("pre", "c_cur", "g_h", "g_c_next", "g_pre", "g_c_cur"):
        rej("16-byte aligned", **{p: A + 8})
    for k in ("n", "H", "W"):
        for v in (0, -1):
            rej("must be >= 1", **{k: v})
    for k in ("pre_item", "c_item", "gh_item", "gcn_item", "gpre_item", "gcc_item"):
        rej("negative item stride", **{k: -64})
        rej("16-byte aligned", **{k: base[k] + 1})
    rej("item larger than 2 GB", H=1450, W=1450)
    rej("output items overlap", gpre_item=px * 256 - 4)
    rej("output items overlap", gcc_item=px * 64 - 4)
    # a null optional map's stride is not looked at, and a null g_c_cur cannot overlap: the next check speaks
    rej("output items overlap", g_h=None, gh_item=-3, g_c_cur=None, gcc_item=-3, gpre_item=0)
    rej("output items overlap", g_c_next=None, gcn_item=-2, g_c_cur=None, gcc_item=2, gpre_item=0)


def c1_args(L, **changed):
    a = L.ConvWgradCatArgs()
    a.x[0], a.x[1], a.gy, a.gw, a.gb = A, A, A, A, A
    a.x_item[0], a.x_item[1], a.gy_item = 5 * 7 * 64, 5 * 7 * 64, 5 * 7 * 64
    a.n, a.H, a.W, a.nx, a.gy_channels, a.cout = 2, 5, 7, 2, 64, 64
    a.workspace, a.workspace_bytes = A, 2 * (64 * 128 + 64) * 4
    for k, v in changed.items():
        if k[-1] in "01" and k[:-1] in ("x", "x_item"):
            getattr(a, k[:-1])[int(k[-1])] = v
        else:
            setattr(a, k, v)
    return a


def test_conv1x1_wgrad_validates_before_launching(stif):
    L = stif._lib
    name = "stif_conv1x1_wgrad"
    rej = lambda text, **ch: rejected(L, name, (C.byref(c1_args(L, **ch)), None), text, ch)
    rejected(L, name, (None, None), "null args", "args")
    for p in ("x0", "gy", "gw"):
        rej("null pointer", **{p: None})
    rej("null pointer (x[1]", x1=None)
    for k in ("n", "H", "W"):
        for v in (0, -1):
            rej("must be >= 1", **{k: v})
    for ch in (dict(nx=0), dict(nx=3), dict(gy_channels=256), dict(cout=216), dict(gy_channels=256, cout=256)):
        rej("unsupported channel counts", **ch)
    for k in ("x_item0", "x_item1", "gy_item"):
        rej("negative item stride", **{k: -64})
        rej("16-byte aligned", **{k: 5 * 7 * 64 + 2})
    for p in ("x0", "x1", "gy"):
        rej("16-byte aligned", **{p: A + 4})
    rej("item larger than 2 GB", H=2900, W=2900, workspace_bytes=1 << 40)
    rej("workspace too small", workspace=None)
    rej("workspace too small", workspace_bytes=2 * (64 * 128 + 64) * 4 - 1)
    rej("workspace too small", workspace_bytes=2 * (64 * 64 + 64) * 4)          # the one-map form's size
    rej("workspace not 16-byte aligned", workspace=A + 4)
    a = c1_args(L, nx=1, x1=None, x_item1=-3, gy=None)                          # one map: x[1] is not looked at
    rejected(L, name, (C.byref(a), None), "null pointer (x[0], gy, gw)", "nx = 1")


P1 = ["w_oihw", "b", "cout", "cin", "ci0", "mode", "flags", "w_dst", "b_dst", "status", "stream"]


def test_conv1x1_packer_validates_before_launching(stif):
    L = stif._lib
    base = dict(w_oihw=A, b=A, cout=64, cin=128, ci0=0, mode=L.PACK_PLAIN | L.PACK_F16X3, flags=0, w_dst=A, b_dst=A,
                status=A, stream=None)

    def rej(text, **ch):
        assert set(ch) <= set(base)
        rejected(L, "stif_pack_conv1x1_dev", [dict(base, **ch)[k] for k in P1], text, ch)

    for p in ("w_oihw", "w_dst", "b_dst"):
        rej("null pointer", **{p: None})
    for mode in (L.PACK_WINO, L.PACK_WINO | L.PACK_F16X3, L.PACK_LSTM, L.PACK_OFFMASK):
        rej("unsupported mode", mode=mode)
    for ch in (dict(cout=128), dict(cin=64), dict(cin=256), dict(cout=256), dict(cout=0)):
        rej("unsupported channel counts", **ch)
    rej("unknown flags", flags=2)
    rej("fp32 layer", flags=L.PACK_DGRAD)                                          # DGRAD with the f16x3 mode
    for ci0 in (64, 32, -64):
        rej("ci0 must be", ci0=ci0)                                                # the forward pack is the whole layer
    for ci0 in (32, 128, -64):
        rej("ci0 must be", ci0=ci0, mode=L.PACK_PLAIN, flags=L.PACK_DGRAD)
    rej("null bias", b=None)
    rej("status word", status=None)


def test_the_block_entry_points_admit_the_cell_and_nothing_more(stif):
    L = stif._lib
    a = L.ConvWgradCatArgs()
    a.x[0], a.x[1], a.gy, a.gw, a.gb = A, A, A, A, A
    a.x_item[0], a.x_item[1], a.gy_item = 5 * 7 * 64, 5 * 7 * 64, 5 * 7 * 256
    a.n, a.H, a.W, a.nx, a.gy_channels, a.cout = 2, 5, 7, 2, 256, 256
    a.workspace, a.workspace_bytes = A, 8 * 6 * PART * 4 - 1                       # 8 blocks x 6 tiles, one byte short:
    rejected(L, "stif_conv3x3_wgrad_cat", (C.byref(a), None), "workspace too small", "cell")   # the shape was admitted
    a.H, a.W, a.workspace_bytes = 1450, 1450, 1 << 40
    rejected(L, "stif_conv3x3_wgrad_cat", (C.byref(a), None), "item larger than 2 GB", "cell")
    blk = lambda **ch: [dict(dict(w_oihw=A, b=A, cout=256, cin=128, co0=0, ci0=0, mode=L.PACK_WINO, flags=0, w_dst=A,
                                  b_dst=A, status=None, stream=None), **ch)[k]
                        for k in ("w_oihw", "b", "cout", "cin", "co0", "ci0", "mode", "flags", "w_dst", "b_dst",
                                  "status", "stream")]
    name = "stif_pack_conv_block_dev"
    rejected(L, name, blk(b=None), "null bias", "the [256, 128] weight is admitted")
    rejected(L, name, blk(co0=256), "multiples of 64 inside the weight", "co0")
    rejected(L, name, blk(co0=192, ci0=128), "multiples of 64 inside the weight", "ci0")
    for ch in (dict(cin=64), dict(cin=256), dict(cout=128), dict(cout=216, cin=256)):
        rejected(L, name, blk(**ch), "unsupported channel counts", ch)
    z = lambda *s: torch.zeros(*s)
    with pytest.raises(ValueError, match="unsupported channel counts"):
        stif.ops.conv3x3_wgrad_cat([z(1, 4, 5, 64)], z(1, 4, 5, 256), 256)
    for fn, args in ((stif.ops.conv1x1_wgrad, ([z(1, 4, 5, 64)], z(1, 4, 5, 64))),
                     (stif.ops.pack_conv1x1_dev, (z(64, 128, 1, 1), z(64))),
                     (stif.ops.lstm_gates, (z(1, 4, 5, 256), z(1, 4, 5, 64))),
                     (stif.ops.lstm_gates_bwd, (z(1, 4, 5, 256), z(1, 4, 5, 64), z(1, 4, 5, 64), None))):
        with pytest.raises(ValueError, match="CUDA"):
            fn(*args)


# ---- the modules ----

def spec_slice(prefix="", drop=()):
    spec = json.load(open(os.path.join(REPO, "tests", "golden", "state_dict_spec.json")))
    return [(k[len(prefix):], tuple(s)) for k, s in spec if k.startswith(prefix) and not k.startswith(drop)]


def test_bilstm_loads_the_reference_slice_strictly(stif, sd):
    net = stif.train.BiDeformableConvLSTM()
    pre = "ConvBLSTM."
    part = {k[len(pre):]: torch.from_numpy(v) for k, v in sd.items() if k.startswith(pre)}
    assert len(part) == 2 * 74 + 4
    net.load_state_dict(part, strict=True)
    got = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
    assert got == spec_slice(pre)                                  # names, shapes and registration order
    assert got == [(k[len(pre):], s) for k, s in T.bilstm_shapes().items()]
    for k, v in net.state_dict().items():
        assert torch.equal(v, part[k]), k
    assert [n for n, _ in net.forward_net.named_children()] == ["cell_list", "pcd_h", "pcd_c"]
    assert [n for n, _ in net.forward_net.pcd_h.named_children()] == [
        "fea_L2_conv1", "fea_L2_conv2", "fea_L3_conv1", "fea_L3_conv2", "pcd_align", "fusion"]


def test_gen_feat_loads_the_non_decoder_slice_strictly(stif, sd):
    TR = stif.train
    net = TR.GenFeat(5, 40)
    part = TR.gen_feat_state_dict(sd)
    assert len(part) == 408 and len(sd) == 442                # 34 decoder and unused-upsampling keys stay out
    assert set(sd) - set(part) == {k for k in sd if k.split(".")[0] in (
        "feat_imnet", "flow_imnet", "encode_imnet", "upconv1", "upconv2", "HRconv", "conv_last")}
    net.load_state_dict(part, strict=True)
    drop = ("feat_imnet.", "flow_imnet.", "encode_imnet.", "upconv1.", "upconv2.", "HRconv.", "conv_last.")
    got = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
    assert got == spec_slice("", drop)
    assert got == list(T.gen_feat_shapes(5, 40).items())
    for k, v in net.state_dict().items():
        assert torch.equal(v, part[k]), k
    small = TR.GenFeat(front_RBs=1, back_RBs=2, mfma="f32")
    assert [(k, tuple(v.shape)) for k, v in small.state_dict().items()] == list(T.gen_feat_shapes(1, 2).items())


def uniform_stats(t, bound):
    t = t.detach()
    return (0.98 * bound < float(t.abs().max()) <= bound and abs(float(t.mean())) < 0.05 * bound
            and float(t.std()) == pytest.approx(bound / 3 ** 0.5, rel=0.03))


def test_parameter_names_shapes_and_initial_values(stif):
    TR = stif.train
    torch.manual_seed(0)
    c = TR.Conv1x1Cat()
    ref = torch.nn.Conv2d(128, 64, 1)
    assert [(k, tuple(v.shape)) for k, v in c.state_dict().items()] == [
        (k, tuple(v.shape)) for k, v in ref.state_dict().items()]
    c.load_state_dict(ref.state_dict(), strict=True)
    # nn.Conv2d's default, kaiming_uniform(a = sqrt 5): weight and bias uniform in +-1 / sqrt(fan_in)
    assert uniform_stats(TR.Conv1x1Cat().weight, 1.0 / 128 ** 0.5)
    assert float(TR.Conv1x1Cat().bias.detach().abs().max()) <= 1.0 / 128 ** 0.5
    cell = TR.ConvLSTMCell()
    ref = torch.nn.Conv2d(128, 256, 3, 1, 1)
    assert [(k, tuple(v.shape)) for k, v in cell.state_dict().items()] == [
        ("conv." + k, tuple(v.shape)) for k, v in ref.state_dict().items()]
    bound = 1.0 / (128 * 9) ** 0.5
    assert uniform_stats(cell.conv.weight, bound)
    assert 0.9 * bound < float(cell.conv.bias.detach().abs().max()) <= bound       # 256 draws
    assert uniform_stats(ref.weight, bound)                       # the yardstick itself
    assert all(p.requires_grad for p in TR.BiDeformableConvLSTM().parameters())


def test_modules_refuse_cpu_tensors_bad_sizes_and_bad_choices(stif):
    TR = stif.train
    z = lambda *s: torch.zeros(*s)
    with pytest.raises(RuntimeError, match="need a CUDA tensor"):
        TR.Conv1x1Cat()(z(1, 64, 4, 5), z(1, 64, 4, 5))
    with pytest.raises(RuntimeError, match="need a CUDA tensor"):
        TR.ConvLSTMCell()(z(1, 64, 4, 5), (z(1, 64, 4, 5), z(1, 64, 4, 5)))
    with pytest.raises(RuntimeError, match="need a CUDA tensor"):
        TR.Easy_PCD()(z(1, 64, 8, 12), z(1, 64, 8, 12))
    with pytest.raises(RuntimeError, match="need a CUDA tensor"):
        TR.DeformableConvLSTM()(z(1, 2, 64, 8, 12))
    with pytest.raises(RuntimeError, match="need a CUDA tensor"):
        TR.BiDeformableConvLSTM()(z(1, 2, 64, 8, 12))
    with pytest.raises(RuntimeError, match="need a CUDA tensor"):
        TR.GenFeat(1, 1)(z(1, 2, 3, 8, 12))
    for h, w in ((6, 12), (8, 10), (9, 12)):
        with pytest.raises(ValueError, match="multiples of 4"):
            TR.Easy_PCD()(z(1, 64, h, w), z(1, 64, h, w))
        with pytest.raises(ValueError, match="multiples of 4"):
            TR.BiDeformableConvLSTM()(z(1, 2, 64, h, w))
        with pytest.raises(ValueError, match="multiples of 4"):
            TR.GenFeat(1, 1)(z(1, 2, 3, h, w))
    with pytest.raises(ValueError, match="expected"):
        TR.Easy_PCD()(z(1, 32, 8, 12), z(1, 32, 8, 12))
    with pytest.raises(ValueError, match="expected"):
        TR.BiDeformableConvLSTM()(z(1, 2, 128, 8, 12))
    with pytest.raises(ValueError, match="expected"):
        TR.BiDeformableConvLSTM()(z(2, 64, 8, 12))
    with pytest.raises(ValueError, match="expected"):
        TR.GenFeat(1, 1)(z(1, 2, 4, 8, 12))
    with pytest.raises(ValueError, match="expected"):
        TR.GenFeat(1, 1)(z(1, 1, 3, 8, 12))
    for mk in (TR.Conv1x1Cat, TR.ConvLSTMCell, TR.Easy_PCD, TR.DeformableConvLSTM, TR.BiDeformableConvLSTM):
        with pytest.raises(ValueError, match="mfma must be"):
            mk(mfma="bf16")
    with pytest.raises(ValueError, match="mfma must be"):
        TR.GenFeat(1, 1, mfma="bf16")
