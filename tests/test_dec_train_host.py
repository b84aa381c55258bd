"""The trainable SIREN decoder and the whole-model ``train.LunaTokis``, the host side (no GPU).  First the torch
reference the GPU tests rest on (tests/dec_torch_ref.py) is pinned to the numpy oracle (oracle.decode_stage1,
decode_stage2, decoding) to 1e-10 of max |ref|.  Then the new symbols are declared, exported and bound; every new
entry point rejects every invalid argument with its reason before any launch (fake pointers that are never
dereferenced, as tests/test_lstm_train_host.py); and the modules carry the reference's 26 / 442 keys, load its state
dict strictly, initialise the SIRENs within the reference's bounds and refuse what they cannot run."""
import ctypes as C
import json
import math
import os
import re

import numpy as np
import pytest
import torch

import dec_torch_ref as R
from oracle import stif_oracle as O

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = 4096
PIN = 1e-10
SIZES = [(2, 5, 7, 11, 13), (1, 16, 20, 40, 50)]

SIGS = {"stif_siren_fwd": ("int", 2), "stif_siren_bwd": ("int", 2), "stif_siren_bwd_workspace_size": ("size_t", 2),
        "stif_siren_wgrad_grid": ("int", 3), "stif_dec_x1_fwd": ("int", 3), "stif_dec_x1_bwd": ("int", 4),
        "stif_dec_x2_fwd": ("int", 4), "stif_dec_x2_bwd": ("int", 5), "stif_dec_x3_fwd": ("int", 5),
        "stif_dec_x3_bwd": ("int", 8)}


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

def case(B, H, W, seed=3):
    g = torch.Generator().manual_seed(seed)
    feat = torch.randn(B, 3, 64, H, W, generator=g, dtype=torch.float64) * 0.5
    inp = torch.rand(B, 2, 3, H, W, generator=g, dtype=torch.float64)
    return feat, inp, g


@pytest.mark.parametrize("B,H,W,HH,WW", SIZES)
def test_reference_stages_match_the_oracle(sd, B, H, W, HH, WW):
    feat, inp, g = case(B, H, W)
    P = {k: torch.as_tensor(np.asarray(v)).double() for k, v in sd.items() if "imnet" in k}
    t = torch.linspace(0.25, 0.75, B, dtype=torch.float64)
    s1 = R.decode_stage1(feat, inp, t, P, HH, WW)
    hr, fl = O.decode_stage1(feat.numpy(), inp.numpy(), t.numpy(), sd, HH, WW)
    assert rel(s1["hrfeat"].reshape(B, HH, WW, 64), hr) < PIN and rel(s1["flow"].reshape(B, HH, WW, 4), fl) < PIN
    # stage 2 from a given flow of several pixels, some of it clamped at the frame edge
    hrfeat = torch.randn(B, HH * WW, 64, generator=g, dtype=torch.float64)
    flow = torch.randn(B, HH * WW, 4, generator=g, dtype=torch.float64) * 2.5
    s2 = R.decode_stage2(feat, inp, hrfeat, flow, t, P, HH, WW)
    assert bool(((s2["ux"] < R.LO) | (s2["ux"] > R.HI)).any())
    ref = O.decode_stage2(feat.numpy(), inp.numpy(), hrfeat.numpy(), flow.numpy(), t.numpy(), sd, HH, WW)
    assert tuple(s2["pred"].shape) == (B, 3, HH, WW) and rel(s2["pred"], ref) < PIN, rel(s2["pred"], ref)
    assert tuple(s1["x1"].shape) == (B, HH * WW, 201) and tuple(s1["x2"].shape) == (B, HH * WW, 263)
    assert tuple(s2["x3"].shape) == (B, HH * WW, 525)


@pytest.mark.parametrize("B,H,W,HH,WW", SIZES)
def test_reference_decoding_matches_the_oracle(sd, B, H, W, HH, WW):
    feat, inp, _ = case(B, H, W, 4)
    got, mids = R.decoding(feat, inp, [0.5, 0.25], sd, (HH, WW))
    cap = {}
    ref = O.decoding(feat.numpy(), inp.numpy(), [0.5, 0.25], sd, (HH, WW), capture=cap)
    for i in range(2):
        assert rel(got[i], ref[i]) < PIN, rel(got[i], ref[i])
        assert rel(mids[i]["hrfeat"], cap["hrfeat"][i]) < PIN and rel(mids[i]["flow"], cap["flow"][i]) < PIN
    if (H, W) == (5, 7):
        ref4 = O.decoding(feat.numpy(), inp.numpy(), [0.5], sd)
        got4 = R.decoding(feat, inp, [0.5], sd)[0]
        assert tuple(got4[0].shape) == (B, 3, 20, 28) and rel(got4[0], ref4[0]) < PIN


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
    for name in ("siren_fwd", "siren_bwd", "DecTrainGeom", "dec_x1_fwd", "dec_x1_bwd", "dec_x2_fwd", "dec_x2_bwd",
                 "dec_x3_fwd", "dec_x3_bwd"):
        assert callable(getattr(stif.ops, name)), name
    for name in ("Siren", "Decoder", "LunaTokis", "TimesLoss"):
        assert callable(getattr(stif.train, name)), name
    mk = open(os.path.join(REPO, "Makefile")).read()
    nopk = re.search(r"^NOPK_SRC := (.*)$", mk, re.M).group(1).split()
    assert "siren_train" in nopk and "dec_train" in nopk
    assert L.SIREN_ROW_TILE == int(re.search(r"#define STIF_SIREN_ROW_TILE (\d+)", hdr).group(1))
    # the struct bindings have the header's fields, in order
    for struct, cls in (("stif_siren_args", L.SirenArgs), ("stif_dec_train_geom", L.DecTrainGeom)):
        body = re.search(r"typedef struct \{([^}]*)\} %s;" % struct, hdr).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = []
        for decl in body.split(";"):
            names += [re.sub(r"\[.*", "", n.strip().lstrip("*")) for n in re.sub(r"^.*?[\w*]\s+\**(?=\w+[\[,]|\w+\s*$)",
                                                                                 "", decl.strip()).split(",") if n.strip()]
        assert names == [f[0] for f in cls._fields_], (struct, names)


def test_workspace_size_and_the_weight_pass_launch_rule(stif):
    lib = stif._lib.lib()
    ws, grid = lib.stif_siren_bwd_workspace_size, lib.stif_siren_wgrad_grid
    part = (64 * 64 + 64) * 4
    for n in (1, 63, 65, 5000):
        w3, w4 = ws(n, 3), ws(n, 4)
        assert w3 > n * 384 * 4 and w4 - w3 == n * 256 * 4 and (w3 - n * 384 * 4) % part == 0
    for bad in ((0, 3), (-1, 4), (5, 2), (5, 5)):
        assert ws(*bad) == 0, bad
    # one workgroup per 64-row chunk until the layer's share of the grid is full; a function of n and the shape only
    assert grid(1, 64, 64) == 1 and grid(64, 64, 64) == 1 and grid(65, 64, 64) == 2 and grid(640, 256, 256) == 10
    cap = grid(10 ** 7, 64, 64)
    assert cap == grid(2 * 10 ** 7, 64, 64) and cap >= grid(10 ** 7, 64, 525) >= grid(10 ** 7, 256, 256) >= 1
    # every layer's partials fit the workspace: blocks x grid partials after the g_z of the sine layers
    for n in (1, 100, 10 ** 6):
        for co, ci in ((64, 201), (64, 263), (64, 525), (64, 64), (256, 64), (256, 256), (64, 256), (4, 256), (3, 256)):
            blocks = ((co + 63) // 64) * ((ci + 63) // 64)
            assert blocks * grid(n, co, ci) * part <= ws(n, 3) - n * 384 * 4, (n, co, ci)
    for bad in ((0, 64, 64), (5, 0, 64), (5, 257, 64), (5, 64, 0), (5, 64, 529)):
        assert grid(*bad) == 0, bad


def siren_args(L, nsine=3, cin=201, cout=64, n=100):
    a = L.SirenArgs()
    kp = (cin + 7) // 8 * 8
    a.x, a.x_stride, a.n, a.cin, a.nsine, a.cout = A, kp, n, cin, nsine, cout
    for l, w in enumerate((64, 64, 256, 256)[:nsine]):
        a.width[l] = w
    for l in range(nsine + 1):
        a.w[l], a.b[l], a.g_w[l], a.g_b[l] = A * (2 + l), A * (8 + l), A * (16 + l), A * (24 + l)
    a.y, a.z, a.g_y, a.g_x, a.gx_stride = A * 32, A * 33, A * 34, A * 35, kp
    a.workspace, a.workspace_bytes = A * 64, L.lib().stif_siren_bwd_workspace_size(n, nsine)
    return a


SIREN_BAD = [
    (dict(x=None), "null pointer (x, z)"), (dict(z=None), "null pointer (x, z)"),
    (dict(n=0), "n must be >= 1"), (dict(n=-3), "n must be >= 1"),
    (dict(nsine=2), "nsine must be 3 or 4"), (dict(nsine=5), "nsine must be 3 or 4"),
    (dict(width=(64, 64, 128, 0)), "unsupported widths"), (dict(width=(64, 64, 256, 256)), "unsupported widths"),
    (dict(width=(32, 64, 256, 0)), "unsupported widths"),
    (dict(cout=5), "cout must be 64, 4 or 3"), (dict(cout=0), "cout must be 64, 4 or 3"),
    (dict(cout=256), "cout must be 64, 4 or 3"),
    (dict(cin=0), "cin outside"), (dict(cin=529), "cin outside"),
    (dict(x_stride=212), "x_stride must be a multiple of 8"), (dict(x_stride=200), "x_stride must be a multiple of 8"),
    (dict(x=A + 4), "16-byte aligned"), (dict(z=A + 8), "16-byte aligned"),
    (dict(w=(0, None)), "null pointer (w[l], b[l])"), (dict(w=(3, None)), "null pointer (w[l], b[l])"),
    (dict(b=(2, None)), "null pointer (w[l], b[l])"),
]
SIREN_BAD_FWD = [(dict(y=None), "null pointer (y)")]
SIREN_BAD_BWD = [
    (dict(g_y=None), "null pointer (g_y)"), (dict(g_w=(1, None)), "null pointer (g_w[l], g_b[l])"),
    (dict(g_b=(3, None)), "null pointer (g_w[l], g_b[l])"),
    (dict(gx_stride=204), "gx_stride must be a multiple of 8"), (dict(gx_stride=8), "gx_stride must be a multiple of 8"),
    (dict(g_x=A + 4), "g_x must be 16-byte aligned"),
    (dict(workspace=None), "workspace too small"), (dict(workspace_bytes=1000), "workspace too small"),
    (dict(workspace=A + 4), "workspace not 16-byte aligned"),
]


def apply_change(a, ch):
    for k, v in ch.items():
        if k in ("w", "b", "g_w", "g_b"):
            getattr(a, k)[v[0]] = v[1]
        elif k == "width":
            for i, w in enumerate(v):
                a.width[i] = w
        else:
            setattr(a, k, v)
    return a


def test_siren_entry_points_validate_before_launching(stif):
    L = stif._lib
    for name, extra in (("stif_siren_fwd", SIREN_BAD_FWD), ("stif_siren_bwd", SIREN_BAD_BWD)):
        rejected(L, name, [None, None], "null args", "null args")
        for ch, text in SIREN_BAD + extra:
            rejected(L, name, [C.byref(apply_change(siren_args(L), ch)), None], text, ch)
        # the four-layer net has its own width list
        rejected(L, name, [C.byref(apply_change(siren_args(L, 4, 525, 3), dict(width=(64, 64, 256, 0)))), None],
                 "unsupported widths", "nsine 4 with three widths")
    # g_x = NULL is a form of the backward, not an error: its stride is then not looked at (the next check fails)
    a = apply_change(siren_args(L), dict(g_x=None, gx_stride=3, workspace=None))
    rejected(L, "stif_siren_bwd", [C.byref(a), None], "workspace too small", "g_x NULL")


def geom(L, B=2, H=5, W=7, HH=11, WW=13):
    g = L.DecTrainGeom()
    g.B, g.H, g.W, g.HH, g.WW = B, H, W, HH, WW
    for i, (n, _) in enumerate(L.DecTrainGeom._fields_[5:]):
        setattr(g, n, A * (i + 1))
    return g


DEC_CALLS = {"stif_dec_x1_fwd": 1, "stif_dec_x1_bwd": 2, "stif_dec_x2_fwd": 2, "stif_dec_x2_bwd": 3,
             "stif_dec_x3_fwd": 3, "stif_dec_x3_bwd": 6}


def test_builder_entry_points_validate_before_launching(stif):
    L = stif._lib
    fields = [n for n, _ in L.DecTrainGeom._fields_[5:]]
    for name, nptr in DEC_CALLS.items():
        ptrs = [A * (40 + i) for i in range(nptr)]
        rejected(L, name, [None] + ptrs + [None], "null geometry", "null geometry")
        for f in fields:
            g = geom(L)
            setattr(g, f, None)
            text = ("null pointer (feat, frames, t)" if f in ("feat", "frames", "t") else
                    "null inverse table pointer" if f.endswith("_first") else "null table pointer")
            rejected(L, name, [C.byref(g)] + ptrs + [None], text, f)
        for ch, text in ((dict(B=0), "B, H, W must be >= 1"), (dict(H=0), "B, H, W must be >= 1"),
                         (dict(W=-1), "B, H, W must be >= 1"), (dict(HH=1), "HH and WW must be >= 2"),
                         (dict(WW=1), "HH and WW must be >= 2"), (dict(HH=0), "HH and WW must be >= 2"),
                         (dict(B=64, HH=4096, WW=4096), "more than 2^31 - 1 float4")):
            g = geom(L)
            for k, v in ch.items():
                setattr(g, k, v)
            rejected(L, name, [C.byref(g)] + ptrs + [None], text, ch)
        for i in range(nptr):
            bad = list(ptrs)
            bad[i] = None
            rejected(L, name, [C.byref(geom(L))] + bad + [None], "null pointer (", (name, i))


def test_inverse_tables_invert_the_monotone_tables(stif):
    Cc = stif.coords
    for h, w, HH, WW in ((1, 1, 3, 2), (5, 7, 11, 13), (4, 4, 16, 16), (8, 12, 16, 24), (16, 20, 40, 50)):
        t = Cc.dec_train_tables(h, w, HH, WW)
        assert set(t) == set(stif._lib.DEC_TRAIN_TABLES)
        for ax, n, N in (("y", h, HH), ("x", w, WW)):
            for k in (f"near_{ax}", f"b{ax}0", f"b{ax}1"):
                tab, first = t[k], t[k + "_first"]
                assert first.dtype == np.int32 and len(first) == n + 1 and first[0] == 0 and first[-1] == N
                for i in range(n):
                    assert (tab[first[i]:first[i + 1]] == i).all() and (tab == i).sum() == first[i + 1] - first[i]
    with pytest.raises(ValueError):
        Cc.first_index(np.array([0, 2, 1]), 3)


# ---- the modules ----

def spec():
    return json.load(open(os.path.join(REPO, "tests", "golden", "state_dict_spec.json")))


def test_decoder_and_lunatokis_carry_the_reference_keys(stif, sd):
    T = stif.train
    full = spec()
    dec_keys = [(k, s) for k, s in full if k.startswith(("feat_imnet.", "flow_imnet.", "encode_imnet."))]
    assert len(full) == 442 and len(dec_keys) == 26
    dec = T.Decoder()
    got = [(k, list(v.shape)) for k, v in dec.state_dict().items()]
    assert got == dec_keys
    assert [k for k, _ in dec.named_parameters()] == [k for k, _ in dec_keys]
    dec.load_state_dict({k: torch.as_tensor(np.asarray(sd[k])) for k, _ in dec_keys}, strict=True)
    net = T.LunaTokis()
    assert [(k, list(v.shape)) for k, v in net.state_dict().items()] == [(k, list(s)) for k, s in full]
    assert len(list(net.parameters())) == 442 and all(p.requires_grad for p in net.parameters())
    net.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in sd.items()}, strict=True)
    for k, v in net.state_dict().items():
        assert np.array_equal(v.numpy(), np.asarray(sd[k])), k
    missing = dict(sd)
    del missing["encode_imnet.net.4.bias"]
    with pytest.raises(RuntimeError):
        net.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in missing.items()}, strict=True)
    # GenFeat's own slice is what remains without the decoder and the unused layers
    assert set(T.gen_feat_state_dict(sd)) == {k for k, _ in full} - {k for k, _ in dec_keys} - {
        k for k, _ in full if k.startswith(("upconv1.", "upconv2.", "HRconv.", "conv_last."))}


def test_siren_initialisation_is_the_references(stif):
    T = stif.train
    torch.manual_seed(7)
    for cin, hidden, cout in ((201, (64, 64, 256), 64), (263, (64, 64, 256), 4), (525, (64, 64, 256, 256), 3)):
        net = T.Siren(cin, list(hidden), cout)
        dims = (cin,) + hidden + (cout,)
        mods = [m.linear for m in net.net[:-1]] + [net.net[-1]]
        assert len(mods) == len(hidden) + 1
        for l, m in enumerate(mods):
            fan = dims[l]
            assert tuple(m.weight.shape) == (dims[l + 1], fan) and tuple(m.bias.shape) == (dims[l + 1],)
            bound = 1.0 / fan if l == 0 else math.sqrt(6.0 / fan) / 30.0          # SIREN.py:39-45, :70-71
            w = m.weight.detach()
            assert float(w.abs().max()) <= bound
            if w.numel() >= 768:      # enough samples for the moments of U(-bound, bound)
                assert float(w.abs().max()) > 0.97 * bound
                assert abs(float(w.std()) / (bound / math.sqrt(3)) - 1) < 0.06 and abs(float(w.mean())) < 0.08 * bound
            bb = 1.0 / math.sqrt(fan)                                              # nn.Linear's default bias
            assert float(m.bias.detach().abs().max()) <= bb
            if m.bias.numel() >= 64:
                assert float(m.bias.detach().abs().max()) > 0.8 * bb
    for bad in ((201, (64, 64), 64), (201, (64, 64, 128), 64), (201, (64, 64, 256), 5), (0, (64, 64, 256), 3),
                (529, (64, 64, 256, 256), 3)):
        with pytest.raises(ValueError):
            T.Siren(*bad)


def test_modules_refuse_what_they_cannot_run(stif):
    T = stif.train
    dec = T.Decoder()
    feat, inp = torch.zeros(1, 3, 64, 4, 4), torch.zeros(1, 2, 3, 4, 4)
    with pytest.raises(RuntimeError, match="CUDA"):
        dec(feat, inp, [0.5])
    with pytest.raises(RuntimeError, match="CUDA"):
        dec.feat_imnet(torch.zeros(5, 201))
    for bad_feat, bad_inp in ((torch.zeros(1, 3, 32, 4, 4), inp), (torch.zeros(1, 2, 64, 4, 4), inp),
                              (feat, torch.zeros(1, 3, 3, 4, 4)), (feat, torch.zeros(1, 2, 3, 4, 8)),
                              (feat[0], inp)):
        with pytest.raises(ValueError, match="expected"):
            dec(bad_feat, bad_inp, [0.5])
    for scale in ((1, 8), (8, 1), (0, 0)):
        with pytest.raises(ValueError, match="at least 2 x 2"):
            dec(feat, inp, [0.5], scale)
    with pytest.raises(ValueError, match="times"):
        dec(feat, inp, [])
    with pytest.raises(ValueError, match="scale"):
        dec(feat, inp, [0.5], (8, 8, 8))
    net = T.LunaTokis(1, 1)
    with pytest.raises(RuntimeError, match="CUDA"):
        net(torch.zeros(1, 2, 3, 8, 8), [0.5])
    for shape in ((1, 2, 3, 6, 8), (1, 2, 3, 8, 10), (1, 3, 3, 8, 8), (1, 2, 4, 8, 8), (2, 3, 8, 8)):
        with pytest.raises(ValueError):
            net(torch.zeros(*shape), [0.5])
    with pytest.raises(ValueError, match="at least 2 x 2"):
        net(torch.zeros(1, 2, 3, 8, 8), [0.5], (1, 4))
    with pytest.raises(ValueError):
        T.LunaTokis(mfma="bf16")
    # the reference's three forms of ``scale`` and its [B, 1] times
    assert T._hr_size(5, 7, None) == (20, 28) and T._hr_size(5, 7, (11, 13)) == (11, 13)
    assert T._hr_size(5, 7, [torch.tensor([11, 11]), torch.tensor([13, 13])]) == (11, 13)
    t = T._item_times(torch.tensor([[0.25], [0.75]]), 2, "cpu")
    assert t.tolist() == [0.25, 0.75] and T._item_times(0.5, 3, "cpu").tolist() == [0.5] * 3
    with pytest.raises(ValueError):
        T._item_times(torch.zeros(3, 1), 2, "cpu")


def test_times_loss_is_the_reference_sum(stif):
    T = stif.train
    outs = [torch.full((2, 3, 4, 4), 1.0), torch.full((2, 3, 4, 4), 3.0)]
    gt = torch.zeros(2, 2, 3, 4, 4)
    cb = T.CharbonnierLoss()
    assert float(T.TimesLoss(cb)(outs, gt)) == pytest.approx(float(cb(outs[0], gt[:, 0]) + cb(outs[1], gt[:, 1])))
