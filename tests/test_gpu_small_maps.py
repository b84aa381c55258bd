"""Every forward launch form at maps smaller than a tile, against the float64 oracle.

The 3x3 / 1x1 convolutions, the DCN core and the fused DCN_sep work on output tiles of 4 or 8 rows by 32 columns;
the model runs them down to 1 x 1 maps (a 4 x 4 frame's L3 level).  Here every pixel is a border pixel, most of the
halo lies outside the map, and the second tile row / column of 5 x 33 holds a single row / column.

Layout of every case: 3 items with different content, given as views with one item stride larger than the dense item
(gaps of GAP floats).  Every buffer starts as a fixed NaN bit pattern (SENT), so the gaps of the inputs are NaN --
anything read past an item and not masked turns the output non-finite -- and the gaps of the outputs must still hold
the pattern bit for bit after the launch, which catches a store past a tiny map into its neighbour; an output
element never written stays non-finite.  The inputs must come back unchanged bit for bit.

Bar: the kernel bar of tests/test_gpu_ops.py and tests/test_gpu_wino.py, max |gpu - ref| / max |ref| < 1e-5 for
both operand modes; weights rnd(scale=0.05) (0.04 for 128 input channels, 0.1 for the 1x1 cat convs, as there),
N(0, 1) activations.  Every case prints its error and each family its worst one when the module is done
(``pytest -s``)."""
import numpy as np
import pytest
import torch

from oracle import stif_oracle as O

pytestmark = pytest.mark.gpu

RTOL = 1e-5
N = 3                # items per launch
GAP = 96             # floats between the end of an item and the next item
SENT = 0x7FC5A5A5    # a quiet NaN with a payload no kernel produces

# output maps: 1 x 33, 5 x 1 and 5 x 33 put a one-column / one-row second tile after a full one (9 x 1 for 8-row tiles)
BASE = [(1, 1), (1, 2), (2, 1), (2, 2), (3, 3), (1, 33), (5, 1), (5, 33)]
BASE8 = BASE + [(9, 1)]
# outputs of the forms with an x2-upsampled second input (coarse maps 1x1, 1x2, 2x1, 1x17, 3x1, 3x17, and 2x2: the
# smallest with a quad of four interior pixels; 5x1 for 8-row tiles)
UP = [(2, 2), (2, 4), (4, 2), (2, 34), (6, 2), (6, 34), (4, 4)]
UP8 = UP + [(10, 2)]
# stride-2 inputs: every base-list output from an odd and an even input side, in both directions
S2_IN = sorted({(2 * h - a, 2 * w - b) for h, w in BASE for a in (0, 1) for b in (0, 1)})

hwid = lambda hw: f"{hw[0]}x{hw[1]}"
MODES = pytest.mark.parametrize("f16", [0, 1], ids=["f32", "f16x3"])

_WORST = {}          # family -> (worst error, case)
_REF = {}            # case key -> inputs and oracle outputs, computed once for every family / operand mode using them
_PACKED = {}         # (weights key, pack mode) -> PackedConv


def rnd(*shape, seed=0, scale=1.0):
    return (np.random.default_rng(seed).standard_normal(shape) * scale).astype(np.float32)


def relmax(a, b):
    return float(np.abs(np.asarray(a, np.float64) - b).max() / max(np.abs(b).max(), 1e-30))


class Items:
    """N NHWC items [h, w, c] as a view, item stride h w c + GAP, of a buffer that starts as SENT everywhere;
    ``nchw``: the content of the maps (None for an output)."""

    def __init__(self, h, w, c, nchw=None):
        self.dense = h * w * c
        stride = self.dense + GAP
        self.bits = torch.full((N, stride), SENT, dtype=torch.int32, device="cuda")
        self.t = torch.as_strided(self.bits.view(torch.float32), (N, h, w, c), (stride, w * c, c, 1))
        if nchw is not None:
            assert nchw.shape == (N, c, h, w)
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(np.asarray(nchw, np.float32).transpose(0, 2, 3, 1))))
        self.before = self.bits.clone()

    def gaps_intact(self):
        return bool((self.bits[:, self.dense:] == SENT).all())

    def unchanged(self):
        return torch.equal(self.bits, self.before)

    def nhwc(self):
        return self.t.cpu().numpy()

    def nchw(self):
        return self.nhwc().transpose(0, 3, 1, 2)


def verify(family, what, pairs, outs, ins, status=None):
    """pairs: (name, gpu array, oracle array) of every output map; outs / ins: the output / input Items."""
    worst = 0.0
    for name, got, ref in pairs:
        assert got.shape == ref.shape, (what, name, got.shape, ref.shape)
        assert np.isfinite(got).all(), (what, name, "non-finite or unwritten output elements", int((~np.isfinite(got)).sum()))
        e = relmax(got, ref)
        print(what, name, f"max |gpu - ref| / max |ref| = {e:.3e} (bar {RTOL:g})")
        worst = max(worst, e)
    if worst >= _WORST.get(family, (-1.0, ""))[0]:
        _WORST[family] = (worst, what)
    assert worst < RTOL, (what, worst)
    for i, o in enumerate(outs):
        assert o.gaps_intact(), (what, f"output {i}: a word between the items was overwritten")
    for i, t in enumerate(ins):
        assert t.unchanged(), (what, f"input {i} was written to")
    if status is not None:
        torch.cuda.synchronize()
        assert int(status.item()) == 0, (what, "f16x3 range status set")


@pytest.fixture(scope="module", autouse=True)
def report():
    """Each family's worst case when the module is done (shown with ``pytest -s``)."""
    yield
    print()
    for fam, (e, what) in sorted(_WORST.items()):
        print(f"small maps: {fam:<10} worst max |gpu - ref| / max |ref| = {e:.3e} at {what} (bar {RTOL:g})")


@pytest.fixture(scope="module")
def L(stif):
    return stif._lib


@pytest.fixture(scope="module")
def ops(stif):
    return stif.ops


def packed(ops, L, key, w, b, mode, want_f16):
    """ops.pack_conv once per (weights, mode); an f16x3 packing must not have fallen back to fp32."""
    k = (key, mode)
    if k not in _PACKED:
        _PACKED[k] = ops.pack_conv(w, b, mode)
    lay = _PACKED[k]
    assert bool(lay.mode & L.PACK_F16X3) == bool(want_f16), (key, "packing fell back to fp32")
    return lay


def status_word(f16):
    return torch.zeros(1, dtype=torch.int32, device="cuda") if f16 else None


# ---------------------------------------------------------------- 3x3 stride 1: Winograd and direct kernel
CONV_FORMS = ["none", "lrelu", "relu", "res", "res_inplace", "cat2g", "up2_s1", "up2_s2", "up2_s8", "offmask", "lstm"]
UP_FORMS = ("up2_s1", "up2_s2", "up2_s8")
_ACT = dict(none=lambda v: v, lrelu=O.lrelu, relu=O.relu)


def conv_weights(form):
    """(weights key, [(w, b) per group]) of a form -- the same for every size."""
    if form in ("none", "lrelu", "relu", "res", "res_inplace"):
        return "plain", [(rnd(64, 64, 3, 3, seed=2, scale=0.05), rnd(64, seed=3))]
    if form == "cat2g":
        return "cat2g", [(rnd(64, 128, 3, 3, seed=10 + g, scale=0.04), rnd(64, seed=12 + g)) for g in range(2)]
    if form in UP_FORMS:
        return "up2", [(rnd(64, 128, 3, 3, seed=23, scale=0.04), rnd(64, seed=24))]
    if form == "offmask":
        return "offmask", [(rnd(216, 64, 3, 3, seed=21, scale=0.05), rnd(216, seed=22))]
    assert form == "lstm"
    return "lstm", [(rnd(256, 128, 3, 3, seed=73, scale=0.04), rnd(256, seed=76))]


def conv_case(form, hw):
    """Inputs (NCHW, per group) and float64 oracle outputs of one 3x3 stride-1 form at output size hw."""
    key = ("conv", form, hw)
    if key in _REF:
        return _REF[key]
    H, W = hw
    s = 1000 * H + W
    _, wb = conv_weights(form)
    c = dict(form=form, hw=hw, in1_mode=0, in1_scale=1.0, cout=64)
    if form in ("none", "lrelu", "relu", "res", "res_inplace"):
        x, r = rnd(N, 64, H, W, seed=s + 1), rnd(N, 64, H, W, seed=s + 4)
        ref = O.conv2d(x, *wb[0])
        ref = ref + r if form.startswith("res") else _ACT[form](ref)
        c.update(epi="res" if form.startswith("res") else form, groups=[dict(in0=x, res=r if form.startswith("res") else None)],
                 refs=[[("out", ref)]])
    elif form == "cat2g":
        a, b = rnd(N, 64, H, W, seed=s + 5), rnd(N, 64, H, W, seed=s + 6)
        c.update(epi="lrelu", in1_mode=1, groups=[dict(in0=a, in1=b), dict(in0=b, in1=a)],
                 refs=[[("out", O.lrelu(O.conv2d(np.concatenate([a, b], 1), *wb[0])))],
                       [("out", O.lrelu(O.conv2d(np.concatenate([b, a], 1), *wb[1])))]])
    elif form in UP_FORMS:
        scale, epi = {"up2_s1": (1.0, "none"), "up2_s2": (2.0, "lrelu"), "up2_s8": (8.0, "lrelu")}[form]
        x0, co = rnd(N, 64, H, W, seed=s + 7), rnd(N, 64, H // 2, W // 2, seed=s + 8)
        up = O.upsample2x(co.astype(np.float64)) * scale
        c.update(epi=epi, in1_mode=2, in1_scale=scale, groups=[dict(in0=x0, in1=co)],
                 refs=[[("out", _ACT[epi](O.conv2d(np.concatenate([x0, up], 1), *wb[0])))]])
    elif form == "offmask":
        x = rnd(N, 64, H, W, seed=s + 9)
        ref = O.conv2d(x, *wb[0])
        off = ref[:, :144].reshape(N, 8, 9, 2, H, W).transpose(0, 4, 5, 1, 2, 3)      # [n, y, x, group, tap, (dy, dx)]
        msk = O.sigmoid(ref[:, 144:].reshape(N, 8, 9, H, W).transpose(0, 3, 4, 1, 2))
        c.update(epi="offmask", cout=216, groups=[dict(in0=x)], refs=[[("offsets", off), ("masks", msk)]])
    else:
        x, h, cc = (rnd(N, 64, H, W, seed=s + 10 + k) for k in range(3))
        hn, cn = O.conv_lstm_cell(x, h, cc, {"conv.weight": wb[0][0], "conv.bias": wb[0][1]}, "", np.float64)
        c.update(epi="lstm", in1_mode=1, groups=[dict(in0=x, in1=h, res=cc)], refs=[[("h_next", hn), ("c_next", cn)]])
    _REF[key] = c
    return c


def run_conv3x3(ops, L, family, form, hw, wino, f16):
    c = conv_case(form, hw)
    H, W = hw
    wkey, wb = conv_weights(form)
    kinds = dict(offmask=(L.PACK_WINO_OFFMASK, L.PACK_OFFMASK), lstm=(L.PACK_WINO_LSTM, L.PACK_LSTM))
    mode = kinds.get(form, (L.PACK_WINO, L.PACK_PLAIN))[0 if wino else 1] | (L.PACK_F16X3 if f16 else 0)
    epi = dict(none=L.EPI_NONE, lrelu=L.EPI_LRELU, relu=L.EPI_RELU, res=L.EPI_RES, offmask=L.EPI_OFFMASK,
               lstm=L.EPI_LSTM)[c["epi"]]
    groups, outs, ins, pairs = [], [], [], []
    for g, (grp, refs) in enumerate(zip(c["groups"], c["refs"])):
        d = dict(layer=packed(ops, L, (wkey, g), *wb[g], mode, f16))
        in0 = Items(H, W, 64, grp["in0"])
        ins.append(in0)
        d["in0"] = in0.t
        if grp.get("in1") is not None:
            h1, w1 = grp["in1"].shape[2:]
            in1 = Items(h1, w1, 64, grp["in1"])
            ins.append(in1)
            d["in1"] = in1.t
        if form == "res_inplace":                       # out is res: the ResidualBlock_noBN update of the model
            out = Items(H, W, 64, grp["res"])
            d["res"] = out.t
        else:
            out = Items(H, W, c["cout"])
            if grp.get("res") is not None:
                res = Items(H, W, 64, grp["res"])
                ins.append(res)
                d["res"] = res.t
        d["out"] = out.t
        outs.append(out)
        if form == "lstm":
            out2 = Items(H, W, 64)
            d["out2"] = out2.t
            outs.append(out2)
        groups.append(d)
        if form == "offmask":                           # the readers run after the launch
            pairs.append((refs, lambda o=out: [o.nhwc().reshape(N, H, W, 8, 9, 3)[..., :2],
                                               o.nhwc().reshape(N, H, W, 8, 9, 3)[..., 2]]))
        elif form == "lstm":
            pairs.append((refs, lambda o=out, o2=out2: [o.nchw(), o2.nchw()]))
        else:
            pairs.append((refs, lambda o=out: [o.nchw()]))
    st = status_word(f16)
    ops.conv2d(groups, epi=epi, in1_mode=c["in1_mode"], in1_scale=c["in1_scale"], status=st)
    what = f"{family} {form} {hwid(hw)} {'f16x3' if f16 else 'f32'}"
    flat = [(f"group {g} {name}", got, ref) for g, (refs, read) in enumerate(pairs)
            for (name, ref), got in zip(refs, read())]
    verify(family, what, flat, outs, ins, st)


def conv_sizes(form, tile8):
    if form in UP_FORMS:
        return UP8 if tile8 else UP
    return BASE8 if tile8 else BASE


WINO_CASES = [(f, hw) for f in CONV_FORMS for hw in conv_sizes(f, False)]
DIRECT_CASES = [(f, hw) for f in CONV_FORMS for hw in conv_sizes(f, True)]
case_id = lambda c: f"{c[0]}-{hwid(c[1])}"


@MODES
@pytest.mark.parametrize("case", WINO_CASES, ids=case_id)
def test_wino(ops, L, case, f16):
    """stif_conv3x3_wino (k_wino, and k_wino_om for the f16x3 offset/mask conv; 4-row tiles): plain epilogues, the
    residual epilogue out of place and in place, cat(in0, in1) in two weight groups, the fused x2 upsample of in1 at
    scale 1 (EPI_NONE), 2 and 8 (EPI_LRELU) -- coarse maps of one row / column, where no quad of the expansion is
    interior and the 2x2-quad form must not be taken (it once was at scale 8, for column 0 of a coarse 2 x 1 and 3 x 1
    map: the test read a scaled row weight for the width), and 3 x 17, where both forms meet in one tile --, the
    offset/mask conv and the ConvLSTM cell conv with out2."""
    run_conv3x3(ops, L, "wino", *case, True, f16)


@pytest.mark.parametrize("case", DIRECT_CASES, ids=case_id)
def test_direct3x3(ops, L, case):
    """stif_conv2d_nhwc, 3x3 stride 1 (k_conv; 8-row tiles, so 9 x 1 and 10 x 2 are added): the same forms on the
    direct implicit-GEMM kernel (fp32 only: the stride-1 direct conv has no f16x3 form)."""
    run_conv3x3(ops, L, "direct3x3", *case, False, 0)


# ---------------------------------------------------------------- 3x3 stride 2
def s2_case(hw):
    key = ("s2", hw)
    if key not in _REF:
        H, W = hw
        x = rnd(N, 64, H, W, seed=2000 * H + W)
        w, b = rnd(64, 64, 3, 3, seed=15, scale=0.05), rnd(64, seed=16)
        _REF[key] = (x, w, b, O.conv2d(x, w, b, stride=2))
    return _REF[key]


@MODES
@pytest.mark.parametrize("epi", ["none", "lrelu"])
@pytest.mark.parametrize("hw", S2_IN, ids=hwid)
def test_stride2(ops, L, hw, epi, f16):
    """stif_conv2d_nhwc, 3x3 stride 2 (the pyramid convs; 4-row tiles), f32 and f16x3: input sizes giving every
    base-list output from odd and even input sides (an even side reads one more input row / column)."""
    H, W = hw
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    assert (Ho, Wo) in BASE
    x, w, b, ref = s2_case(hw)
    lay = packed(ops, L, "s2", w, b, L.PACK_PLAIN | (L.PACK_F16X3 if f16 else 0), f16)
    xin, out = Items(H, W, 64, x), Items(Ho, Wo, 64)
    st = status_word(f16)
    ops.conv2d([dict(layer=lay, in0=xin.t, out=out.t)], epi=L.EPI_LRELU if epi == "lrelu" else L.EPI_NONE, stride=2,
               status=st)
    what = f"stride2 {epi} in {hwid(hw)} out {Ho}x{Wo} {'f16x3' if f16 else 'f32'}"
    verify("stride2", what, [("out", out.nchw(), _ACT[epi](ref))], [out], [xin], st)


# ---------------------------------------------------------------- 1x1
def c1_weights(form):
    if form == "proj":
        return [(rnd(256, 200, 1, 1, seed=18, scale=0.05), rnd(256, seed=19))]
    return [(rnd(64, 128, 1, 1, seed=41 + g, scale=0.1), rnd(64, seed=43 + g)) for g in range(2)]


def c1_case(form, hw):
    key = ("c1", form, hw)
    if key not in _REF:
        H, W = hw
        s = 3000 * H + W
        wb = c1_weights(form)
        if form == "proj":
            x = rnd(N, 200, H, W, seed=s)
            _REF[key] = ([dict(in0=x)], [O.conv2d(x, *wb[0])])
        else:
            a, b = rnd(N, 64, H, W, seed=s + 1), rnd(N, 64, H, W, seed=s + 2)
            _REF[key] = ([dict(in0=a, in1=b), dict(in0=b, in1=a)],
                         [O.conv2d(np.concatenate([a, b], 1), *wb[0]), O.conv2d(np.concatenate([b, a], 1), *wb[1])])
    return _REF[key]


@MODES
@pytest.mark.parametrize("form", ["proj", "cat2g"])
@pytest.mark.parametrize("hw", BASE8, ids=hwid)
def test_conv1x1(ops, L, hw, form, f16):
    """stif_conv2d_nhwc, 1x1: the decoder's LR projection 200 -> 256 (fp32 k_conv with 8-row tiles, or k_conv1x1<13>)
    and the fusion convs on cat(64, 64) in two weight groups (fp32 k_conv, or k_conv1x1<8>); the f16x3 kernels walk
    32-pixel M-tiles over the items, so an item of 1..9 pixels is a fraction of one and 33 pixels one and a bit."""
    H, W = hw
    grps, refs = c1_case(form, hw)
    wb = c1_weights(form)
    cin0, cout = (200, 256) if form == "proj" else (64, 64)
    groups, outs, ins, pairs = [], [], [], []
    for g, grp in enumerate(grps):
        d = dict(layer=packed(ops, L, ("c1", form, g), *wb[g], L.PACK_PLAIN | (L.PACK_F16X3 if f16 else 0), f16))
        for k in ("in0", "in1"):
            if k in grp:
                it = Items(H, W, cin0, grp[k])
                ins.append(it)
                d[k] = it.t
        out = Items(H, W, cout)
        d["out"] = out.t
        outs.append(out)
        groups.append(d)
    st = status_word(f16)
    ops.conv2d(groups, in1_mode=0 if form == "proj" else 1, status=st)
    what = f"conv1x1 {form} {hwid(hw)} {'f16x3' if f16 else 'f32'}"
    verify("conv1x1", what, [(f"group {g} out", o.nchw(), r) for g, (o, r) in enumerate(zip(outs, refs))], outs, ins, st)


# ---------------------------------------------------------------- conv_first
@pytest.mark.parametrize("hw", BASE8, ids=hwid)
def test_conv_first(ops, hw):
    """stif_conv_first (3 -> 64 on the NCHW frames, LeakyReLU): its ABI takes dense buffers, so the three frames and
    their outputs lie back to back, each buffer between GAP-float guards that start as SENT."""
    H, W = hw
    x = np.random.default_rng(4000 * H + W).random((N, 3, H, W)).astype(np.float32)
    w, b = rnd(64, 3, 3, 3, seed=27, scale=0.2), rnd(64, seed=28)

    def guarded(numel):
        bits = torch.full((numel + 2 * GAP,), SENT, dtype=torch.int32, device="cuda")
        return bits, bits.view(torch.float32)[GAP:GAP + numel]
    xb, xt = guarded(x.size)
    ob, ot = guarded(N * H * W * 64)
    xt.copy_(torch.from_numpy(x).reshape(-1))
    x_before = xb.clone()
    out = ot.view(N, H, W, 64)
    ops.conv_first(xt.view(N, 3, H, W), torch.from_numpy(w).cuda(), torch.from_numpy(b).cuda(), out)
    what = f"conv_first {hwid(hw)}"
    verify("conv_first", what, [("out", out.cpu().numpy().transpose(0, 3, 1, 2), O.lrelu(O.conv2d(x, w, b)))], [], [])
    assert bool((ob[:GAP] == SENT).all()) and bool((ob[-GAP:] == SENT).all()), (what, "a guard word was overwritten")
    assert torch.equal(xb, x_before), (what, "the input was written to")


# ---------------------------------------------------------------- DCN core and fused DCN_sep
# offsets of ~0.3 px keep the samples near the 3x3 footprint; at 3 px most samples leave a 1- or 2-pixel map
OSCALES = [0.3, 3.0]


def assert_not_bias_only(ref, bias, what):
    """The oracle output (before the activation) differs from the bias at every pixel: a case that samples nothing
    -- every sample outside the map, or masked -- would pass any kernel that writes the bias."""
    d = np.abs(ref - np.asarray(bias, np.float64)[None, :, None, None]).max(axis=1)     # [n, H, W]: max over channels
    assert (d > 1e-2).all(), (what, "a pixel of the reference holds the bias only", float(d.min()))


def dcn_case(hw, oscale):
    """x, weights, offsets / masks (reference channel order) with four samples exactly on the sampling gates, the
    packed [n, H, W, 216] offmask map and the oracle output before the activation."""
    key = ("dcn", hw, oscale)
    if key in _REF:
        return _REF[key]
    H, W = hw
    s = 5000 * H + W
    x = rnd(N, 64, H, W, seed=s)
    w, b = rnd(64, 64, 3, 3, seed=31, scale=0.05), rnd(64, seed=32)
    rng = np.random.default_rng(s + 1)
    off = (rng.standard_normal((N, 144, H, W)) * oscale).astype(np.float32)
    mask = rng.random((N, 72, H, W)).astype(np.float32)
    # the centre tap (4) of pixel (0, 0) samples (dy, dx): exactly on the `> -1` gates (groups 0, 2: not sampled) and
    # exactly on the `< H`, `< W` gates (groups 1, 3: not sampled) -- these fit a 1 x 1 map
    off[:, 0 * 18 + 2 * 4, 0, 0] = -1.0
    off[:, 1 * 18 + 2 * 4, 0, 0] = float(H)
    off[:, 2 * 18 + 2 * 4 + 1, 0, 0] = -1.0
    off[:, 3 * 18 + 2 * 4 + 1, 0, 0] = float(W)
    ref = O.dcn_v2_forward(x, w, b, off, mask, 3, 3, 1, 1, 1, 1, 1, 1, 8)
    o = off.reshape(N, 8, 9, 2, H, W).transpose(0, 4, 5, 1, 2, 3)
    m = mask.reshape(N, 8, 9, H, W).transpose(0, 3, 4, 1, 2)
    om = np.ascontiguousarray(np.concatenate([o, m[..., None]], -1).reshape(N, H, W, 216).transpose(0, 3, 1, 2))
    _REF[key] = (x, w, b, om, ref)
    return _REF[key]


@MODES
@pytest.mark.parametrize("epi", ["none", "lrelu"])
@pytest.mark.parametrize("oscale", OSCALES)
@pytest.mark.parametrize("hw", BASE, ids=hwid)
def test_dcn(ops, L, hw, oscale, epi, f16):
    """stif_dcn_nhwc (k_dcn; 4-row tiles at these grid sizes) through ops.dcn, f32 and f16x3."""
    H, W = hw
    x, w, b, om, ref = dcn_case(hw, oscale)
    what = f"dcn {epi} {hwid(hw)} offsets {oscale} px {'f16x3' if f16 else 'f32'}"
    if oscale < 1:
        assert_not_bias_only(ref, b, what)
    lay = packed(ops, L, "dcn", w, b, L.PACK_PLAIN | (L.PACK_F16X3 if f16 else 0), f16)
    xin, omin, out = Items(H, W, 64, x), Items(H, W, 216, om), Items(H, W, 64)
    st = status_word(f16)
    ops.dcn([dict(layer=lay, inp=xin.t, offmask=omin.t, out=out.t)], epi=L.EPI_LRELU if epi == "lrelu" else L.EPI_NONE,
            status=st)
    verify("dcn", what, [("out", out.nchw(), _ACT[epi](ref))], [out], [xin, omin], st)


def dcnsep_weights(oscale):
    """conv_offset_mask / DCN weights in the style of tests/test_gpu_ops.py::_dcnsep_weights: offsets with a std of
    about ``oscale`` px on N(0, 1) features (less where most of the 3x3 footprint of the offset conv is padding).  Four
    offset channels have zero weights and a bias, so the centre tap of groups 0..3 samples at exactly (oy - 1, ox),
    (oy + 1, ox), (oy, ox - 1) and (oy, ox + 1): on the `> -1` gate in row / column 0 and on the `< H` / `< W` gate in
    the last row / column -- whatever the size of the map."""
    if ("dcnsep_w", oscale) not in _REF:
        w_om = rnd(216, 64, 3, 3, seed=40, scale=oscale / 24.0)
        b_om = rnd(216, seed=41, scale=0.5)
        b_om[:144] *= oscale
        for ch, v in ((0 * 18 + 2 * 4, -1.0), (1 * 18 + 2 * 4, 1.0), (2 * 18 + 2 * 4 + 1, -1.0), (3 * 18 + 2 * 4 + 1, 1.0)):
            w_om[ch] = 0.0
            b_om[ch] = v
        _REF["dcnsep_w", oscale] = {"x.conv_offset_mask.weight": w_om, "x.conv_offset_mask.bias": b_om,
                                     "x.weight": rnd(64, 64, 3, 3, seed=42, scale=0.05), "x.bias": rnd(64, seed=43)}
    return _REF["dcnsep_w", oscale]


def dcnsep_case(hw, oscale):
    key = ("dcnsep", hw, oscale)
    if key not in _REF:
        H, W = hw
        s = 6000 * H + W
        x, fea = rnd(N, 64, H, W, seed=s), rnd(N, 64, H, W, seed=s + 1)
        _REF[key] = (x, fea, O.dcn_sep(x, fea, dcnsep_weights(oscale), "x"))
    return _REF[key]


@pytest.mark.parametrize("epi", ["none", "lrelu"])
@pytest.mark.parametrize("oscale", OSCALES)
@pytest.mark.parametrize("hw", BASE, ids=hwid)
def test_dcn_sep(ops, L, hw, oscale, epi):
    """stif_dcn_sep_nhwc (k_dcn_sep: offset/mask conv + sigmoid + deformable conv in one launch; 4-row tiles,
    PACK_DCNSEP / PACK_DCNPAIR packings, f16x3 only)."""
    H, W = hw
    sdx = dcnsep_weights(oscale)
    x, fea, ref = dcnsep_case(hw, oscale)
    what = f"dcn_sep {epi} {hwid(hw)} offsets {oscale} px"
    if oscale < 1:
        assert_not_bias_only(ref, sdx["x.bias"], what)
    k = ("dcnsep", oscale)
    if k not in _PACKED:
        _PACKED[k] = (ops.pack_conv(sdx["x.conv_offset_mask.weight"], sdx["x.conv_offset_mask.bias"],
                                    L.PACK_DCNSEP | L.PACK_F16X3, range_fallback=False),
                      ops.pack_conv(sdx["x.weight"], sdx["x.bias"], L.PACK_DCNPAIR | L.PACK_F16X3, range_fallback=False))
    om, core = _PACKED[k]
    xin, fin, out = Items(H, W, 64, x), Items(H, W, 64, fea), Items(H, W, 64)
    st = status_word(1)
    ops.dcn_sep([dict(om_layer=om, layer=core, fea=fin.t, inp=xin.t, out=out.t)],
                epi=L.EPI_LRELU if epi == "lrelu" else L.EPI_NONE, status=st)
    verify("dcn_sep", what, [("out", out.nchw(), _ACT[epi](ref))], [out], [xin, fin], st)
