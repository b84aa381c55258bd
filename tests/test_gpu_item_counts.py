"""Launches whose weight sets carry their own item counts (stif.h item_base), against the uniform form, bit for bit.

Every kernel computes an item from that item's maps and its set's weights alone, so one launch over sets of
(1, 3, 2) items must write exactly what three uniform launches -- one per set -- write: torch.equal on every output,
for both operand modes.  The map is 12 x 36: three row tiles of 4 (two of 8 for the 8-row kernels, the second
partial) and two column tiles, the second 4 columns wide; sets get different weights and items different content, so
an item decoded into the wrong set or the wrong slot cannot match.  Outputs start as NaN, so an item never written
cannot match either.  Ten sets of one item on a 4 x 4 map go past the former limit of 8 sets below the tile size.
A table that does not increase, has an empty set, names more than 16 sets or holds more items than the launch grid
is refused with STIF_E_INVALID before anything is launched: the outputs keep their bits."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

H, W = 12, 36
COUNTS = (1, 3, 2)
MODES = pytest.mark.parametrize("f16", [0, 1], ids=["f32", "f16x3"])
_PACKED = {}


def rnd(*shape, seed=0, scale=1.0):
    return (np.random.default_rng(seed).standard_normal(shape) * scale).astype(np.float32)


def dev(*shape, seed):
    return torch.from_numpy(rnd(*shape, seed=seed)).cuda()


def nan(*shape):
    return torch.full(shape, float("nan"), device="cuda")


@pytest.fixture(scope="module")
def L(stif):
    return stif._lib


@pytest.fixture(scope="module")
def ops(stif):
    return stif.ops


def packed(ops, L, key, shape, mode, f16, scale=0.05, **kw):
    """One layer per (key, mode): weights N(0, scale), bias N(0, 1); an f16x3 packing must not fall back."""
    k = (key, shape, mode)
    if k not in _PACKED:
        seed = 1000 + len(_PACKED)
        _PACKED[k] = ops.pack_conv(rnd(*shape, seed=seed, scale=scale), rnd(shape[0], seed=seed + 500), mode, **kw)
    assert bool(_PACKED[k].mode & L.PACK_F16X3) == bool(f16), (key, "packing fell back to fp32")
    return _PACKED[k]


def sets_of(counts, *shape, seed):
    """One input per set: slices of one buffer, so every set has the same item stride."""
    flat = dev(sum(counts), *shape, seed=seed)
    b = np.concatenate([[0], np.cumsum(counts)])
    return [flat[b[i]:b[i + 1]] for i in range(len(counts))]


def outs_of(counts, *shape):
    flat = nan(sum(counts), *shape)
    b = np.concatenate([[0], np.cumsum(counts)])
    return [flat[b[i]:b[i + 1]] for i in range(len(counts))]


def both_ways(launch, groups, out_keys, status):
    """``launch(groups)`` once over all sets (their own counts) and once per set (uniform); every output equal."""
    merged = [dict(g, **{k: torch.full_like(g[k], float("nan")) for k in out_keys}) for g in groups]
    launch(merged)
    for i, g in enumerate(groups):
        launch([g])
        for k in out_keys:
            assert bool(torch.isfinite(g[k]).all()), (i, k, "uniform launch left elements unwritten")
            assert torch.equal(merged[i][k], g[k]), (i, k, "per-set counts differ from the uniform launch")
    if status is not None:
        assert int(status.item()) == 0, "f16x3 range status set"


def status_word(f16):
    return torch.zeros(1, dtype=torch.int32, device="cuda") if f16 else None


WINO_FORMS = ["lrelu", "none", "res", "cat_lrelu", "up2_s1_none", "up2_s2_lrelu"]


@MODES
@pytest.mark.parametrize("form", WINO_FORMS)
def test_wino(ops, L, form, f16):
    """stif_conv3x3_wino: epilogues LRELU / NONE / RES on one input, cat(in0, in1) (in1_mode 1) and cat(in0, s * up2(in1))
    from a 6 x 18 coarse map (in1_mode 2) at scales 1 and 2."""
    in1_mode = 1 if form.startswith("cat") else 2 if form.startswith("up2") else 0
    scale = 2.0 if "s2" in form else 1.0
    epi = L.EPI_RES if form == "res" else L.EPI_LRELU if form.endswith("lrelu") else L.EPI_NONE
    cin = 128 if in1_mode else 64
    mode = L.PACK_WINO | (L.PACK_F16X3 if f16 else 0)
    x = sets_of(COUNTS, H, W, 64, seed=1)
    x1 = sets_of(COUNTS, *((H // 2, W // 2) if in1_mode == 2 else (H, W)), 64, seed=2)
    r = sets_of(COUNTS, H, W, 64, seed=3)
    o = outs_of(COUNTS, H, W, 64)
    groups = []
    for g in range(len(COUNTS)):
        d = dict(layer=packed(ops, L, ("wino", g), (64, cin, 3, 3), mode, f16, scale=0.04 if in1_mode else 0.05),
                 in0=x[g], out=o[g])
        if in1_mode:
            d["in1"] = x1[g]
        if form == "res":
            d["res"] = r[g]
        groups.append(d)
    st = status_word(f16)
    both_ways(lambda gs: ops.conv2d(gs, epi=epi, in1_mode=in1_mode, in1_scale=scale, status=st), groups, ["out"], st)


@MODES
def test_wino_lstm_cell(ops, L, f16):
    """The ConvLSTM cell (128 -> 256, out = h_next, out2 = c_next, res = c_cur), sets of (2, 1) items."""
    counts = (2, 1)
    mode = L.PACK_WINO_LSTM | (L.PACK_F16X3 if f16 else 0)
    x, h, c = (sets_of(counts, H, W, 64, seed=10 + k) for k in range(3))
    o, o2 = outs_of(counts, H, W, 64), outs_of(counts, H, W, 64)
    groups = [dict(layer=packed(ops, L, ("lstm", g), (256, 128, 3, 3), mode, f16, scale=0.04), in0=x[g], in1=h[g],
                   res=c[g], out=o[g], out2=o2[g]) for g in range(2)]
    st = status_word(f16)
    both_ways(lambda gs: ops.conv2d(gs, epi=L.EPI_LSTM, in1_mode=1, status=st), groups, ["out", "out2"], st)


@MODES
def test_conv_stride2(ops, L, f16):
    """stif_conv2d_nhwc, 3x3 stride 2 (12 x 36 -> 6 x 18), LeakyReLU: the pyramid convs."""
    mode = L.PACK_PLAIN | (L.PACK_F16X3 if f16 else 0)
    x = sets_of(COUNTS, H, W, 64, seed=20)
    o = outs_of(COUNTS, H // 2, W // 2, 64)
    groups = [dict(layer=packed(ops, L, ("s2", g), (64, 64, 3, 3), mode, f16), in0=x[g], out=o[g]) for g in range(3)]
    st = status_word(f16)
    both_ways(lambda gs: ops.conv2d(gs, epi=L.EPI_LRELU, stride=2, status=st), groups, ["out"], st)


@MODES
def test_conv1x1_cat(ops, L, f16):
    """stif_conv2d_nhwc, 1x1 on cat(64, 64): the fusion convs (k_conv1x1 walks each set's own items)."""
    mode = L.PACK_PLAIN | (L.PACK_F16X3 if f16 else 0)
    a, b = sets_of(COUNTS, H, W, 64, seed=30), sets_of(COUNTS, H, W, 64, seed=31)
    o = outs_of(COUNTS, H, W, 64)
    groups = [dict(layer=packed(ops, L, ("c1", g), (64, 128, 1, 1), mode, f16, scale=0.1), in0=a[g], in1=b[g], out=o[g])
              for g in range(3)]
    st = status_word(f16)
    both_ways(lambda gs: ops.conv2d(gs, in1_mode=1, status=st), groups, ["out"], st)


def offmask_sets(counts, seed):
    """Packed offset / mask maps [n, H, W, 216] = [group][tap][dy, dx, mask]: offsets N(0, 1.5 px), masks U(0, 1)."""
    rng = np.random.default_rng(seed)
    om = rng.standard_normal((sum(counts), H, W, 72, 3)).astype(np.float32) * 1.5
    om[..., 2] = rng.random((sum(counts), H, W, 72)).astype(np.float32)
    flat = torch.from_numpy(om.reshape(sum(counts), H, W, 216)).cuda()
    b = np.concatenate([[0], np.cumsum(counts)])
    return [flat[b[i]:b[i + 1]] for i in range(len(counts))]


@MODES
@pytest.mark.parametrize("epi", ["none", "lrelu"])
def test_dcn(ops, L, epi, f16):
    """stif_dcn_nhwc (the deformable conv of the fp32 re-run path, and its f16x3 form)."""
    mode = L.PACK_PLAIN | (L.PACK_F16X3 if f16 else 0)
    x, om = sets_of(COUNTS, H, W, 64, seed=40), offmask_sets(COUNTS, 41)
    o = outs_of(COUNTS, H, W, 64)
    groups = [dict(layer=packed(ops, L, ("dcn", g), (64, 64, 3, 3), mode, f16), inp=x[g], offmask=om[g], out=o[g])
              for g in range(3)]
    st = status_word(f16)
    both_ways(lambda gs: ops.dcn(gs, epi=L.EPI_LRELU if epi == "lrelu" else L.EPI_NONE, status=st), groups, ["out"], st)


@pytest.mark.parametrize("epi", ["none", "lrelu"])
def test_dcn_sep(ops, L, epi):
    """stif_dcn_sep_nhwc (f16x3 only): offsets of about 1 px from N(0, 1) features."""
    x, fea = sets_of(COUNTS, H, W, 64, seed=50), sets_of(COUNTS, H, W, 64, seed=51)
    o = outs_of(COUNTS, H, W, 64)
    groups = [dict(om_layer=packed(ops, L, ("sep_om", g), (216, 64, 3, 3), L.PACK_DCNSEP | L.PACK_F16X3, 1, scale=1 / 24.0,
                                   range_fallback=False),
                   layer=packed(ops, L, ("sep", g), (64, 64, 3, 3), L.PACK_DCNPAIR | L.PACK_F16X3, 1, range_fallback=False),
                   fea=fea[g], inp=x[g], out=o[g]) for g in range(3)]
    st = status_word(1)
    both_ways(lambda gs: ops.dcn_sep(gs, epi=L.EPI_LRELU if epi == "lrelu" else L.EPI_NONE, status=st), groups, ["out"], st)


@MODES
def test_ten_sets_of_one_item_below_the_tile(ops, L, f16):
    """Ten weight sets (more than the former 8) of one item each on a 4 x 4 map, in one launch: the Winograd conv,
    the stride-2 conv and the 1x1 cat conv; every set equals its own uniform launch."""
    n, hw = 10, (4, 4)
    f = L.PACK_F16X3 if f16 else 0
    x, y = sets_of([1] * n, *hw, 64, seed=60), sets_of([1] * n, *hw, 64, seed=61)
    st = status_word(f16)
    g3 = [dict(layer=packed(ops, L, ("ten", g), (64, 64, 3, 3), L.PACK_WINO | f, f16), in0=x[g], out=o)
          for g, o in enumerate(outs_of([1] * n, *hw, 64))]
    both_ways(lambda gs: ops.conv2d(gs, epi=L.EPI_LRELU, status=st), g3, ["out"], st)
    g2 = [dict(layer=packed(ops, L, ("ten_s2", g), (64, 64, 3, 3), L.PACK_PLAIN | f, f16), in0=x[g], out=o)
          for g, o in enumerate(outs_of([1] * n, 2, 2, 64))]
    both_ways(lambda gs: ops.conv2d(gs, epi=L.EPI_LRELU, stride=2, status=st), g2, ["out"], st)
    g1 = [dict(layer=packed(ops, L, ("ten_c1", g), (64, 128, 1, 1), L.PACK_PLAIN | f, f16, scale=0.1), in0=x[g], in1=y[g],
               out=o) for g, o in enumerate(outs_of([1] * n, *hw, 64))]
    both_ways(lambda gs: ops.conv2d(gs, in1_mode=1, status=st), g1, ["out"], st)
    if f16:
        gd = [dict(om_layer=packed(ops, L, ("ten_om", g), (216, 64, 3, 3), L.PACK_DCNSEP | f, 1, scale=1 / 24.0,
                                   range_fallback=False),
                   layer=packed(ops, L, ("ten_sep", g), (64, 64, 3, 3), L.PACK_DCNPAIR | f, 1, range_fallback=False),
                   fea=y[g], inp=x[g], out=o) for g, o in enumerate(outs_of([1] * n, *hw, 64))]
        both_ways(lambda gs: ops.dcn_sep(gs, status=st), gd, ["out"], st)


# ---------------------------------------------------------------- tables the launchers refuse
BAD_TABLES = {
    "not_monotonic": (3, [0, 3, 2, 6]),
    "empty_set": (3, [0, 2, 2, 6]),
    "seventeen_sets": (17, [0] + list(range(1, 17))),
    "grid_overflow": (1, [0, 2 ** 31 - 1]),
}
SENT = 0x7FC5A5A5


def _fill(a, ngroups, table, ptr_fields, ptrs):
    a.ngroups, a.nitems = ngroups, 0
    for i, v in enumerate(table):
        a.item_base[i] = v
    for name, p in zip(ptr_fields, ptrs):
        for g in range(min(ngroups, 16)):
            getattr(a, name)[g] = p


@pytest.mark.parametrize("entry", ["wino", "conv_s2", "conv1x1", "dcn", "dcn_sep"])
@pytest.mark.parametrize("bad", sorted(BAD_TABLES))
def test_bad_tables_are_refused_before_any_launch(stif, ops, L, entry, bad):
    ngroups, table = BAD_TABLES[bad]
    lib = L.lib()
    f = L.PACK_F16X3
    x = dev(6, H, W, 64, seed=70)
    om = offmask_sets((6,), 71)[0]
    Ho, Wo = (H // 2, W // 2) if entry == "conv_s2" else (H, W)
    bits = torch.full((6, Ho, Wo, 64), SENT, dtype=torch.int32, device="cuda")
    out = bits.view(torch.float32)
    item = H * W * 64
    if entry in ("wino", "conv_s2", "conv1x1"):
        shape, mode = {"wino": ((64, 64, 3, 3), L.PACK_WINO | f), "conv_s2": ((64, 64, 3, 3), L.PACK_PLAIN | f),
                       "conv1x1": ((64, 128, 1, 1), L.PACK_PLAIN | f)}[entry]
        lay = packed(ops, L, ("bad", entry), shape, mode, 1)
        a = L.ConvArgs()
        _fill(a, ngroups, table, ["in0", "in1", "w", "bias", "out"],
              [x.data_ptr(), x.data_ptr(), lay.w.data_ptr(), lay.b.data_ptr(), out.data_ptr()])
        a.in0_item = a.in1_item = item
        a.out_item = Ho * Wo * 64
        a.H, a.W, a.C0, a.Ho, a.Wo, a.cout, a.flags = H, W, 64, Ho, Wo, 64, L.CONV_F16X3
        a.ks, a.stride, a.epi = (1 if entry == "conv1x1" else 3), (2 if entry == "conv_s2" else 1), L.EPI_NONE
        if entry == "conv1x1":
            a.C1, a.in1_mode = 64, 1
        fn = lib.stif_conv3x3_wino if entry == "wino" else lib.stif_conv2d_nhwc
    elif entry == "dcn":
        lay = packed(ops, L, ("bad", entry), (64, 64, 3, 3), L.PACK_PLAIN | f, 1)
        a = L.DcnArgs()
        _fill(a, ngroups, table, ["inp", "offmask", "w", "bias", "out"],
              [x.data_ptr(), om.data_ptr(), lay.w.data_ptr(), lay.b.data_ptr(), out.data_ptr()])
        a.in_item = a.out_item = item
        a.om_item = H * W * 216
        a.H, a.W, a.flags = H, W, L.CONV_F16X3
        fn = lib.stif_dcn_nhwc
    else:
        lo = packed(ops, L, ("bad", "om"), (216, 64, 3, 3), L.PACK_DCNSEP | f, 1, scale=1 / 24.0, range_fallback=False)
        lw = packed(ops, L, ("bad", "sep"), (64, 64, 3, 3), L.PACK_DCNPAIR | f, 1, range_fallback=False)
        a = L.DcnSepArgs()
        _fill(a, ngroups, table, ["fea", "inp", "w_om", "b_om", "w", "bias", "out"],
              [x.data_ptr(), x.data_ptr(), lo.w.data_ptr(), lo.b.data_ptr(), lw.w.data_ptr(), lw.b.data_ptr(),
               out.data_ptr()])
        a.fea_item = a.in_item = a.out_item = item
        a.H, a.W, a.flags = H, W, L.CONV_F16X3
        fn = lib.stif_dcn_sep_nhwc
    rc = fn(C.byref(a), torch.cuda.current_stream().cuda_stream)
    assert rc == L.E_INVALID, (entry, bad, rc, lib.stif_last_error())
    torch.cuda.synchronize()
    assert bool((bits == SENT).all()), (entry, bad, "a refused launch wrote to its output")


def test_valid_table_through_the_struct_runs(stif, ops, L):
    """The struct filled by hand (the ABI a C caller sees): sets of (2, 4) items of one buffer equal one uniform
    launch of 6 items with the same weights."""
    lib = L.lib()
    lay = packed(ops, L, ("bad", "wino"), (64, 64, 3, 3), L.PACK_WINO | L.PACK_F16X3, 1)
    x = dev(6, H, W, 64, seed=70)
    ref, out = nan(6, H, W, 64), nan(6, H, W, 64)
    ops.conv2d([dict(layer=lay, in0=x, out=ref)], epi=L.EPI_NONE)
    a = L.ConvArgs()
    item = H * W * 64
    _fill(a, 2, [0, 2, 6], ["w", "bias"], [lay.w.data_ptr(), lay.b.data_ptr()])
    a.in0[0], a.in0[1] = x.data_ptr(), x[2:].data_ptr()
    a.out[0], a.out[1] = out.data_ptr(), out[2:].data_ptr()
    a.in0_item = a.out_item = item
    a.H, a.W, a.C0, a.Ho, a.Wo, a.cout, a.flags = H, W, 64, H, W, 64, L.CONV_F16X3
    a.ks, a.stride, a.epi = 3, 1, L.EPI_NONE
    assert lib.stif_conv3x3_wino(C.byref(a), torch.cuda.current_stream().cuda_stream) == 0, lib.stif_last_error()
    assert torch.equal(out, ref)
