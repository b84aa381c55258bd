"""Deterministic training on the GPU: stif_segsum, stif_dcn_bwd_contrib, stif_dec_x3_bwd_contrib, the
``deterministic=True`` paths of ops.dcn_bwd / ops.dec_x3_bwd and the switch of the train module.

The ordered sum has a value that does not depend on the kernel: tests/segsum_ref.py computes it in numpy from the
definition in include/stif.h (pinned by tests/test_deterministic_host.py), and the kernels are held to it bit for bit,
on inputs for which another order of the same terms gives other bits (asserted).  Everything else reuses the inputs,
float64 references and tolerances of the atomic paths' own files: tests/test_gpu_dcn_bwd.py (RTOL_DCN = 2e-5 of
max |ref|, the data kernel's tile-edge shapes), tests/test_gpu_dec_train.py (RTOL = 1e-5 for the builders' adjoints,
``chain_tol`` for the decoder) and tests/test_gpu_pcd_train.py (the DCN_sep module case).  Outputs are pre-filled with
NaN, index buffers with -1."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import segsum_ref as S
import test_gpu_dcn_bwd as TD
import test_gpu_dec_train as TT
import test_gpu_pcd_train as TP

pytestmark = pytest.mark.gpu

NAN = float("nan")
RTOL_DCN = TD.RTOL_DCN


def bits(t):
    t = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(t).view(np.int32)


def same_bits(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and bool(np.array_equal(a, b))


def stream():
    return torch.cuda.current_stream().cuda_stream


# ---- 1. stif_segsum against the emulation ----

# C: (D, K, col0, row_stride, E) -- K, col0 and row_stride of the three uses; D * C / 4 lanes fill more than one
# 256-lane workgroup and the last one only partly
SEG_CASES = {8: (301, 72, 0, 576, 5760), 64: (53, 2, 0, 528, 5600), 192: (19, 2, 128, 528, 5600)}
LONG = 2 * S.CHUNK + 3


@functools.lru_cache(maxsize=None)
def segsum_case(Cc):
    D, K, col0, row_stride, E = SEG_CASES[Cc]
    rng = np.random.default_rng(40 + Cc)
    empty, single, long_row = (1, D - 1), 2, 4
    allowed = np.array([d for d in range(D + 1) if d not in empty + (single, long_row)])   # D itself: the sentinel
    key = rng.choice(allowed, E)
    where = rng.permutation(E)
    key[where[:LONG]] = long_row
    key[where[LONG]] = single
    w = rng.random(E, dtype=np.float32)
    src = rng.standard_normal(((E // 4 + K - 1) // K) * row_stride).astype(np.float32)
    rows = S.sub_rows(src, E, row_stride, K, Cc, col0)
    words = S.pack(key)
    ref = S.emulate(words, w, rows, D)
    counts = np.bincount(key, minlength=D + 1)
    assert counts[long_row] == LONG and counts[single] == 1 and counts[D] > 0 and not counts[list(empty)].any()
    return key, w, src, words, ref, S.emulate(words, w, rows, D, reverse=True)


@pytest.mark.parametrize("Cc", sorted(SEG_CASES))
def test_segsum_is_the_emulation_bit_for_bit(stif, Cc):
    D, K, col0, row_stride, E = SEG_CASES[Cc]
    key, w, src, words, ref, rev = segsum_case(Cc)
    changed = float((bits(rev) != bits(ref)).mean())
    print(f"C = {Cc}: reversing every list changes {100 * changed:.0f} % of the elements")
    assert changed > 0.25, "the order must matter on these inputs, or the comparison below shows nothing"
    srt, seg = S.sorted_segments(words, D)
    dev_srt, dev_seg = stif.ops._sorted_segments(torch.from_numpy(words).cuda(), D)
    assert np.array_equal(dev_srt.cpu().numpy(), srt) and np.array_equal(dev_seg.cpu().numpy(), seg)
    dst = torch.full((D + 1, Cc), NAN, device="cuda")
    out = stif.ops.segsum(dst[:D], torch.from_numpy(src).cuda(), row_stride, K, col0, torch.from_numpy(w).cuda(),
                          dev_srt, dev_seg)
    torch.cuda.synchronize()
    assert out.data_ptr() == dst.data_ptr() and bool(torch.isnan(dst[D]).all())
    got = dst[:D].cpu().numpy()
    assert not np.isnan(got).any()
    assert np.array_equal(bits(got[[1, D - 1]]), np.zeros((2, Cc), np.int32)), "an empty list is +0.0"
    bad = np.flatnonzero((bits(got) != bits(ref)).any(1))
    assert bad.size == 0, (Cc, bad[:8], float(np.abs(got - ref).max()))


# ---- 2. the deformable conv ----

SHAPES = ["1x1x1", "2x5x7", "1x3x33", "3x33x70"]


def ordered_call(stif, m, lrelu=False):
    """stif_dcn_bwd_contrib through the C ABI on NaN / -1 filled buffers, the sort, stif_segsum into a NaN-filled g_in"""
    L, ops = stif._lib, stif.ops
    px = m.n * m.H * m.W
    E, D = px * 288, px * 8
    a = L.DcnBwdContribArgs()
    a.inp, a.offmask, a.w, a.gout = m.inp.data_ptr(), m.offmask.data_ptr(), m.weight.data_ptr(), m.gout.data_ptr()
    a.in_item, a.om_item, a.gout_item = m.in_item, m.om_item, m.gout_item
    if lrelu:
        a.out, a.out_item, a.epi = m.out.data_ptr(), m.out_item, L.EPI_LRELU
    g_om, a.gom_item = m.empty(256)
    cm = torch.full((px, 576), NAN, device="cuda")
    wgt = torch.full((E,), NAN, device="cuda")
    words = torch.full((E,), -1, dtype=torch.int64, device="cuda")
    a.g_om, a.cm, a.wgt, a.words = g_om.data_ptr(), cm.data_ptr(), wgt.data_ptr(), words.data_ptr()
    a.n, a.H, a.W = m.n, m.H, m.W
    L.check(L.lib().stif_dcn_bwd_contrib(C.byref(a), stream()), "stif_dcn_bwd_contrib")
    g_in = torch.full((m.n, m.H, m.W, 64), NAN, device="cuda")
    ops.segsum(g_in.view(D, 8), cm, 576, 72, 0, wgt, *ops._sorted_segments(words, D))
    torch.cuda.synchronize()
    return dict(g_in=g_in, g_om=g_om, cm=cm, wgt=wgt, words=words)


@pytest.mark.parametrize("name", SHAPES)
def test_dcn_exact_inputs_give_the_reference_bit_for_bit(stif, name):
    t, ref = TD.exact_case(name)
    got = ordered_call(stif, TD.Maps(*t))
    for k in ("g_in", "g_om"):
        assert torch.equal(got[k].cpu().double(), ref[k]), (k, TD.relmax(got[k], ref[k]))
    assert not bool(torch.isnan(got["cm"]).any()) and not bool(torch.isnan(got["wgt"]).any())
    assert int(got["words"].min()) >= 0


@pytest.mark.parametrize("lrelu", [False, True], ids=["none", "lrelu"])
@pytest.mark.parametrize("name", SHAPES)
def test_dcn_tamed_inputs_against_float64_and_g_om_keeps_its_bytes(stif, name, lrelu):
    t, refs = TD.tame_case(name)
    out, ref = refs[lrelu]
    m = TD.Maps(*t, out=out if lrelu else None)
    got = ordered_call(stif, m, lrelu=lrelu)
    errs = {k: TD.relmax(got[k], ref[k]) for k in ("g_in", "g_om")}
    print(name, lrelu, errs)
    assert errs["g_in"] <= RTOL_DCN and errs["g_om"] <= RTOL_DCN, errs
    atomic, _ = TD.call(stif, m, need=(False, True, False), lrelu=lrelu)
    assert TD.same_bytes(got["g_om"], atomic["g_om"])


def test_dcn_wild_offsets_against_the_drop_in(stif):
    ops = stif.ops
    inp, offset, mask, weight, gout = (t.cuda() for t in TD.wild_inputs((3, 33, 70), 3 + 33))
    gi = ops.dcn_v2_backward(inp, weight, torch.zeros(64, device="cuda"), offset, mask, gout, *TD.GEOM)[0]
    args = (TD.nhwc(inp), TD.to_offmask(offset, mask), weight, TD.nhwc(gout))
    got = ops.dcn_bwd(*args, deterministic=True)
    err = TD.relmax(got[0], TD.nhwc(gi))
    print("3x33x70 wild g_in", err)
    assert err <= RTOL_DCN
    atomic = ops.dcn_bwd(*args)
    for k, a, b in zip(TD.OUTS[1:], got[1:], atomic[1:]):      # g_om, g_w and g_b are untouched
        assert TD.same_bytes(a, b), k


def expected_entries(m):
    """keys [E] and weights [E] of the entry numbering e = ((p * 8 + g) * 9 + k) * 4 + j, in the kernel's float32
    expressions (dcn_bilinear.h): position (y - 1 + ky) + dy, corners low/low, low/high, high/low, high/high."""
    n, H, W = m.n, m.H, m.W
    om = m.offmask.cpu().numpy().reshape(n, H, W, 8, 9, 3)
    ky, kx = np.divmod(np.arange(9), 3)
    y = np.arange(H, dtype=np.float32).reshape(1, H, 1, 1, 1)
    x = np.arange(W, dtype=np.float32).reshape(1, 1, W, 1, 1)
    h = (y - 1 + ky.astype(np.float32)) + om[..., 0]
    w = (x - 1 + kx.astype(np.float32)) + om[..., 1]
    assert h.dtype == w.dtype == np.float32
    valid = (h > -1) & (w > -1) & (h < H) & (w < W)
    fh, fw = np.floor(h), np.floor(w)
    lh, lw = h - fh, w - fw
    hh, hw = np.float32(1) - lh, np.float32(1) - lw
    hl, wl = fh.astype(np.int64), fw.astype(np.int64)
    item = np.arange(n).reshape(n, 1, 1, 1, 1)
    g = np.arange(8).reshape(1, 1, 1, 8, 1)
    keys, wts = [], []
    for (cy, cx, wt) in ((hl, wl, hh * hw), (hl, wl + 1, hh * lw), (hl + 1, wl, lh * hw), (hl + 1, wl + 1, lh * lw)):
        ok = valid & (cy >= 0) & (cy <= H - 1) & (cx >= 0) & (cx <= W - 1)
        keys.append(np.where(ok, ((item * H + cy) * W + cx) * 8 + g, n * H * W * 8))
        wts.append(np.where(ok, wt, np.float32(0)).astype(np.float32))
    return np.stack(keys, -1).reshape(-1), np.stack(wts, -1).reshape(-1)


def check_against_emulation(m, got):
    E, D = m.n * m.H * m.W * 288, m.n * m.H * m.W * 8
    words = got["words"].cpu().numpy()
    assert np.array_equal(words & 0xffffffff, np.arange(E)), "the low word is the entry id"
    keys, wts = expected_entries(m)
    assert np.array_equal(words >> 32, keys), "entry numbering"
    assert np.array_equal(bits(got["wgt"]), bits(wts)), "corner weights"
    cm = got["cm"].cpu().numpy().reshape(-1, 8)
    dead = (keys.reshape(-1, 4) == D).all(1)
    assert not cm[dead].any(), "a sub-row no corner of which counts is zero"
    ref = S.emulate(words, wts, cm, D)
    assert np.array_equal(bits(got["g_in"].cpu().numpy().reshape(D, 8)), bits(ref))
    return keys, ref, S.emulate(words, wts, cm, D, reverse=True)


def test_dcn_entry_numbering_and_order_at_2x5x7(stif):
    t, refs = TD.tame_case("2x5x7")
    m = TD.Maps(*t)
    got = ordered_call(stif, m)
    keys, ref, rev = check_against_emulation(m, got)
    assert int((keys == m.n * m.H * m.W * 8).sum()) > 0, "border samples have corners that do not count"
    assert float((bits(rev) != bits(ref)).mean()) > 0.25


def test_dcn_every_sample_on_one_pixel(stif):
    """Every (pixel, tap) of an item samples (4.25, 6.5) of 5 x 7: only the low/low corner (4, 6) lies in the frame, so
    each item has eight lists of 35 * 9 entries and 34 * 8 empty ones."""
    n, H, W = 2, 5, 7
    inp, _, mask, weight, gout = (v.clone() for v in TD.tame_case("2x5x7")[0])
    ky, kx = np.divmod(np.arange(9), 3)
    y, x = torch.arange(H).view(H, 1, 1).double(), torch.arange(W).view(1, W, 1).double()
    dy = 4.25 - (y - 1 + torch.from_numpy(ky).double())            # [H, 1, 9]
    dx = 6.5 - (x - 1 + torch.from_numpy(kx).double())             # [1, W, 9]
    off = torch.stack([dy.expand(H, W, 9), dx.expand(H, W, 9)], -1)           # [H, W, 9, 2]
    offset = off.permute(2, 3, 0, 1).reshape(1, 1, 18, H, W).expand(n, 8, 18, H, W).reshape(n, 144, H, W).contiguous()
    t = (inp, offset, mask, weight, gout)
    m = TD.Maps(*t)
    got = ordered_call(stif, m)
    keys, ref, rev = check_against_emulation(m, got)
    lists = np.bincount(keys, minlength=n * H * W * 8 + 1)[:-1].reshape(n, H * W, 8)
    assert (lists[:, -1] == 35 * 9).all() and not lists[:, :-1].any()
    assert float((bits(rev) != bits(ref)).mean()) > 0.25 * 16 / (n * H * W * 8)     # of the 16 rows that are not empty
    _, r64 = TD.reference(*t, lrelu=False)
    assert TD.relmax(got["g_in"], r64["g_in"]) <= RTOL_DCN and TD.relmax(got["g_om"], r64["g_om"]) <= RTOL_DCN
    assert not bool(got["g_in"][:, :4].any()) and not bool(got["g_in"][:, 4, :6].any())


def test_dcn_two_calls_give_the_same_bytes_and_chunking_changes_nothing(stif, monkeypatch):
    ops = stif.ops
    t, refs = TD.tame_case("3x33x70")
    m = TD.Maps(*t, out=refs[True][0])
    first, second = ordered_call(stif, m, lrelu=True), ordered_call(stif, m, lrelu=True)
    for k in first:
        assert TD.same_bytes(first[k].view(torch.float32), second[k].view(torch.float32)), k
    args = (m.inp, m.offmask, m.weight, m.gout)
    whole = ops.dcn_bwd(*args, out=m.out, epi=stif._lib.EPI_LRELU, deterministic=True)
    monkeypatch.setattr(ops, "DET_TRANSIENT_BYTES", 1)              # one item per chunk
    chunks = []
    real = stif._lib.lib().stif_dcn_bwd_contrib
    monkeypatch.setattr(stif._lib.lib(), "stif_dcn_bwd_contrib", lambda a, s: chunks.append(a._obj.n) or real(a, s))
    parts = ops.dcn_bwd(*args, out=m.out, epi=stif._lib.EPI_LRELU, deterministic=True)
    assert chunks == [1, 1, 1]
    for k, a, b in zip(TD.OUTS, whole, parts):
        assert TD.same_bytes(a, b), k
    assert TD.same_bytes(whole[0], first["g_in"]) and TD.same_bytes(whole[1], first["g_om"])
    g_in_only = ops.dcn_bwd(*args, out=m.out, epi=stif._lib.EPI_LRELU, need=(True, False, False), deterministic=True)
    assert TD.same_bytes(g_in_only[0], whole[0]) and g_in_only[1:] == (None, None, None)


# ---- 3. the decoder's warped gather ----

def x3_contrib(stif, geom, hr, fl, g3):
    L = stif._lib
    E = 8 * geom.N
    g_flow = TT.nan_like((geom.N, 4))
    w = [torch.full((E,), NAN, device="cuda") for _ in range(2)]
    words = [torch.full((E,), -1, dtype=torch.int64, device="cuda") for _ in range(2)]
    rc = L.lib().stif_dec_x3_bwd_contrib(C.byref(geom.c), hr.data_ptr(), fl.data_ptr(), g3.data_ptr(), g_flow.data_ptr(),
                                         w[0].data_ptr(), words[0].data_ptr(), w[1].data_ptr(), words[1].data_ptr(),
                                         stream())
    L.check(rc, "stif_dec_x3_bwd_contrib")
    torch.cuda.synchronize()
    return g_flow, w, words


@pytest.mark.parametrize("name", sorted(TT.SIZES))
def test_x3_adjoint_ordered(stif, name):
    ops = stif.ops
    B, H, W, HH, WW = TT.SIZES[name]
    N, E = B * HH * WW, 8 * B * HH * WW
    feat, inp, t, hrfeat, flow, (gx1, gx2, gx3), ref = TT.builder_case(name)
    geom = TT.make_geom(stif, name)
    hr, fl, g3 = hrfeat.reshape(N, 64).cuda(), flow.reshape(N, 4).cuda(), gx3.reshape(N, 528).cuda()
    atomic = ops.dec_x3_bwd(geom, hr, fl, g3, TT.nan_like((N, 4)))
    g_flow, w, words = x3_contrib(stif, geom, hr, fl, g3)
    assert TT.same_bytes(g_flow, atomic[0])
    print(f"{name}:")
    got = []
    for k, (Cc, col0, D) in enumerate(((64, 0, N), (192, 128, B * H * W))):
        wk, wordk = w[k].cpu().numpy(), words[k].cpu().numpy()
        assert not np.isnan(wk).any() and np.array_equal(wordk & 0xffffffff, np.arange(E))
        keys = wordk >> 32
        assert keys.min() >= 0 and keys.max() == D, "clamped grids put corners outside the map (the sentinel)"
        dst = torch.full((D, Cc), NAN, device="cuda")
        ops.segsum(dst, g3, 528, 2, col0, w[k], *ops._sorted_segments(words[k], D))
        rows = S.sub_rows(gx3.numpy(), E, 528, 2, Cc, col0)
        emu = S.emulate(wordk, wk, rows, D)
        assert np.array_equal(bits(dst), bits(emu)), ("g_hrfeat", "g_feat")[k]
        if D > 1:
            assert float((bits(S.emulate(wordk, wk, rows, D, reverse=True)) != bits(emu)).mean()) > 0.05
        got.append(dst)
    TT.check("ordered g_hrfeat", got[0], ref["g_hr3"].reshape(N, 64), TT.RTOL)
    TT.check("ordered g_feat", got[1].view(B, H, W, 192), TT.nhwc_lat(ref["g_feat3"]), TT.RTOL)
    one = ops.dec_x3_bwd(geom, hr, fl, g3, TT.nan_like((N, 4)), deterministic=True)
    two = ops.dec_x3_bwd(geom, hr, fl, g3, TT.nan_like((N, 4)), deterministic=True)
    for a, b, c in zip(one, two, (g_flow, got[0], got[1].view(B, H, W, 192))):
        assert TT.same_bytes(a, b) and TT.same_bytes(a, c)


# ---- 4. the modules under the switch ----

ENTRIES = ("stif_dcn_bwd_nhwc", "stif_dcn_bwd_contrib", "stif_dec_x3_bwd", "stif_dec_x3_bwd_contrib", "stif_segsum")


@pytest.fixture
def calls(stif, monkeypatch):
    """How often each entry point of the two paths is called (a counting wrapper on the loaded library)."""
    lib, n = stif._lib.lib(), dict.fromkeys(ENTRIES, 0)

    def counting(name, fn):
        def wrapper(*args):
            n[name] += 1
            return fn(*args)
        return wrapper

    for name in ENTRIES:
        monkeypatch.setattr(lib, name, counting(name, getattr(lib, name)))
    return n


def dcn_module_grads(stif, inp, fea, gout, P):
    m = stif.train.DCN_sep("lrelu", "f32")
    m.load_state_dict({k: v.float() for k, v in P.items()}, strict=True)
    m = m.cuda()
    ig, fg = TP.gpu_leaf(inp), TP.gpu_leaf(fea)
    m(ig, fg).backward(gout.float().cuda())
    return {"input": ig.grad, "fea": fg.grad, **{k: p.grad for k, p in m.named_parameters()}}


def test_dcn_sep_module_under_the_switch(stif, calls):
    TR = stif.train
    shape = (2, 12, 20)
    inp, fea, gout, P = TP.dcn_module_case(shape, sum(shape))
    Pr = {k: TP.leaf(v) for k, v in P.items()}
    ir, fr = TP.leaf(inp), TP.leaf(fea)
    offset, mask = TP.R.offset_mask(fr, Pr["conv_offset_mask.weight"], Pr["conv_offset_mask.bias"])
    TP.R.lrelu(TP.R.dcn(ir, offset, mask, Pr["weight"], Pr["bias"])).backward(gout)
    want = {"input": ir.grad, "fea": fr.grad, **{k: v.grad for k, v in Pr.items()}}
    off = dcn_module_grads(stif, inp, fea, gout, P)
    assert calls["stif_dcn_bwd_nhwc"] == 1 and calls["stif_dcn_bwd_contrib"] == 0 and calls["stif_segsum"] == 0
    with TR.deterministic():
        on = dcn_module_grads(stif, inp, fea, gout, P)
        again = dcn_module_grads(stif, inp, fea, gout, P)
    assert calls["stif_dcn_bwd_contrib"] == 2 and calls["stif_segsum"] == 2
    assert calls["stif_dcn_bwd_nhwc"] == 3, "the weight kernel alone, once per deterministic backward"
    for k in want:
        TP.check("deterministic g_" + k, on[k], want[k], RTOL_DCN)
        assert TD.same_bytes(on[k], again[k]), k
        if k != "input":
            assert TD.same_bytes(on[k], off[k]), k


def decoder_grads(stif, B, H, W, HH, WW):
    feat, inp, G, P = TT.decoder_case(B, H, W, HH, WW)[:4]
    dec = stif.train.Decoder()
    dec.load_state_dict(P, strict=True)
    dec = dec.cuda()
    fd = feat.cuda().requires_grad_(True)
    outs = dec(fd, inp.cuda(), [torch.full((B, 1), TT.DEC_TIMES[0]), TT.DEC_TIMES[1]], (HH, WW))
    sum((o * g.cuda()).sum() for o, g in zip(outs, G)).backward()
    return outs, fd.grad, {k: p.grad for k, p in dec.named_parameters()}


def test_decoder_module_under_the_switch(stif, calls):
    TR = stif.train
    size = TT.DEC_SIZES[0]
    r64, r32 = TT.decoder_case(*size)[4:]
    decoder_grads(stif, *size)
    assert calls["stif_dec_x3_bwd"] == 2 and calls["stif_dec_x3_bwd_contrib"] == 0 and calls["stif_segsum"] == 0
    with TR.deterministic():
        outs, g_feat, grads = decoder_grads(stif, *size)
        _, g_feat2, grads2 = decoder_grads(stif, *size)
    assert calls["stif_dec_x3_bwd"] == 2 and calls["stif_dec_x3_bwd_contrib"] == 4 and calls["stif_segsum"] == 8
    for i, o in enumerate(outs):
        TT.check(f"pred[{i}]", o, r64[0][i], TT.chain_tol(r64[0][i], r32[0][i]))
    TT.check("g_feat", g_feat, r64[3], TT.chain_tol(r64[3], r32[3]))
    assert TT.same_bytes(g_feat, g_feat2)
    assert len(grads) == 26
    for k in sorted(grads):
        TT.check("g " + k, grads[k], r64[2][k], TT.chain_tol(r64[2][k], r32[2][k]))
        assert TT.same_bytes(grads[k], grads2[k]), k


# ---- 5. the whole model ----

def two_steps(stif, sd, x, times, gt):
    TR = stif.train
    net = TR.LunaTokis(5, 40)
    net.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in sd.items()}, strict=True)
    net = net.cuda()
    opt, _ = TR.make_optimizer(net, dict(lr_G=1e-4, beta1=0.9, beta2=0.99, lr_scheme="MultiStepLR", lr_steps=[10],
                                         lr_gamma=0.5))
    crit = TR.TimesLoss(TR.CharbonnierLoss())
    losses = [TR.optimize_step(net, opt, crit, (x, times, (16, 24)), gt) for _ in range(2)]
    assert net.range_status() == 0
    return losses, net


def test_two_nets_take_the_same_two_steps(stif, sd, calls):
    TR = stif.train
    g = torch.Generator().manual_seed(11)
    x = torch.rand(1, 2, 3, 8, 12, generator=g).cuda()
    times = [torch.tensor([[0.25]]), torch.tensor([[0.75]])]
    gt = torch.rand(1, 2, 3, 16, 24, generator=g).cuda()
    with TR.deterministic():
        la, a = two_steps(stif, sd, x, times, gt)
        lb, b = two_steps(stif, sd, x, times, gt)
    assert not TR.is_deterministic()
    assert calls["stif_dec_x3_bwd"] == 0 and calls["stif_dec_x3_bwd_contrib"] > 0 and calls["stif_dcn_bwd_contrib"] > 0
    assert all(np.isfinite(v) and v > 0 for v in la) and la == lb and la[0] != la[1]
    pa, pb = dict(a.named_parameters()), dict(b.named_parameters())
    assert len(pa) == 442
    grads = 0
    for k in pa:
        assert TD.same_bytes(pa[k].detach(), pb[k].detach()), k
        assert (pa[k].grad is None) == (pb[k].grad is None), k
        if pa[k].grad is not None:
            grads += 1
            assert bool(torch.isfinite(pa[k].grad).all()) and TD.same_bytes(pa[k].grad, pb[k].grad), k
    assert grads == 434
