"""The BiConvLSTM's first step once per frame on the window path, against the per-pair path, bit for bit.

Step 0 of either recurrence reads one frame and the all-zero state through the same weights, so reversed step 0 of
pair b and forward step 0 of pair b + 1 are one computation (model.step0_plan).  gen_feat_window runs it per frame;
gen_feat on the same pairs keeps the per-pair form.  Every kernel computes an item from that item's maps alone, so
the latents must be equal bit for bit (torch.equal) -- for both operand modes, under pair chunking, lanes, the
directions on two streams, trunk lanes, a PCD side stream and precomputed frame features, and when the cached zero
state maps of one window length are followed by another length."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

WINDOWS = [(7, 16, 16), (5, 12, 20), (2, 16, 16)]       # (frames, H, W); two frames: one pair, nothing shared
MODES = ["f16x3", "f32"]
FRONT, BACK = 5, 40
_REF = {}


def frames_of(win):
    n, H, W = win
    return torch.rand(n, 3, H, W, generator=torch.Generator().manual_seed(100 * n + H + W)).cuda()


@pytest.fixture(scope="module")
def models(stif, sd):
    ms = {}
    for mf in MODES:
        m = stif.LunaTokis(64, 6, 8, FRONT, BACK, mfma=mf)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
        ms[mf] = m.eval()
    return ms


def pairs_latent(models, mf, win):
    """The per-pair path's latent [3, B, H, W, 64] of the window's adjacent pairs: once per (mode, window)."""
    if (mf, win) not in _REF:
        fr = frames_of(win)
        with torch.no_grad():
            models[mf].gen_feat(torch.stack([fr[:-1], fr[1:]], dim=1))
            _REF[mf, win] = models[mf]._feat.clone()
    return _REF[mf, win]


def window_latent(m, fr, **kw):
    with torch.no_grad():
        m.gen_feat_window(fr, **kw)
        return m._feat.clone()


class Settings:
    """Set attributes of the model for one block, then put them back."""

    def __init__(self, m, **kw):
        self.m, self.kw = m, kw

    def __enter__(self):
        self.keep = {k: getattr(self.m, k) for k in self.kw}
        for k, v in self.kw.items():
            setattr(self.m, k, v)

    def __exit__(self, *exc):
        for k, v in self.keep.items():
            setattr(self.m, k, v)


@pytest.mark.parametrize("mf", MODES)
@pytest.mark.parametrize("win", WINDOWS, ids=lambda w: "x".join(map(str, w)))
def test_window_equals_pairs(models, mf, win):
    m = models[mf]
    ref, fr = pairs_latent(models, mf, win), frames_of(win)
    assert torch.isfinite(ref).all()
    assert torch.equal(window_latent(m, fr), ref)


def variants(win):
    n, H, W = win
    B = n - 1
    return {
        "chunks2": dict(chunk_px=math.ceil(B / 2) * H * W),
        "chunks3": dict(chunk_px=math.ceil(B / 3) * H * W),
        "lanes2": dict(lanes=2),
        "lstm_lanes2": dict(lstm_lanes=2),
        "trunk_lanes1": dict(trunk_lanes=1),
        "trunk_lanes2": dict(trunk_lanes=2),
        "pcd_streams2": dict(pcd_streams=2),
        "all": dict(chunk_px=math.ceil(B / 2) * H * W, lanes=2, lstm_lanes=2, trunk_lanes=2, pcd_streams=2),
    }


@pytest.mark.parametrize("mf", MODES)
@pytest.mark.parametrize("name", sorted(variants(WINDOWS[0])))
@pytest.mark.parametrize("win", WINDOWS, ids=lambda w: "x".join(map(str, w)))
def test_window_equals_pairs_under_chunks_and_lanes(models, mf, win, name):
    m = models[mf]
    ref, fr = pairs_latent(models, mf, win), frames_of(win)
    kw = variants(win)[name]
    if win == WINDOWS[0] and name.startswith("chunks"):       # 6 pairs: 3 + 3 and 2 + 2 + 2
        B, per = win[0] - 1, max(1, kw["chunk_px"] // (win[1] * win[2]))
        assert math.ceil(B / per) == int(name[-1])
    with Settings(m, **kw):
        assert torch.equal(window_latent(m, fr), ref), (name, kw)


@pytest.mark.parametrize("mf", MODES)
@pytest.mark.parametrize("win", WINDOWS, ids=lambda w: "x".join(map(str, w)))
def test_frame_feats_entries(models, mf, win):
    """Precomputed features of every frame (frame_feats=) and of the last frame only (last_frame_feats=)."""
    m = models[mf]
    ref, fr = pairs_latent(models, mf, win), frames_of(win)
    with torch.no_grad():
        feats = m.frame_features(fr)
    assert torch.equal(window_latent(m, fr, frame_feats=feats), ref)
    assert torch.equal(window_latent(m, fr, frame_feats=tuple(f.clone() for f in feats)), ref)
    assert torch.equal(window_latent(m, fr, last_frame_feats=tuple(f[-1] for f in feats)), ref)
    with Settings(m, lanes=2, chunk_px=2 * win[1] * win[2]):
        assert torch.equal(window_latent(m, fr, frame_feats=feats), ref)


@pytest.mark.parametrize("mf", MODES)
def test_caches_across_calls_and_window_lengths(models, mf):
    """Two calls in a row (the second finds the zero-state maps of 7 frames cached), then 5 frames of the same size,
    then 7 again: every call equals its per-pair reference."""
    m = models[mf]
    a, b = (7, 16, 16), (5, 16, 16)
    for win in (a, a, b, a, b):
        assert torch.equal(window_latent(m, frames_of(win)), pairs_latent(models, mf, win)), win


def test_fp32_rerun_follows_the_same_plan(stif, models):
    """range_check="rerun" on the window path: the first fused DCN_sep launch sees one offset feature of 5000 (outside
    the split-fp16 range) and sets the status word; the call runs again on the fp32 layers -- per-frame step 0 again,
    through the conv + DCN pair instead of the fused kernel -- and the latent equals the fp32 model's per-pair one."""
    import warnings
    ops, m = stif.ops, models["f16x3"]
    win = WINDOWS[0]
    ref, fr = pairs_latent(models, "f32", win), frames_of(win)
    orig, seen = ops.dcn_sep, []

    def poisoned(groups, epi=0, status=None):
        if seen:
            return orig(groups, epi=epi, status=status)
        g0 = dict(groups[0])
        g0["fea"] = g0["fea"].clone()
        g0["fea"].view(-1)[g0["fea"].numel() // 3] = 5000.0
        orig([g0] + list(groups[1:]), epi=epi, status=status)
        seen.append(1)
    before = m.range_reruns
    ops.dcn_sep = poisoned
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            got = window_latent(m, fr)
    finally:
        ops.dcn_sep = orig
    assert seen == [1] and m.range_reruns == before + 1
    assert torch.equal(got, ref)


class Recorder:
    def __init__(self):
        self.launches = []

    def begin(self, kind, flops, nbytes=None):
        self.launches.append((kind, flops))

    def end(self):
        pass


def predicted_flops(stif, frames_encoded, B, H, W, window):
    """Algorithmic FLOPs of the encoder from the planner's item counts (ops.py's TRACE formulas per item)."""
    px = H * W
    c3 = lambda cout, cin, div=1: 2.0 * cout * cin * 9 * px // div
    sep = lambda div: 2.0 * (216 + 64) * 576 * px // div
    pyr = 2 * c3(64, 64, 4) + 2 * c3(64, 64, 16)
    l1_offsets = 2 * c3(64, 128) + c3(64, 64) + sep(1)
    unit_zero = (c3(64, 128, 16) + c3(64, 64, 16) + sep(16)                              # L3
                 + 3 * c3(64, 128, 4) + c3(64, 64, 4) + sep(4)                            # L2
                 + c3(64, 128))                                                           # L1_fea_conv
    unit = unit_zero + l1_offsets
    fus, cell = 2.0 * 64 * 128 * px, c3(256, 128)
    plan = stif.model.step0_plan(B, window)
    la = plan["launches"]
    total = frames_encoded * (FRONT * 2 * c3(64, 64) + pyr)
    total += sum(la["first_pcd"]) * unit + sum(la["first_fusion"]) * fus
    total += (sum(la["input_pyramid"]) + sum(la["step1_pyramid"])) * pyr
    total += sum(n * (unit_zero if i in plan["zero_l1"] else unit) for i, n in enumerate(la["step0_pcd"]))
    total += sum(la["step0_fusion"]) * fus + sum(la["step0_cell"]) * cell
    total += 4 * B * pyr                                                                  # step 2's state pyramids
    total += 2 * (8 * B * unit + 4 * B * fus + 2 * B * cell)                              # steps 1 and 2
    total += 3 * B * fus + BACK * 2 * 3 * B * c3(64, 64)                                  # conv_1x1, recon trunk
    return total


@pytest.mark.parametrize("mf", MODES)
def test_traced_launches_and_flops_follow_the_plan(stif, models, mf):
    """ops.TRACE over the 7-frame window's encoder and over its six pairs on the per-pair path: the same number of
    launches (the per-frame step 0 runs the kernels of the per-pair one, on 7 items per weight set instead of 12),
    total algorithmic FLOPs equal to what the planner's item counts give for either path, and the ConvLSTM cell
    launched once on 7 items (step 0) and twice on two sets of 6 (steps 1 and 2)."""
    m, ops, L = models[mf], stif.ops, stif._lib
    win = WINDOWS[0]
    n, H, W = win
    B, fr = n - 1, frames_of(win)
    cells, orig = [], ops.conv2d

    def conv2d(groups, **kw):
        if kw.get("epi") == L.EPI_LSTM:
            cells.append(tuple(g["in0"].shape[0] for g in groups))
        return orig(groups, **kw)
    rec = {}
    pairs_in = torch.stack([fr[:-1], fr[1:]], dim=1)
    with torch.no_grad():            # the zero-state maps of both item counts cached: the traced runs compute none
        m.gen_feat(pairs_in)
        m.gen_feat_window(fr)
    ops.conv2d = conv2d
    try:
        for path in ("window", "pairs"):
            rec[path], keep = Recorder(), ops.TRACE
            ops.TRACE = rec[path]
            try:
                with torch.no_grad():
                    if path == "window":
                        m.gen_feat_window(fr)
                    else:
                        m.gen_feat(pairs_in)
            finally:
                ops.TRACE = keep
    finally:
        ops.conv2d = orig
    torch.cuda.synchronize()
    assert cells == [(n,), (B, B), (B, B), (B, B), (B, B), (B, B)], cells          # window, then pairs (3 steps)
    got = {p: sum(f for _, f in r.launches) for p, r in rec.items()}
    print(f"{mf}: launches window {len(rec['window'].launches)} pairs {len(rec['pairs'].launches)}; "
          f"GFLOP window {got['window'] / 1e9:.4f} pairs {got['pairs'] / 1e9:.4f}")
    assert len(rec["window"].launches) == len(rec["pairs"].launches)
    assert got["pairs"] == predicted_flops(stif, 2 * B, B, H, W, False)
    assert got["window"] == predicted_flops(stif, n, B, H, W, True)
    assert got["window"] < got["pairs"]
