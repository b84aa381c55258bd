"""The model at the smallest frames ``LunaTokis._check_input`` accepts, against the float64 oracle.

A 4 x 4 frame is legal (sides are multiples of 4) and its pyramid levels are 4 x 4, 2 x 2 and 1 x 1: every conv, DCN
and upsample of PCD_Align and of the BiConvLSTM's Easy_PCD runs on maps smaller than a tile, the decoder's LR
projection on items (16 pixels) smaller than one 32-pixel M-tile.  L3 of the cases below is 1x1, 1x2, 2x1, 3x5 and
5x3 (odd: the Winograd 2x2 sub-tiles and the x2 upsample's border clamps meet in one tile); B = 2 puts two different
pairs into one batch.

Bar: the project's model bar, |gpu - ref| <= 1e-4 |ref| + 1e-6 for every element (``close`` of
tests/test_gpu_model.py).  The oracle evaluated in float32 stays at or below 0.045 of that bound on every encoder
stage and 0.016 on the outputs at these sizes, so the reference leaves a margin of more than 20x.  Every test prints
its worst ratio to the bound (``pytest -s``)."""
import numpy as np
import pytest
import torch

from oracle import stif_oracle as O

pytestmark = pytest.mark.gpu

RTOL = 1e-4
ATOL = 1e-6
CASES = [(1, 4, 4), (2, 4, 8), (2, 8, 4), (2, 12, 20), (1, 20, 12)]
TIMES = [0.0, float(np.float32(0.37)), 1.0]       # 0.37 as the float32 the engine decodes at
T1 = TIMES[1]
KINDS = {"f16x3": dict(mfma="f16x3"), "f32": dict(mfma="f32"), "direct": dict(winograd=False)}
# every case on both operand modes; the direct-conv model (winograd=False) at 4 x 8 and 12 x 20
RUNS = [(c, k) for c in CASES for k in ("f16x3", "f32")] + [(c, "direct") for c in ((2, 4, 8), (2, 12, 20))]
run_id = lambda r: f"{r[0][0]}x{r[0][1]}x{r[0][2]}-{r[1]}"
RUNS_B2 = [r for r in RUNS if r[0][0] == 2]

_ORACLE, _GPU = {}, {}


def close(a, b, rtol=RTOL, atol=ATOL):
    """(ok, max |a - b|, worst ratio of |a - b| to its elementwise bound); a non-finite element fails"""
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    b = np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    d = np.abs(a - b)
    lim = rtol * np.abs(b) + atol
    return bool((d <= lim).all()), float(d.max()), float((d / lim).max())


def frames(case):
    B, H, W = case
    return np.random.default_rng(100 * H + W).random((B, 2, 3, H, W)).astype(np.float32)


def grid_of(case):
    """a decode size that is no multiple of the frame"""
    _, H, W = case
    return 2 * H + 1, 3 * W - 1


def oracle(case, sd):
    """Stage captures, latent and outputs of the float64 oracle, once per case."""
    if case not in _ORACLE:
        x = frames(case)
        cap = {}
        outs = O.forward(x, TIMES, sd, capture=cap)
        _ORACLE[case] = dict(x=x, cap=cap, outs=outs, scaled=O.decoding(cap["feat"], x, [T1], sd, scale=grid_of(case))[0])
    return _ORACLE[case]


@pytest.fixture(scope="module")
def models(stif, sd):
    made = {}

    def get(kind):
        if kind not in made:
            m = stif.LunaTokis(64, 6, 8, 5, 40, **KINDS[kind])
            m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
            made[kind] = m.eval()
        return made[kind]
    return get


def gpu_run(models, case, kind):
    """One forward of the model with the encoder stages captured the way tests/test_gpu_model.py takes them
    (wrapping _pcd_align / _bilstm_steps for the call), the 4x outputs, the latent and one odd-sized decode."""
    if (case, kind) in _GPU:
        return _GPU[case, kind]
    model = models(kind)
    x = torch.from_numpy(frames(case)).cuda()
    cap = {}
    orig_bilstm, orig_pcd = model._bilstm_steps, model._pcd_align

    def bilstm(X, *a, **k):                             # a stage generator (LunaTokis._run_lanes)
        cap["fusion"] = X[1].detach().clone()           # fusion output = latent step 1 input
        out = yield from orig_bilstm(X, *a, **k)
        cap["bilstm"] = out.detach().clone()
        return out

    def pcd(units, **kw):
        orig_pcd(units, **kw)
        if units[0][0] == "pcd_align.":                 # the frame pair's alignment, not the BiConvLSTM's Easy_PCD
            cap["pcd"] = [u[4].detach().clone() for u in units]
    model._bilstm_steps, model._pcd_align = bilstm, pcd
    try:
        with torch.no_grad():
            outs = [o.clone() for o in model(x, TIMES)]
    finally:
        del model._bilstm_steps, model._pcd_align
    with torch.no_grad():
        feat = model.feat.detach().clone()
        scaled = model.decoding([T1], scale=grid_of(case))[0].clone()
    torch.cuda.synchronize()
    nchw = lambda t: t.permute(0, 3, 1, 2)
    stages = {"pcd_align": torch.cat([nchw(cap["pcd"][0]), nchw(cap["pcd"][1])], 1),      # cat(y1, y2) (:130)
              "fusion": nchw(cap["fusion"]),
              "bilstm": cap["bilstm"].permute(1, 0, 4, 2, 3),                            # [3, B, H, W, 64] -> [B, 3, 64, H, W]
              "feat": feat}
    _GPU[case, kind] = dict(x=x, stages=stages, outs=outs, scaled=scaled)
    return _GPU[case, kind]


@pytest.mark.parametrize("run", RUNS, ids=run_id)
def test_encoder_stages_match_oracle(models, sd, run):
    """PCD_Align output, fusion, the BiConvLSTM latents and the final latent, every element of every item."""
    case, kind = run
    ref, got = oracle(case, sd), gpu_run(models, case, kind)
    bad = []
    for name in ("pcd_align", "fusion", "bilstm", "feat"):
        ok, err, worst = close(got["stages"][name], ref["cap"][name])
        print(f"small frames: {run_id(run)} {name:<9} max |gpu - ref| = {err:.3e}, worst ratio to the bound = {worst:.4f}")
        if not ok:
            bad.append((name, err, worst))
    assert not bad, (run_id(run), bad)


@pytest.mark.parametrize("run", RUNS, ids=run_id)
def test_outputs_match_oracle(models, sd, run):
    """model(x, times) at the default 4x size against O.forward, and decoding at (2H + 1, 3W - 1) against the
    oracle's decode of its own latent."""
    case, kind = run
    B, H, W = case
    ref, got = oracle(case, sd), gpu_run(models, case, kind)
    bad = []
    assert len(got["outs"]) == len(TIMES)
    for t, o, r in zip(TIMES, got["outs"], ref["outs"]):
        assert tuple(o.shape) == (B, 3, 4 * H, 4 * W)
        ok, err, worst = close(o, r)
        print(f"small frames: {run_id(run)} out t={t:.2f} max |gpu - ref| = {err:.3e}, worst ratio to the bound = {worst:.4f}")
        if not ok:
            bad.append((t, err, worst))
    assert tuple(got["scaled"].shape) == (B, 3, *grid_of(case))
    ok, err, worst = close(got["scaled"], ref["scaled"])
    print(f"small frames: {run_id(run)} out {grid_of(case)} t={T1:.2f} max |gpu - ref| = {err:.3e}, "
          f"worst ratio to the bound = {worst:.4f}")
    if not ok:
        bad.append((grid_of(case), err, worst))
    assert not bad, (run_id(run), bad)


@pytest.mark.parametrize("run", RUNS_B2, ids=run_id)
def test_batch_item_is_bit_identical_alone(models, run):
    """Item 1 of a batch of two different pairs, run alone: the same bits (the launches of the batch and of the
    single pair differ in item counts, grids and tile placement, never in a pixel's arithmetic)."""
    case, kind = run
    got = gpu_run(models, case, kind)
    with torch.no_grad():
        one = models(kind)(got["x"][1:2], TIMES)
    for t, o, b in zip(TIMES, one, got["outs"]):
        assert torch.equal(o, b[1:2]), (run_id(run), t, float((o - b[1:2]).abs().max()))


@pytest.mark.parametrize("kind", ["f16x3", "f32"])
def test_local_ensemble_4x8(models, sd, kind):
    """decoding(ensemble=True) of the batch of two 4 x 8 pairs against O.decoding_localensemble of each item of the
    oracle's own latent (four shifted decodes of a 4 x 8 latent and the area blend)."""
    case = (2, 4, 8)
    ref = oracle(case, sd)
    model = models(kind)
    with torch.no_grad():
        model.gen_feat(torch.from_numpy(ref["x"]).cuda())
        got = model.decoding([T1], ensemble=True)[0]
    assert tuple(got.shape) == (2, 3, 16, 32)
    bad = []
    for b in range(2):
        r = O.decoding_localensemble(ref["cap"]["feat"][b:b + 1], ref["x"][b:b + 1], [T1], sd)
        ok, err, worst = close(got[b:b + 1], r)
        print(f"small frames: 2x4x8-{kind} ensemble item {b} max |gpu - ref| = {err:.3e}, worst ratio to the bound = {worst:.4f}")
        if not ok:
            bad.append((b, err, worst))
    assert not bad, bad


@pytest.mark.parametrize("kind", ["f16x3", "f32"])
def test_decoding_test_4x4(models, sd, kind):
    """decoding_test at scale 4 of the 4 x 4 pair against O.decoding_test: the HR-image path (stif_upsample_image
    of a 4 x 4 frame pair, the projection without the LR image) and its tables at a 4 x 4 latent."""
    case = (1, 4, 4)
    ref = oracle(case, sd)
    model = models(kind)
    with torch.no_grad():
        model.gen_feat(torch.from_numpy(ref["x"]).cuda())
        got = model.decoding_test([T1], 4)[0]
    assert tuple(got.shape) == (1, 3, 16, 16)
    ok, err, worst = close(got, O.decoding_test(ref["cap"]["feat"], ref["x"], [T1], sd, 4)[0])
    print(f"small frames: 1x4x4-{kind} decoding_test max |gpu - ref| = {err:.3e}, worst ratio to the bound = {worst:.4f}")
    assert ok, (err, worst)
