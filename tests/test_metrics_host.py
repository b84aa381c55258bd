"""Host side of the on-device PSNR / SSIM metric (no GPU): the window table, workspace sizing, argument
validation (every check comes before the first launch, so it runs here), the host arithmetic of
``metrics.finish``, and the numpy restatement of the metric against tests/golden/metrics.npz -- whose reference
values come from the reference's own tensor2img / bgr2ycbcr / calculate_psnr / ssim / calc_psnr
(tests/golden/make_metrics_golden.py).  The GPU tests import the restatement from this file."""
import ctypes as C
import math
import os

import numpy as np
import pytest

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "metrics.npz")
CASES = ["11x11", "10x23", "12x37", "45x70", "32x64"]
COLS = {"y": (0, 1), "rgb": (2, 3)}      # columns of ref / exact / diff: psnr_y, ssim_y, psnr_rgb, ssim_rgb, calc_psnr
F32 = np.float32


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLD) as z:
        return {k: z[k] for k in z.files}


def gt_as_float(gt):
    """calc_psnr's float ground truth: the RGB planes of gt / 255 in fp32"""
    return np.ascontiguousarray(gt[..., ::-1].transpose(2, 0, 1)).astype(F32) / F32(255.0)


def load_case(gold, name):
    """(pred [n,3,H,W] fp32, gt [n,H,W,3] uint8 BGR, ref, exact, diff [n,5]); the item that equals its ground
    truth is stored as zeros and rebuilt here."""
    pred = gold[f"{name}__pred"].copy()
    gt = gold[f"{name}__gt"]
    eq = int(gold[f"{name}__eq_item"])
    if eq >= 0:
        pred[eq] = gt_as_float(gt[eq])
    return pred, gt, gold[f"{name}__ref"], gold[f"{name}__exact"], gold[f"{name}__diff"]


# ------------------------------------------------------------------ numpy restatement (exact-integer GT, float64)
def window11():
    x = np.arange(11, dtype=np.float64) - 5.0
    k = np.exp(-(x * x) / 4.5)
    return k * (1.0 / k.sum())


def quantise(pred):
    return np.rint(np.clip(pred.astype(F32), F32(0), F32(1)) * F32(255.0)).astype(np.float64)


def luma(b, g, r):
    return (24.966 * b + 128.553 * g + 65.481 * r) / 255.0 + 16.0


def plane_sums(a, b, k):
    H, W = a.shape
    sse, npix = float(((a - b) ** 2).sum()), H * W
    if H < 11 or W < 11:
        return sse, npix, 0.0, 0

    def filt(img):
        h = sum(k[j] * img[:, j:W - 10 + j] for j in range(11))
        return sum(k[j] * h[j:H - 10 + j, :] for j in range(11))

    C1, C2 = 6.5025, 58.5225
    mu1, mu2 = filt(a), filt(b)
    s1, s2, s12 = filt(a * a) - mu1 * mu1, filt(b * b) - mu2 * mu2, filt(a * b) - mu1 * mu2
    m = ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))
    return sse, npix, float(m.sum()), m.size


def exact_sums(pred, gt, channels):
    """pred [3,H,W] fp32 RGB, gt [H,W,3] uint8 BGR -> (sse, npix, ssim_sum, nwin)"""
    k = window11()
    q = quantise(pred)
    g = gt.astype(np.float64)
    if channels == "y":
        return plane_sums(luma(q[2], q[1], q[0]), luma(g[..., 0], g[..., 1], g[..., 2]), k)
    parts = [plane_sums(q[c], g[..., 2 - c], k) for c in range(3)]
    return tuple(sum(p[i] for p in parts) for i in range(4))


def restate(pred, gt, channels):
    """(psnr, ssim) of one item"""
    sse, npix, ssum, nwin = exact_sums(pred, gt, channels)
    mse = sse / npix
    return (math.inf if mse == 0 else 20.0 * math.log10(255.0 / math.sqrt(mse))), (ssum / nwin if nwin else math.nan)


def restate_float(pred, ref):
    d = pred.astype(np.float64) - ref.astype(np.float64)
    return -10.0 * math.log10(float((d * d).mean()) + 1e-8)


def within(got, want, tol):
    """|got - want| <= tol, with NaN matching NaN and an infinity matching only itself (tol = inf: anything)"""
    if math.isnan(want):
        return math.isnan(got)
    if math.isinf(tol):
        return not math.isnan(got)
    if math.isinf(want) or math.isinf(got):
        return got == want
    return abs(got - want) <= tol


def rel_tol(want, rel):
    """a relative tolerance; an infinite expected value must be matched exactly"""
    return rel * abs(want) if math.isfinite(want) else 0.0


# ------------------------------------------------------------------ window, workspace
def test_window_matches_fixture(stif, gold):
    k = stif.metrics.window()
    assert k.shape == (11,) and k.dtype == np.float64
    assert np.abs(k - gold["window"]).max() <= 1e-15
    assert abs(k.sum() - 1) < 1e-15 and np.all(k == k[::-1])


def test_workspace_size_grows(stif):
    L = stif._lib
    ws = L.lib().stif_metric_workspace_size
    Y = L.METRIC_Y | L.METRIC_SSIM
    base = ws(1, 45, 70, Y)
    assert base > 0 and base % 8 == 0
    assert ws(3, 45, 70, Y) > base
    assert ws(1, 45 + 32, 70, Y) > base and ws(1, 45, 70 + 32, Y) > base
    assert ws(1, 45, 70, L.METRIC_SSIM) > base           # three planes in RGB mode
    assert ws(1, 45, 70, L.METRIC_FLOAT) > 0
    for bad in [(0, 45, 70, Y), (1, 0, 70, Y), (1, 45, 0, Y), (1, 45, 70, L.METRIC_FLOAT | L.METRIC_Y),
                (1, 45, 70, L.METRIC_FLOAT | L.METRIC_SSIM), (1, 45, 70, 8)]:
        assert ws(*bad) == 0, bad


# ------------------------------------------------------------------ validation (before any launch)
FAKE = 0x10000     # a non-null address no valid path may touch: every case below fails validation first


def _args(L, **kw):
    a = L.MetricArgs()
    a.pred, a.gt_u8, a.n, a.H, a.W, a.flags = FAKE, FAKE, 2, 45, 70, L.METRIC_Y | L.METRIC_SSIM
    for k, v in kw.items():
        setattr(a, k, v)
    return a


INVALID = {
    "null_pred": dict(pred=None),
    "null_gt": dict(gt_u8=None),
    "n0": dict(n=0),
    "H0": dict(H=0),
    "W_negative": dict(W=-3),
    "pred_pitch_below_W": dict(pred_item=3 * 48 * 72, pred_plane=48 * 72, pred_pitch=69),
    "pred_planes_overlap": dict(pred_item=3 * 48 * 72, pred_plane=44 * 72, pred_pitch=72),
    "pred_items_overlap": dict(pred_item=2 * 48 * 72, pred_plane=48 * 72, pred_pitch=72),
    "gt_pitch_below_3W": dict(gt_item=45 * 209, gt_pitch=209),
    "gt_items_overlap": dict(gt_item=44 * 216, gt_pitch=216),
    "unknown_flag": dict(flags=8),
    "float_with_ssim": dict(flags=4 | 2, gt_f32=FAKE),
    "float_with_y": dict(flags=4 | 1, gt_f32=FAKE),
    "float_without_gt_f32": dict(flags=4),
    "float_gt_pitch_below_W": dict(flags=4, gt_f32=FAKE, gtf_item=3 * 45 * 70, gtf_plane=45 * 70, gtf_pitch=60),
}


@pytest.mark.parametrize("case", sorted(INVALID))
def test_invalid_arguments_are_rejected_before_any_launch(stif, case):
    L = stif._lib
    lib = L.lib()
    a = _args(L, **INVALID[case])
    rc = lib.stif_metric_psnr_ssim(C.byref(a), FAKE, FAKE, 1 << 30, None)
    # a launch attempt would have come back as STIF_E_LAUNCH here (no device) or touched FAKE
    assert rc == L.E_INVALID, (case, rc)
    msg = lib.stif_last_error().decode()
    assert msg.startswith("stif_metric_psnr_ssim:") and len(msg) > 30, msg


def test_null_struct_out_and_workspace(stif):
    L = stif._lib
    lib = L.lib()
    a = _args(L)
    assert lib.stif_metric_psnr_ssim(None, FAKE, FAKE, 1 << 30, None) == L.E_INVALID
    assert lib.stif_metric_psnr_ssim(C.byref(a), None, FAKE, 1 << 30, None) == L.E_INVALID
    need = lib.stif_metric_workspace_size(a.n, a.H, a.W, a.flags)
    # the header's own code for a short or missing workspace
    assert lib.stif_metric_psnr_ssim(C.byref(a), FAKE, FAKE, need - 1, None) == L.E_WORKSPACE
    assert "workspace" in lib.stif_last_error().decode()
    assert lib.stif_metric_psnr_ssim(C.byref(a), FAKE, None, need, None) == L.E_WORKSPACE
    with pytest.raises(stif._lib.StifError):
        L.check(lib.stif_metric_window(None), "stif_metric_window")


# ------------------------------------------------------------------ host arithmetic
def test_finish(stif):
    fin = stif.metrics.finish
    out4 = np.array([[450.0, 200.0, 30.0, 40.0],      # ordinary
                     [0.0, 200.0, 40.0, 40.0],        # identical images: inf, exactly 1
                     [450.0, 200.0, 0.0, 0.0]])       # no window fits: NaN
    psnr, ssim = fin(out4)
    assert psnr.dtype == np.float64 and ssim.dtype == np.float64 and psnr.shape == (3,)
    assert psnr[0] == pytest.approx(20 * math.log10(255 / math.sqrt(2.25)), rel=1e-15)
    assert ssim[0] == 0.75
    assert psnr[1] == np.inf and ssim[1] == 1.0
    assert psnr[2] == psnr[0] and np.isnan(ssim[2])
    pf, sf = fin(np.array([[0.02, 200.0, 0.0, 0.0], [0.0, 200.0, 0.0, 0.0]]), float_mode=True)
    assert pf[0] == pytest.approx(-10 * math.log10(1e-4 + 1e-8), rel=1e-15)
    assert pf[1] == pytest.approx(80.0, rel=1e-15)     # the +1e-8 keeps it finite
    assert np.isnan(sf).all()
    assert fin(out4[0])[0].shape == (1,)               # a single row is accepted


def test_package_exposes_metrics(stif):
    assert stif.metrics.psnr_ssim and stif.metrics.psnr_float
    assert stif.metrics.mode_flags("y", True) == 3 and stif.metrics.mode_flags("rgb", False) == 0
    with pytest.raises(ValueError):
        stif.metrics.mode_flags("yuv")


# ------------------------------------------------------------------ restatement against the fixture
@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_exact_values(gold, name):
    pred, gt, _, exact, _ = load_case(gold, name)
    for i in range(pred.shape[0]):
        for ch, (cp, cs) in COLS.items():
            p, s = restate(pred[i], gt[i], ch)
            assert within(p, exact[i, cp], rel_tol(exact[i, cp], 1e-12)), (name, i, ch, p, exact[i, cp])
            assert within(s, exact[i, cs], rel_tol(exact[i, cs], 1e-12)), (name, i, ch, s, exact[i, cs])
        f = restate_float(pred[i], gt_as_float(gt[i]))
        assert within(f, exact[i, 4], rel_tol(exact[i, 4], 1e-12))


@pytest.mark.parametrize("name", CASES)
def test_restatement_within_recorded_difference_of_reference(gold, name):
    """The recorded difference is |reference - exact|: the fp32 noise of the reference's GT (and of calc_psnr's
    fp32 mean).  It is inf for the Y PSNR of the item that equals its GT: the reference's noise makes that
    ~150 dB where the exact integers give inf."""
    pred, gt, ref, _, diff = load_case(gold, name)
    assert np.nanmax(np.where(np.isinf(diff), 0, diff)) < 1e-5
    for i in range(pred.shape[0]):
        for ch, (cp, cs) in COLS.items():
            p, s = restate(pred[i], gt[i], ch)
            assert within(p, ref[i, cp], diff[i, cp] + rel_tol(ref[i, cp], 1e-12)), (name, i, ch, p, ref[i, cp])
            assert within(s, ref[i, cs], diff[i, cs] + 1e-12), (name, i, ch, s, ref[i, cs])
        f = restate_float(pred[i], gt_as_float(gt[i]))
        assert within(f, ref[i, 4], diff[i, 4] + rel_tol(ref[i, 4], 1e-12))


def test_fixture_content(gold):
    """what the cases are for: out-of-range values, exact rounding ties of both parities, one item equal to its
    ground truth, no window at 10x23, one window at 11x11"""
    pred, gt, ref, exact, _ = load_case(gold, "45x70")
    assert pred.min() < 0 and pred.max() > 1
    p255 = (pred.astype(F32) * F32(255.0)).astype(np.float64)
    ties = p255[(p255 % 1.0 == 0.5) & (p255 > 0) & (p255 < 255)]
    assert (np.floor(ties) % 2 == 0).any() and (np.floor(ties) % 2 == 1).any()
    assert exact[1, 0] == np.inf and exact[1, 1] == 1.0 and exact[1, 2] == np.inf and exact[1, 3] == 1.0
    others = np.delete(exact, 1, 0)
    assert np.isfinite(others).all() and (others[:, [1, 3]] > 0.05).all() and (others[:, [1, 3]] < 0.98).all()
    assert np.isnan(load_case(gold, "10x23")[3][0, [1, 3]]).all()
    assert exact_sums(*[a[0] for a in load_case(gold, "11x11")[:2]], "y")[3] == 1
