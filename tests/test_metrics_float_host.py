"""Host side of the float-protocol metric (stif_metric_float: calc_psnr beside ssim_matlab / myutils.ssim), no
GPU: the numpy restatement against tests/golden/metrics_float.npz -- whose reference values come from the
reference's own calc_psnr / ssim_matlab / ssim (tests/golden/make_metrics_float_golden.py) -- the 3 x 3 channel mix
against direct 3-D padding, workspace sizing and argument validation (every check comes before the first launch,
so it runs here).  The GPU tests import the restatement from this file."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from test_metrics_host import gold, gt_as_float, load_case, rel_tol, window11, within  # noqa: F401

GOLD_FLOAT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "metrics_float.npz")
CASES = ["11x11", "12x37", "45x70", "32x64", "33x65"]
COL_PSNR, COL_SSIM = 0, {True: 1, False: 2}      # columns of ref / exact / diff: calc_psnr, ssim_volume, ssim_planar
F32 = np.float32
FAKE = 0x10000     # a non-null address no valid path may touch: every invalid case fails validation first


@pytest.fixture(scope="module")
def gold_float():
    with np.load(GOLD_FLOAT) as z:
        return {k: z[k] for k in z.files}


def load_float_case(gold, gold_float, name):
    """(pred [n,3,H,W] fp32, ref [n,3,H,W] fp32 = gt RGB / 255, ref values, exact, diff [n,3])"""
    if f"{name}__pred" in gold_float:
        pred, gt = gold_float[f"{name}__pred"], gold_float[f"{name}__gt"]
    else:
        pred, gt = load_case(gold, name)[:2]
    fref = np.stack([gt_as_float(g) for g in gt])
    return pred, fref, gold_float[f"{name}__ref"], gold_float[f"{name}__exact"], gold_float[f"{name}__diff"]


# ------------------------------------------------------------------ numpy restatement (float64, fp64 window)
def channel_mix(k):
    """M[d][c]: the weight of input channel c in output channel d of the depth pass (3 channels, radius 5,
    replicate padding): tap j of output d reads channel clamp(d - 5 + j, 0, 2)"""
    return np.array([[k[:6 - d].sum(), k[6 - d], k[7 - d:].sum()] for d in range(3)])


def filt(v, k, volume, via_mix=False):
    """v [3, H, W] float64 -> the 11-tap Gaussian over (channel,) row, column with replicate padding of 5"""
    _, H, W = v.shape
    if volume and via_mix:
        v, volume = np.einsum("dc,chw->dhw", channel_mix(k), v), False
    v = np.pad(v, ((5, 5) if volume else (0, 0), (5, 5), (5, 5)), mode="edge")
    if volume:
        v = sum(k[j] * v[j:j + 3] for j in range(11))
    v = sum(k[j] * v[:, j:j + H] for j in range(11))
    return sum(k[j] * v[:, :, j:j + W] for j in range(11))


def float_sums(pred, ref, volume=True, via_mix=False):
    """pred, ref [3, H, W] fp32 -> (sse, npix, ssim_sum, nwin) as stif_metric_float defines them"""
    k = window11()
    d = pred.astype(np.float64) - ref.astype(np.float64)
    a, b = np.clip(pred, 0, 1).astype(np.float64), np.clip(ref, 0, 1).astype(np.float64)
    mu1, mu2 = filt(a, k, volume, via_mix), filt(b, k, volume, via_mix)
    s1 = filt(a * a, k, volume, via_mix) - mu1 * mu1
    s2 = filt(b * b, k, volume, via_mix) - mu2 * mu2
    s12 = filt(a * b, k, volume, via_mix) - mu1 * mu2
    C1, C2 = 1e-4, 9e-4
    m = ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))
    return float((d * d).sum()), d.size, float(m.sum()), m.size


def restate_eval(pred, ref, volume=True, via_mix=False):
    """(calc_psnr, ssim) of one item"""
    sse, npix, ssum, nwin = float_sums(pred, ref, volume, via_mix)
    return -10.0 * math.log10(sse / npix + 1e-8), ssum / nwin


# ------------------------------------------------------------------ restatement against the fixture
@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_exact_values(gold, gold_float, name):
    pred, fref, _, exact, _ = load_float_case(gold, gold_float, name)
    for i in range(pred.shape[0]):
        for volume, cs in COL_SSIM.items():
            p, s = restate_eval(pred[i], fref[i], volume)
            assert within(p, exact[i, COL_PSNR], rel_tol(exact[i, COL_PSNR], 1e-12)), (name, i, p)
            assert within(s, exact[i, cs], rel_tol(exact[i, cs], 1e-12)), (name, i, volume, s, exact[i, cs])


@pytest.mark.parametrize("name", CASES)
def test_restatement_within_recorded_difference_of_reference(gold, gold_float, name):
    """The recorded difference is |reference - exact|: the reference's fp32 window and fp32 convolutions (and
    calc_psnr's fp32 mean); the generator bounds it by 5e-5 for the SSIM columns."""
    pred, fref, ref, _, diff = load_float_case(gold, gold_float, name)
    assert diff[:, 1:].max() < 5e-5
    for i in range(pred.shape[0]):
        for volume, cs in COL_SSIM.items():
            p, s = restate_eval(pred[i], fref[i], volume)
            assert within(p, ref[i, COL_PSNR], diff[i, COL_PSNR] + rel_tol(ref[i, COL_PSNR], 1e-12))
            assert within(s, ref[i, cs], diff[i, cs] + 1e-12), (name, i, volume, s, ref[i, cs])


def test_fixture_content(gold, gold_float):
    """what the cases are for: out-of-range values in every input, one item equal to its ground truth (SSIM
    exactly 1 in both modes, PSNR 80 dB from the 1e-8), the two modes really differ, 33x65 is two items"""
    assert list(gold_float["columns"]) == ["calc_psnr", "ssim_volume", "ssim_planar"]
    for name in CASES:
        pred = load_float_case(gold, gold_float, name)[0]
        assert pred.min() == F32(-0.25) and pred.max() == F32(1.25), name
    _, _, ref, exact, _ = load_float_case(gold, gold_float, "45x70")
    assert exact[1, 1] == 1.0 and exact[1, 2] == 1.0 and ref[1, 1] == 1.0 and ref[1, 2] == 1.0
    assert exact[1, 0] == pytest.approx(80.0, rel=1e-12)
    others = np.delete(exact, 1, 0)
    assert (others[:, 1:] > 0.05).all() and (others[:, 1:] < 0.98).all()
    assert (np.abs(others[:, 1] - others[:, 2]) > 1e-3).all()
    assert gold_float["33x65__pred"].shape == (2, 3, 33, 65)


@pytest.mark.parametrize("name", CASES)
def test_channel_mix_equals_direct_depth_padding(gold, gold_float, name):
    """the depth pass over three replicated channels is the 3 x 3 mix of channel_mix, field by field"""
    k = window11()
    M = channel_mix(k)
    assert np.abs(M.sum(1) - 1).max() < 1e-15 and (M[0] == M[2][::-1]).all() and M[1, 0] == M[1, 2]
    pred, fref = load_float_case(gold, gold_float, name)[:2]
    for i in range(pred.shape[0]):
        direct, mixed = float_sums(pred[i], fref[i], True), float_sums(pred[i], fref[i], True, via_mix=True)
        assert direct[:2] == mixed[:2] and direct[3] == mixed[3] == 3 * pred.shape[2] * pred.shape[3]
        assert abs(mixed[2] - direct[2]) <= 1e-12 * abs(direct[2]), (name, i, direct[2], mixed[2])


# ------------------------------------------------------------------ workspace
def test_workspace_size(stif):
    L = stif._lib
    ws = L.lib().stif_metric_float_workspace_size
    for mode in (L.FSSIM_VOLUME, L.FSSIM_PLANAR):
        base = ws(1, 45, 70, mode)
        assert base > 0 and base % 8 == 0
        assert ws(1, 11, 11, mode) > 0
        assert [ws(n, 45, 70, mode) for n in (2, 3, 8)] == [2 * base, 3 * base, 8 * base]
        assert ws(1, 45 + 32, 70, mode) > base and ws(1, 45, 70 + 32, mode) > base
    for bad in [(0, 45, 70, 0), (-1, 45, 70, 0), (1, 0, 70, 0), (1, 45, 0, 0), (1, -5, 70, 0), (1, 10, 70, 0),
                (1, 45, 10, 0), (1, 10, 23, 1), (1, 45, 70, 2), (1, 45, 70, -1)]:
        assert ws(*bad) == 0, bad


# ------------------------------------------------------------------ validation (before any launch)
def _args(L, **kw):
    a = L.MetricArgs()
    a.pred, a.gt_f32, a.n, a.H, a.W, a.flags = FAKE, FAKE, 2, 45, 70, L.METRIC_FLOAT
    for k, v in kw.items():
        setattr(a, k, v)
    return a


INVALID = {
    "null_pred": dict(pred=None),
    "null_gt_f32": dict(gt_f32=None),
    "gt_u8_is_not_a_reference": dict(gt_f32=None, gt_u8=FAKE),
    "n0": dict(n=0),
    "H10": dict(H=10),
    "W10": dict(W=10),
    "H0": dict(H=0),
    "W_negative": dict(W=-3),
    "flag_y": dict(flags=1),
    "flag_ssim": dict(flags=2),
    "flag_float_with_ssim": dict(flags=4 | 2),
    "unknown_flag": dict(flags=8),
    "pred_pitch_below_W": dict(pred_item=3 * 48 * 72, pred_plane=48 * 72, pred_pitch=69),
    "pred_planes_overlap": dict(pred_item=3 * 48 * 72, pred_plane=44 * 72, pred_pitch=72),
    "pred_items_overlap": dict(pred_item=2 * 48 * 72, pred_plane=48 * 72, pred_pitch=72),
    "ref_pitch_below_W": dict(gtf_item=3 * 45 * 70, gtf_plane=45 * 70, gtf_pitch=60),
    "ref_planes_overlap": dict(gtf_item=3 * 48 * 72, gtf_plane=44 * 72, gtf_pitch=72),
    "ref_items_overlap": dict(gtf_item=2 * 48 * 72, gtf_plane=48 * 72, gtf_pitch=72),
}


@pytest.mark.parametrize("case", sorted(INVALID))
def test_invalid_arguments_are_rejected_before_any_launch(stif, case):
    L = stif._lib
    lib = L.lib()
    a = _args(L, **INVALID[case])
    rc = lib.stif_metric_float(C.byref(a), L.FSSIM_VOLUME, FAKE, FAKE, 1 << 30, None)
    # a launch attempt would have come back as STIF_E_LAUNCH here (no device) or touched FAKE
    assert rc == L.E_INVALID, (case, rc)
    msg = lib.stif_last_error().decode()
    assert msg.startswith("stif_metric_float:") and len(msg) > 30, msg


def test_mode_struct_out_workspace_and_alignment(stif):
    L = stif._lib
    lib = L.lib()
    a = _args(L)
    call = lib.stif_metric_float
    for mode in (2, -1):
        assert call(C.byref(a), mode, FAKE, FAKE, 1 << 30, None) == L.E_INVALID
        assert lib.stif_last_error().decode().startswith("stif_metric_float:")
    assert call(None, 0, FAKE, FAKE, 1 << 30, None) == L.E_INVALID
    assert call(C.byref(a), 0, None, FAKE, 1 << 30, None) == L.E_INVALID
    for mode in (L.FSSIM_VOLUME, L.FSSIM_PLANAR):
        need = lib.stif_metric_float_workspace_size(a.n, a.H, a.W, mode)
        # the header's own code for a short or missing workspace
        assert call(C.byref(a), mode, FAKE, FAKE, need - 1, None) == L.E_WORKSPACE
        msg = lib.stif_last_error().decode()
        assert msg.startswith("stif_metric_float:") and "workspace" in msg
        assert call(C.byref(a), mode, FAKE, None, need, None) == L.E_WORKSPACE
        assert call(C.byref(a), mode, FAKE + 4, FAKE, need, None) == L.E_INVALID       # misaligned out
        assert "aligned" in lib.stif_last_error().decode()
        assert call(C.byref(a), mode, FAKE, FAKE + 4, need + 8, None) == L.E_INVALID   # misaligned workspace
        assert lib.stif_last_error().decode().startswith("stif_metric_float:")


# ------------------------------------------------------------------ Python entry points
def test_eval_metrics_rejects_bad_inputs(stif):
    torch = pytest.importorskip("torch")
    M = stif.metrics
    assert M.sums_float and M.ssim_float
    p = torch.zeros(2, 3, 12, 23)
    with pytest.raises(ValueError, match="does not match"):
        M.eval_metrics(p, torch.zeros(2, 3, 12, 24))
    with pytest.raises(ValueError, match="does not match"):
        M.eval_metrics(p, torch.zeros(1, 3, 12, 23))
    with pytest.raises(ValueError, match=r"\[n, 3, H, W\]"):
        M.eval_metrics(torch.zeros(2, 1, 12, 23), torch.zeros(2, 1, 12, 23))
    t = torch.zeros(2, 3, 23, 12).permute(0, 1, 3, 2)
    assert tuple(t.shape) == tuple(p.shape) and t.stride(-1) != 1
    with pytest.raises(ValueError, match="contiguous"):
        M.eval_metrics(t, p)
    with pytest.raises(ValueError, match="contiguous"):
        M.eval_metrics(p, t)
    small = torch.zeros(1, 3, 10, 23)
    for volume in (True, False):
        with pytest.raises(ValueError, match="smaller than the 11 x 11 window"):
            M.eval_metrics(small, small, volume)
    with pytest.raises(ValueError, match="smaller than the 11 x 11 window"):
        M.ssim_float(small.permute(0, 1, 3, 2).contiguous(), small.permute(0, 1, 3, 2).contiguous())
