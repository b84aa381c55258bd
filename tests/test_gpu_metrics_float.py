"""The float-protocol metric on the device (k_metric_float in csrc/metrics.hip through stif_metric_float,
stif_amd.metrics.eval_metrics and video.evaluate_sequence(metric="float")) against tests/golden/metrics_float.npz.

Tolerances, as for the quantised metric (test_gpu_metrics.py).  Against the fp64 restatement: 1e-9 relative --
float64 sums of at most 2^14 terms per item (3 x 45 x 70), reordered, give N * 2^-53 ~ 2e-12, and the per-pixel
filter and division chain is a few hundred float64 operations on values of order 1.  Against the reference's own
functions: twice the difference the fixture records for that item and column (the reference's fp32 window and
fp32 convolutions; one sample, not a bound) plus 1e-9."""
import ctypes as C
import math

import numpy as np
import pytest

from test_metrics_float_host import (CASES, COL_PSNR, COL_SSIM, float_sums, gold_float, load_float_case,  # noqa: F401
                                     restate_eval)
from test_metrics_host import gold, gt_as_float, load_case, rel_tol, within  # noqa: F401

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
REL = 1e-9
F32 = np.float32


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


@pytest.fixture(scope="module")
def scored(stif, gold, gold_float):
    """every fixture case in both modes, computed once: {(name, volume): (psnr [n], ssim [n], sums [n, 4])}"""
    res = {}
    for name in CASES:
        pred, fref = load_float_case(gold, gold_float, name)[:2]
        for volume in COL_SSIM:
            out = stif.metrics.sums_float(_dev(pred), _dev(fref), volume).cpu().numpy()
            res[name, volume] = stif.metrics.finish(out, float_mode=True) + (out,)
    return res


@pytest.mark.parametrize("volume", [True, False])
@pytest.mark.parametrize("name", CASES)
def test_matches_fp64_restatement(scored, gold, gold_float, name, volume):
    exact = load_float_case(gold, gold_float, name)[3]
    psnr, ssim, _ = scored[name, volume]
    cs = COL_SSIM[volume]
    assert psnr.dtype == np.float64 and psnr.shape == (exact.shape[0],) and ssim.shape == psnr.shape
    for i in range(exact.shape[0]):
        print(name, volume, i, "psnr", psnr[i], exact[i, COL_PSNR], "ssim", ssim[i], exact[i, cs])
        assert within(psnr[i], exact[i, COL_PSNR], rel_tol(exact[i, COL_PSNR], REL)), (i, psnr[i], exact[i, COL_PSNR])
        assert within(ssim[i], exact[i, cs], rel_tol(exact[i, cs], REL)), (i, ssim[i], exact[i, cs])


@pytest.mark.parametrize("volume", [True, False])
@pytest.mark.parametrize("name", CASES)
def test_matches_reference_functions(scored, gold, gold_float, name, volume):
    _, _, ref, _, diff = load_float_case(gold, gold_float, name)
    psnr, ssim, _ = scored[name, volume]
    cs = COL_SSIM[volume]
    for i in range(ref.shape[0]):
        print(name, volume, i, "psnr", psnr[i], ref[i, COL_PSNR], "ssim", ssim[i], ref[i, cs], diff[i])
        assert within(psnr[i], ref[i, COL_PSNR], 2 * diff[i, COL_PSNR] + 1e-9), (i, psnr[i], ref[i, COL_PSNR])
        assert within(ssim[i], ref[i, cs], 2 * diff[i, cs] + 1e-9), (i, ssim[i], ref[i, cs], diff[i, cs])


def test_identical_item_and_counts(scored, gold, gold_float):
    for volume in COL_SSIM:
        psnr, ssim, _ = scored["45x70", volume]
        assert abs(ssim[1] - 1.0) <= REL
        want = -10.0 * math.log10(1e-8)
        assert abs(psnr[1] - want) <= REL * want
    for (name, volume), (_, _, out) in scored.items():
        H, W = load_float_case(gold, gold_float, name)[0].shape[2:]
        assert (out[:, 1] == 3 * H * W).all() and (out[:, 3] == 3 * H * W).all(), (name, volume, out)


def test_wrappers_agree(stif, gold, gold_float, scored):
    pred, fref = load_float_case(gold, gold_float, "33x65")[:2]
    for volume in COL_SSIM:
        p, s = stif.metrics.eval_metrics(_dev(pred), _dev(fref), volume)
        assert np.array_equal(p, scored["33x65", volume][0]) and np.array_equal(s, scored["33x65", volume][1])
        assert np.array_equal(stif.metrics.ssim_float(_dev(pred), _dev(fref), volume), s)
    # the PSNR half is the existing float mode's
    assert np.allclose(stif.metrics.psnr_float(_dev(pred), _dev(fref)), scored["33x65", True][0], rtol=REL, atol=0)
    # a [3, H, W] pair is one item; a host reference is moved to the device
    p1, s1 = stif.metrics.eval_metrics(_dev(pred[1]), torch.from_numpy(fref[1]))
    assert p1[0] == scored["33x65", True][0][1] and s1[0] == scored["33x65", True][1][1]


@pytest.mark.parametrize("volume", [True, False])
def test_clamp_placement(stif, gold, gold_float, volume):
    """the SSIM sees clamp(x, 0, 1), the PSNR the raw floats: replacing the out-of-range values by 0 and 1 changes
    the sse column and leaves the ssim_sum column bit-identical"""
    M = stif.metrics
    pred, fref = load_float_case(gold, gold_float, "33x65")[:2]
    assert (pred == F32(-0.25)).any() and (pred == F32(1.25)).any()
    inside = np.clip(pred, F32(0), F32(1))
    a = M.sums_float(_dev(pred), _dev(fref), volume).cpu().numpy()
    b = M.sums_float(_dev(inside), _dev(fref), volume).cpu().numpy()
    assert (a[:, 0] != b[:, 0]).all()
    assert a[:, 2].tobytes() == b[:, 2].tobytes()
    # and the same on the reference's side
    c = M.sums_float(_dev(fref), _dev(pred), volume).cpu().numpy()
    d = M.sums_float(_dev(fref), _dev(inside), volume).cpu().numpy()
    assert (c[:, 0] != d[:, 0]).all() and c[:, 2].tobytes() == d[:, 2].tobytes()


@pytest.mark.parametrize("volume", [True, False])
def test_strided_view_equals_dense_bit_for_bit(stif, gold, gold_float, volume):
    """the 45x70 data in the top-left of 48x72 buffers whose padding holds values that would change every sum: as
    torch views (strides passed through) and through the C ABI with explicit strides.  The replicate padding
    clamps to the image rectangle: a halo clamped to the buffer would read the fill."""
    M, L = stif.metrics, stif._lib
    pred, fref = load_float_case(gold, gold_float, "45x70")[:2]
    dense = M.sums_float(_dev(pred), _dev(fref), volume).cpu().numpy()
    big = torch.full((3, 3, 48, 72), 0.37, device="cuda:0")
    gbig = torch.full((3, 3, 48, 72), 0.81, device="cuda:0")
    big[:, :, :45, :70] = _dev(pred)
    gbig[:, :, :45, :70] = _dev(fref)
    view, gview = big[:, :, :45, :70], gbig[:, :, :45, :70]
    assert not view.is_contiguous() and not gview.is_contiguous()
    assert M.sums_float(view, gview, volume).cpu().numpy().tobytes() == dense.tobytes()
    a = L.MetricArgs()
    a.pred, a.pred_item, a.pred_plane, a.pred_pitch = big.data_ptr(), 3 * 48 * 72, 48 * 72, 72
    a.gt_f32, a.gtf_item, a.gtf_plane, a.gtf_pitch = gbig.data_ptr(), 3 * 48 * 72, 48 * 72, 72
    a.n, a.H, a.W, a.flags = 3, 45, 70, 0
    mode = L.FSSIM_VOLUME if volume else L.FSSIM_PLANAR
    nbytes = L.lib().stif_metric_float_workspace_size(3, 45, 70, mode)
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device="cuda:0")
    out = torch.empty(3, 4, dtype=torch.float64, device="cuda:0")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    L.check(L.lib().stif_metric_float(C.byref(a), mode, out.data_ptr(), ws.data_ptr(), nbytes, st), "metric_float")
    assert out.cpu().numpy().tobytes() == dense.tobytes()


def test_two_calls_are_bit_identical(stif, gold, gold_float):
    M = stif.metrics
    pred, fref = load_float_case(gold, gold_float, "45x70")[:2]
    p, g = _dev(pred), _dev(fref)
    for volume in COL_SSIM:
        a = M.sums_float(p, g, volume).cpu().numpy()
        b = M.sums_float(p, g, volume).cpu().numpy()
        assert a.tobytes() == b.tobytes()


def test_small_images_raise(stif):
    small = torch.zeros(1, 3, 10, 23, device="cuda:0")
    with pytest.raises(ValueError, match="smaller than the 11 x 11 window"):
        stif.metrics.eval_metrics(small, small)
    with pytest.raises(ValueError, match="on the GPU"):
        stif.metrics.eval_metrics(torch.zeros(1, 3, 12, 12), torch.zeros(1, 3, 12, 12))


@pytest.fixture(scope="module")
def model(stif, sd):
    m = stif.LunaTokis(64, 6, 8, 5, 40)
    m.load_state_dict(sd)
    return m


def test_evaluate_sequence_float(stif, model):
    """the shapes of test_gpu_metrics.test_evaluate_sequence: 3 frames of 11x13 (48x64 outputs) at times 0 and 0.5
    against random 44x52 ground truth -- uint8 BGR, and one as float RGB planes -- one entry None; the top-left
    crop of every output is scored in place and must equal the restatement applied to run_sequence's outputs
    copied to the host.  metric="quantised" is the call without the argument."""
    rng = np.random.default_rng(7)
    frames = torch.from_numpy(rng.random((3, 3, 11, 13)).astype(np.float32)).to("cuda:0")
    times = [0.0, 0.5]
    outs = stif.video.run_sequence(model, frames, times)
    assert tuple(outs[0][0].shape) == (3, 48, 64)
    host = [[o.cpu().numpy().copy() for o in row] for row in outs]
    gt = [[rng.integers(0, 256, (44, 52, 3), dtype=np.uint8) for _ in times] for _ in range(2)]
    gt[1][0] = None
    as_float = {(i, k): gt_as_float(gt[i][k]) for i in range(2) for k in range(2) if gt[i][k] is not None}
    as_float[0, 1] = (as_float[0, 1] * F32(1.3) - F32(0.1)).astype(F32)      # unclamped on both sides
    gt[0][1] = torch.from_numpy(as_float[0, 1])
    res = stif.video.evaluate_sequence(model, frames, gt, times, metric="float")
    assert res["count"] == 3 and res["psnr"][1][0] is None and res["ssim"][1][0] is None
    ps, ss = [], []
    for (i, k), g in sorted(as_float.items()):
        p, s = restate_eval(host[i][k][:, :44, :52], g)
        print(i, k, res["psnr"][i][k], p, res["ssim"][i][k], s)
        assert within(res["psnr"][i][k], p, rel_tol(p, REL))
        assert within(res["ssim"][i][k], s, rel_tol(s, REL))
        ps.append(p)
        ss.append(s)
    assert within(res["avg_psnr"], float(np.mean(ps)), REL * abs(np.mean(ps)))
    assert within(res["avg_ssim"], float(np.mean(ss)), REL * abs(np.mean(ss)))

    gt[0][1] = rng.integers(0, 256, (44, 52, 3), dtype=np.uint8)
    for ch in ("y", "rgb"):
        assert stif.video.evaluate_sequence(model, frames, gt, times, channels=ch, metric="quantised") == \
            stif.video.evaluate_sequence(model, frames, gt, times, channels=ch)
    gt[0][0] = rng.integers(0, 256, (10, 52, 3), dtype=np.uint8)
    with pytest.raises(ValueError, match="smaller than the 11 x 11 window"):
        stif.video.evaluate_sequence(model, frames, gt, times, metric="float")
    with pytest.raises(ValueError, match="metric must be"):
        stif.video.evaluate_sequence(model, frames, gt, times, metric="ssim_matlab")
