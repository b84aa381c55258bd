"""On-device PSNR / SSIM (csrc/metrics.hip through stif_amd.metrics and video.evaluate_*) against
tests/golden/metrics.npz.

Tolerances.  Against the exact-integer float64 values: 1e-9 relative -- float64 sums of at most 2^13 terms per
case, reordered, give N * 2^-53 ~ 1e-12, and three decades are left for the per-pixel division chain.  Against
the reference's own functions: twice the difference the fixture records for that case and column (one sample of
the reference's fp32 ground-truth noise, not a bound) plus 1e-9."""
import ctypes as C

import numpy as np
import pytest

from test_metrics_host import (CASES, COLS, gold, gt_as_float, load_case, rel_tol, restate,  # noqa: F401
                               restate_float, within)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
REL = 1e-9


def _rel(want):
    """1e-9 relative; an infinite expected value (PSNR of identical images) must be matched exactly"""
    return rel_tol(want, REL)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


@pytest.fixture(scope="module")
def scored(stif, gold):
    """every fixture case in both modes, computed once: {(name, channels): (psnr [n], ssim [n])}"""
    res = {}
    for name in CASES:
        pred, gt = load_case(gold, name)[:2]
        for ch in COLS:
            res[name, ch] = stif.metrics.psnr_ssim(_dev(pred), gt, channels=ch)
    return res


@pytest.mark.parametrize("ch", sorted(COLS))
@pytest.mark.parametrize("name", CASES)
def test_matches_exact_integer_values(scored, gold, name, ch):
    exact = load_case(gold, name)[3]
    psnr, ssim = scored[name, ch]
    cp, cs = COLS[ch]
    assert psnr.dtype == np.float64 and psnr.shape == (exact.shape[0],)
    for i in range(exact.shape[0]):
        print(name, ch, i, "psnr", psnr[i], exact[i, cp], "ssim", ssim[i], exact[i, cs])
        assert within(psnr[i], exact[i, cp], _rel(exact[i, cp])), (i, psnr[i], exact[i, cp])
        assert within(ssim[i], exact[i, cs], _rel(exact[i, cs])), (i, ssim[i], exact[i, cs])


@pytest.mark.parametrize("ch", sorted(COLS))
@pytest.mark.parametrize("name", CASES)
def test_matches_reference_functions(scored, gold, name, ch):
    _, _, ref, _, diff = load_case(gold, name)
    psnr, ssim = scored[name, ch]
    cp, cs = COLS[ch]
    for i in range(ref.shape[0]):
        assert within(psnr[i], ref[i, cp], 2 * diff[i, cp] + 1e-9), (i, psnr[i], ref[i, cp], diff[i, cp])
        assert within(ssim[i], ref[i, cs], 2 * diff[i, cs] + 1e-9), (i, ssim[i], ref[i, cs], diff[i, cs])


def test_identical_item_and_no_window(scored):
    for ch in COLS:
        psnr, ssim = scored["45x70", ch]
        assert psnr[1] == np.inf and abs(ssim[1] - 1.0) <= REL     # the squared error is exactly 0
        assert np.isnan(scored["10x23", ch][1]).all() and np.isfinite(scored["10x23", ch][0]).all()


@pytest.mark.parametrize("ch", sorted(COLS))
def test_strided_view_equals_dense_bit_for_bit(stif, gold, ch):
    """the 45x70 data inside a 48x72 buffer: the prediction as a torch view (strides passed through), the ground
    truth with a row pitch through the C ABI; the padding holds values that would change every sum"""
    M, L = stif.metrics, stif._lib
    pred, gt = load_case(gold, "45x70")[:2]
    flags = M.mode_flags(ch, True)
    dense = M.sums(_dev(pred), gt, flags).cpu().numpy()
    big = torch.full((3, 3, 48, 72), 0.37, device="cuda:0")
    big[:, :, :45, :70] = _dev(pred)
    view = big[:, :, :45, :70]
    assert not view.is_contiguous()
    got = M.sums(view, gt, flags).cpu().numpy()
    assert got.tobytes() == dense.tobytes()
    gbig = torch.full((3, 48, 72, 3), 99, dtype=torch.uint8, device="cuda:0")
    gbig[:, :45, :70] = _dev(gt)
    a = L.MetricArgs()
    a.pred, a.pred_item, a.pred_plane, a.pred_pitch = big.data_ptr(), 3 * 48 * 72, 48 * 72, 72
    a.gt_u8, a.gt_item, a.gt_pitch = gbig.data_ptr(), 48 * 72 * 3, 72 * 3
    a.n, a.H, a.W, a.flags = 3, 45, 70, flags
    nbytes = L.lib().stif_metric_workspace_size(3, 45, 70, flags)
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device="cuda:0")
    out = torch.empty(3, 4, dtype=torch.float64, device="cuda:0")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    L.check(L.lib().stif_metric_psnr_ssim(C.byref(a), out.data_ptr(), ws.data_ptr(), nbytes, st), "metric")
    assert out.cpu().numpy().tobytes() == dense.tobytes()
    # the sums themselves: pixel and window counts are exact
    planes = 1 if ch == "y" else 3
    assert (dense[:, 1] == planes * 45 * 70).all() and (dense[:, 3] == planes * 35 * 60).all()


def test_two_calls_are_bit_identical(stif, gold):
    M = stif.metrics
    pred, gt = load_case(gold, "45x70")[:2]
    p, g = _dev(pred), _dev(gt)
    for flags in (M.mode_flags("y", True), M.mode_flags("rgb", True)):
        a = M.sums(p, g, flags).cpu().numpy()
        b = M.sums(p, g, flags).cpu().numpy()
        assert a.tobytes() == b.tobytes()


def test_psnr_only_mode(stif, gold, scored):
    pred, gt = load_case(gold, "45x70")[:2]
    for ch in COLS:
        psnr, ssim = stif.metrics.psnr_ssim(_dev(pred), gt, channels=ch, ssim=False)
        assert np.array_equal(psnr, scored["45x70", ch][0]) and np.isnan(ssim).all()


@pytest.mark.parametrize("name", CASES)
def test_psnr_float_matches_calc_psnr(stif, gold, name):
    pred, gt, ref, exact, diff = load_case(gold, name)
    fref = np.stack([gt_as_float(g) for g in gt])
    got = stif.metrics.psnr_float(_dev(pred), _dev(fref))
    assert got.shape == (pred.shape[0],)
    for i in range(pred.shape[0]):
        print(name, i, got[i], exact[i, 4], ref[i, 4])
        assert within(got[i], exact[i, 4], _rel(exact[i, 4]))
        assert within(got[i], ref[i, 4], 2 * diff[i, 4] + 1e-9)


def test_bad_inputs_raise(stif):
    M = stif.metrics
    p = torch.zeros(1, 3, 12, 12, device="cuda:0")
    with pytest.raises(ValueError):
        M.psnr_ssim(p, np.zeros((1, 12, 13, 3), np.uint8))
    with pytest.raises(ValueError):
        M.psnr_ssim(p, np.zeros((1, 12, 12, 3), np.float32))
    with pytest.raises(ValueError):
        M.psnr_ssim(p.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2), np.zeros((1, 12, 12, 3), np.uint8))


@pytest.fixture(scope="module")
def model(stif, sd):
    m = stif.LunaTokis(64, 6, 8, 5, 40)
    m.load_state_dict(sd)
    return m


def test_evaluate_sequence(stif, model):
    """3 frames of 11x13 (padded to 12x16: 48x64 outputs) at times 0 and 0.5 against random 44x52 ground truth:
    the top-left crop of every output is scored in place and must equal the numpy restatement applied to
    run_sequence's outputs copied to the host."""
    rng = np.random.default_rng(7)
    frames = torch.from_numpy(rng.random((3, 3, 11, 13)).astype(np.float32)).to("cuda:0")
    times = [0.0, 0.5]
    outs = stif.video.run_sequence(model, frames, times)
    assert tuple(outs[0][0].shape) == (3, 48, 64)
    host = [[o.cpu().numpy().copy() for o in row] for row in outs]
    gt = [[rng.integers(0, 256, (44, 52, 3), dtype=np.uint8) for _ in times] for _ in range(2)]
    gt[1][0] = None
    for ch in COLS:
        res = stif.video.evaluate_sequence(model, frames, gt, times, channels=ch)
        assert res["count"] == 3 and res["psnr"][1][0] is None and res["ssim"][1][0] is None
        ps, ss = [], []
        for i in range(2):
            for k in range(2):
                if gt[i][k] is None:
                    continue
                p, s = restate(host[i][k][:, :44, :52], gt[i][k], ch)
                print(ch, i, k, res["psnr"][i][k], p, res["ssim"][i][k], s)
                assert within(res["psnr"][i][k], p, _rel(p))
                assert within(res["ssim"][i][k], s, _rel(s))
                ps.append(p)
                ss.append(s)
        assert within(res["avg_psnr"], float(np.mean(ps)), REL * abs(np.mean(ps)))
        assert within(res["avg_ssim"], float(np.mean(ss)), REL * abs(np.mean(ss)))


def test_evaluate_folder(stif, model, tmp_path, capsys):
    """frames on disk: two 12x16 low-resolution PNGs, ground truth for the first of the two output frames"""
    from PIL import Image
    rng = np.random.default_rng(11)
    lr = rng.integers(0, 256, (2, 12, 16, 3), dtype=np.uint8)        # RGB on disk
    g0 = rng.integers(0, 256, (48, 64, 3), dtype=np.uint8)
    (tmp_path / "lr").mkdir()
    (tmp_path / "gt").mkdir()
    for i in range(2):
        Image.fromarray(lr[i]).save(tmp_path / "lr" / f"{i}.png")
    Image.fromarray(g0).save(tmp_path / "gt" / "0.png")
    res = stif.video.evaluate_folder(model, str(tmp_path / "lr"), str(tmp_path / "gt"), times=[0.25, 0.5])
    frames = torch.from_numpy(lr).to("cuda:0").permute(0, 3, 1, 2).float() / 255.0
    want = stif.video.evaluate_sequence(model, frames.contiguous(), [[g0[:, :, ::-1].copy(), None]], [0.25, 0.5])
    assert res["count"] == 1 and res["psnr"] == want["psnr"] and res["ssim"] == want["ssim"]
    assert capsys.readouterr().out.strip().endswith(
        "AVG PSNR: {:.4f}, AVG SSIM: {:.4f}".format(res["avg_psnr"], res["avg_ssim"]))
