"""Generate tests/golden/metrics.npz by running the REFERENCE's own metric functions on the CPU.

Like make_golden.py this script is the only thing that touches the reference checkout; it is run by hand
(it does nothing when the reference is absent) and only its output -- inputs and recorded values -- is committed.

The reference's evaluation loop (myutils.test_metric_adobe_liif4x, myutils.py:1151-1174) is reproduced call for
call with its own ``utils.util.tensor2img``, ``data.util.bgr2ycbcr``, ``utils.util.calculate_psnr``,
``utils.util.ssim`` and ``myutils.calc_psnr``.  Shims, in the manner of make_golden.install_shims:
  1. stub ``torchvision`` (``transforms`` names, ``utils.make_grid``: imported, never called on a 3-D tensor);
  2. a ``cv2`` module with the two functions ``ssim`` calls: ``getGaussianKernel`` by its closed form
     (exp(-(i - (n-1)/2)^2 / (2 sigma^2)) times the reciprocal of the sum) and ``filter2D`` as
     ``scipy.ndimage.correlate(mode="mirror")`` (BORDER_REFLECT_101) per channel.  Only the centres whose window
     lies inside the image are kept by ``ssim``, so the border mode never reaches a recorded value.

For every case the file holds the inputs, the reference's values, the values of the exact-integer restatement the
engine implements (the ground truth as exact integers in float64; the reference's GT goes through ``uint8 / 255`` in
fp32 and an fp32 cast of its luma) and their absolute difference.  Columns of ref / exact / diff, per item:
psnr_y, ssim_y, psnr_rgb, ssim_rgb, calc_psnr (float PSNR against gt RGB / 255).

Usage:  python tests/golden/make_metrics_golden.py
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF  # noqa: E402  (the reference checkout make_golden.py reads)
F32 = np.float32

# name: (n, H, W); the kernel's tile is 32 x 32
CASES = {
    "11x11": (1, 11, 11),      # exactly one SSIM window
    "10x23": (1, 10, 23),      # no window: SSIM is NaN
    "12x37": (1, 12, 37),      # crosses one tile edge
    "45x70": (3, 45, 70),      # crosses tile edges both ways with a remainder; three different items
    "32x64": (1, 32, 64),      # exact multiples of the tile
}
EQ_ITEM = {"45x70": 1}         # this item's prediction is its ground truth / 255


def window11():
    x = np.arange(11, dtype=np.float64) - 5.0
    k = np.exp(-(x * x) / 4.5)
    return k * (1.0 / k.sum())


def install_shims():
    import scipy.ndimage as ndi
    import torch

    tv = types.ModuleType("torchvision")
    tvt = types.ModuleType("torchvision.transforms")
    for n in ["Resize", "Compose", "ToTensor", "Normalize"]:
        setattr(tvt, n, object)
    tvu = types.ModuleType("torchvision.utils")
    tvu.make_grid = None
    tv.transforms, tv.utils = tvt, tvu
    sys.modules.update({"torchvision": tv, "torchvision.transforms": tvt, "torchvision.utils": tvu})

    cv2 = types.ModuleType("cv2")

    def getGaussianKernel(ksize, sigma):
        x = np.arange(ksize, dtype=np.float64) - (ksize - 1) / 2.0
        k = np.exp(-(x * x) / (2.0 * sigma * sigma))
        return (k * (1.0 / k.sum())).reshape(ksize, 1)

    def filter2D(src, ddepth, kernel):
        assert ddepth == -1
        if src.ndim == 2:
            return ndi.correlate(src, kernel, mode="mirror")
        return np.stack([ndi.correlate(src[..., c], kernel, mode="mirror") for c in range(src.shape[2])], -1)

    cv2.getGaussianKernel, cv2.filter2D = getGaussianKernel, filter2D
    sys.modules["cv2"] = cv2
    torch.Tensor.cuda = lambda self, *a, **k: self
    sys.path.insert(0, REF)


# ------------------------------------------------------------------ the exact-integer restatement (numpy)
def quantise(pred):
    """tensor2img: round(clamp(o, 0, 1) * 255) in fp32, half to even -> float64 integers, [3, H, W] RGB."""
    return np.rint(np.clip(pred.astype(F32), F32(0), F32(1)) * F32(255.0)).astype(np.float64)


def luma(b, g, r):
    return (24.966 * b + 128.553 * g + 65.481 * r) / 255.0 + 16.0


def plane_sums(a, b, k):
    """(sse, npix, ssim_sum, nwin) of two float64 planes; separable 11-tap window, valid region only."""
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
    """pred [3, H, W] fp32 RGB, gt [H, W, 3] uint8 BGR -> (sse, npix, ssim_sum, nwin)."""
    k = window11()
    q = quantise(pred)
    g = gt.astype(np.float64)
    if channels == "y":
        return plane_sums(luma(q[2], q[1], q[0]), luma(g[..., 0], g[..., 1], g[..., 2]), k)
    parts = [plane_sums(q[c], g[..., 2 - c], k) for c in range(3)]
    return tuple(sum(p[i] for p in parts) for i in range(4))


def finish(s):
    sse, npix, ssum, nwin = s
    mse = sse / npix
    psnr = float("inf") if mse == 0 else 20.0 * np.log10(255.0 / np.sqrt(mse))
    return psnr, (ssum / nwin if nwin else float("nan"))


def gt_as_float(gt):
    """the float ground truth of calc_psnr: RGB planes of gt / 255 in fp32"""
    return np.ascontiguousarray(gt[..., ::-1].transpose(2, 0, 1)).astype(F32) / F32(255.0)


# ------------------------------------------------------------------ inputs
def tie(kk):
    """an fp32 value v with v * 255 == kk + 0.5 exactly in fp32 (an exact rounding tie of tensor2img)"""
    v = F32((kk + 0.5) / 255.0)
    for _ in range(8):
        p = F32(v * F32(255.0))
        if p == F32(kk + 0.5):
            return v
        v = np.nextafter(v, F32(2.0) if p < kk + 0.5 else F32(-1.0), dtype=F32)
    raise AssertionError(f"no fp32 tie for {kk}")


def make_case(name, rng):
    n, H, W = CASES[name]
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    gt = np.empty((n, H, W, 3), np.uint8)
    pred = np.empty((n, 3, H, W), F32)
    for i in range(n):
        for c in range(3):
            smooth = 128 + 120 * np.sin(0.21 * yy + 0.6 * c + i) * np.cos(0.17 * xx - 0.4 * c + 0.5 * i)
            gt[i, :, :, c] = np.clip(np.rint(smooth + rng.normal(0, 12, (H, W))), 0, 255).astype(np.uint8)
        base = gt_as_float(gt[i]).astype(np.float64) + rng.normal(0, 0.06, (3, H, W))
        # multiples of 1/256: exact in fp32 (and compressible); the smooth extremes leave [0, 1] on both sides
        pred[i] = (np.rint(base * 256) / 256).astype(F32)
        flat = pred[i].reshape(-1)
        pos = rng.choice(flat.size, size=min(12, flat.size // 4), replace=False)
        ks = [0, 1, 2, 3, 100, 101, 126, 127, 200, 201, 253, 254]
        for j, p in enumerate(pos):
            flat[p] = tie(ks[j % len(ks)])
        flat[rng.choice(flat.size, 2, replace=False)] = [F32(-0.25), F32(1.25)]
    eq = EQ_ITEM.get(name, -1)
    if eq >= 0:
        pred[eq] = gt_as_float(gt[eq])
    return pred, gt, eq


def main():
    if not os.path.isdir(REF):
        print("reference absent; nothing to do")
        return
    install_shims()
    import torch
    import utils.util as U
    from data.util import bgr2ycbcr
    import myutils

    out = {"window": U.cv2.getGaussianKernel(11, 1.5).reshape(-1)}
    assert np.abs(out["window"] - window11()).max() == 0
    rng = np.random.default_rng(20240611)
    for name in CASES:
        pred, gt, eq = make_case(name, rng)
        n = pred.shape[0]
        ref, exact = np.empty((n, 5)), np.empty((n, 5))
        for i in range(n):
            # myutils.py:1127,1156-1163 (the LIIF branch and its commented-out three-channel alternative)
            gt_f = gt[i].astype(np.float32) / 255.
            output1 = U.tensor2img(torch.from_numpy(pred[i].copy())) / 255.
            with np.errstate(invalid="ignore"), __import__("warnings").catch_warnings():
                __import__("warnings").simplefilter("ignore")
                ref[i, 2] = U.calculate_psnr(output1 * 255, gt_f * 255)
                ref[i, 3] = U.ssim(output1 * 255, gt_f * 255)
                output_y = bgr2ycbcr(output1.copy(), only_y=True)
                gt_y = bgr2ycbcr(gt_f.copy(), only_y=True)
                ref[i, 0] = U.calculate_psnr(output_y * 255, gt_y * 255)
                ref[i, 1] = U.ssim(output_y * 255, gt_y * 255)
            ref[i, 4] = myutils.calc_psnr(torch.from_numpy(pred[i]), torch.from_numpy(gt_as_float(gt[i])))
            exact[i, 0:2] = finish(exact_sums(pred[i], gt[i], "y"))
            exact[i, 2:4] = finish(exact_sums(pred[i], gt[i], "rgb"))
            d = pred[i].astype(np.float64) - gt_as_float(gt[i]).astype(np.float64)
            exact[i, 4] = -10.0 * np.log10((d * d).mean() + 1e-8)
            has_win = min(pred.shape[2:]) >= 11
            if i == eq:
                # exact integers: PSNR inf and SSIM exactly 1 in both modes.  The reference agrees in RGB mode; its
                # Y-mode PSNR is finite (~150 dB) only because of the fp32 noise in its GT luma: diff is inf there
                assert exact[i, 0] == np.inf and exact[i, 2] == np.inf and exact[i, 1] == 1.0 and exact[i, 3] == 1.0
                assert ref[i, 0] > 120 and ref[i, 2] == np.inf and abs(ref[i, 1] - 1) < 1e-9 and ref[i, 3] == 1.0, ref[i]
            else:      # the reference alone: finite and away from the degenerate ends
                assert all(10 < ref[i, c] < 60 for c in (0, 2, 4)), ref[i]
                assert (not has_win) or all(0.05 < ref[i, c] < 0.98 for c in (1, 3)), ref[i]
            assert has_win or (np.isnan(ref[i, 1]) and np.isnan(ref[i, 3]))
        same = (ref == exact) | (np.isnan(ref) & np.isnan(exact))
        with np.errstate(invalid="ignore"):
            diff = np.where(same, 0.0, np.abs(ref - exact))
        fin = np.ones_like(diff, bool)
        if eq >= 0:
            fin[eq, 0] = False
            assert diff[eq, 0] == np.inf
        assert diff[fin].max() < 1e-5, (name, diff)
        stored = pred.copy()
        if eq >= 0:
            stored[eq] = 0          # rebuilt by the tests as gt RGB / 255 (fp32): incompressible otherwise
        out.update({f"{name}__pred": stored, f"{name}__gt": gt, f"{name}__eq_item": np.int64(eq),
                    f"{name}__ref": ref, f"{name}__exact": exact, f"{name}__diff": diff})
        print(name, "max |ref - exact| per column:", diff.max(0))
    path = os.path.join(HERE, "metrics.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 100 * 1024


if __name__ == "__main__":
    main()
