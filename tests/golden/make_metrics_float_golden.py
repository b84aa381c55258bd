"""Generate tests/golden/metrics_float.npz by running the REFERENCE's own float-protocol metrics on the CPU.

Like make_metrics_golden.py this script is run by hand (it does nothing when the reference is absent) and only
its output -- one new input and the recorded values -- is committed.

The reference's ``eval_metrics`` (myutils.py:234-241) is reproduced call for call: ``calc_psnr`` on the raw
tensors, ``ssim_matlab(output.clamp(0, 1), gt.clamp(0, 1), val_range=1.)``; ``myutils.ssim`` is called the same
way for the planar mode.  The shims are make_metrics_golden.install_shims (``Tensor.cuda`` is the identity there,
so the reference's windows stay on the CPU).

Cases: the four inputs of metrics.npz with H, W >= 11, read from that file and not stored again, and one new input,
33x65 (n = 2): its last tile row and column own a single pixel line, whose halo is almost entirely replicated.

For every case the file holds, per item, the reference's values (``ref``), the values of the fp64 restatement the
engine implements (``exact``: the same definition with the fp64 window of stif_metric_window, by direct edge
padding on all three axes -- not through the 3 x 3 channel mix, so that it checks the mix) and their absolute
difference (``diff``: the reference's fp32 window and fp32 convolutions).  Columns: calc_psnr, ssim_volume,
ssim_planar.

Usage:  python tests/golden/make_metrics_float_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_metrics_golden as G  # noqa: E402

OLD_CASES = ["11x11", "12x37", "45x70", "32x64"]
NEW_CASES = {"33x65": (2, 33, 65)}
COLUMNS = ["calc_psnr", "ssim_volume", "ssim_planar"]


# ------------------------------------------------------------------ the fp64 restatement (numpy, direct padding)
def filt(v, k, volume):
    """v [3, H, W] float64 -> the 11-tap Gaussian over (channel,) row, column with replicate padding of 5"""
    _, H, W = v.shape
    v = np.pad(v, ((5, 5) if volume else (0, 0), (5, 5), (5, 5)), mode="edge")
    if volume:
        v = sum(k[j] * v[j:j + 3] for j in range(11))
    v = sum(k[j] * v[:, j:j + H] for j in range(11))
    return sum(k[j] * v[:, :, j:j + W] for j in range(11))


def exact_values(pred, ref):
    """pred, ref [3, H, W] fp32 -> (calc_psnr, ssim_volume, ssim_planar) in float64"""
    k = G.window11()
    d = pred.astype(np.float64) - ref.astype(np.float64)
    out = [-10.0 * np.log10((d * d).mean() + 1e-8)]
    a = np.clip(pred, 0, 1).astype(np.float64)
    b = np.clip(ref, 0, 1).astype(np.float64)
    C1, C2 = 1e-4, 9e-4
    for volume in (True, False):
        mu1, mu2 = filt(a, k, volume), filt(b, k, volume)
        s1 = filt(a * a, k, volume) - mu1 * mu1
        s2 = filt(b * b, k, volume) - mu2 * mu2
        s12 = filt(a * b, k, volume) - mu1 * mu2
        m = ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))
        out.append(m.mean())
    return out


def main():
    if not os.path.isdir(G.REF):
        print("reference absent; nothing to do")
        return
    G.install_shims()
    import torch
    import myutils

    cases = {}
    with np.load(os.path.join(HERE, "metrics.npz")) as z:
        for name in OLD_CASES:
            pred, gt, eq = z[f"{name}__pred"].copy(), z[f"{name}__gt"], int(z[f"{name}__eq_item"])
            if eq >= 0:
                pred[eq] = G.gt_as_float(gt[eq])
            cases[name] = (pred, gt, eq)
    out = {}
    G.CASES.update(NEW_CASES)
    rng = np.random.default_rng(20241019)
    for name in NEW_CASES:
        pred, gt, eq = G.make_case(name, rng)
        assert eq < 0 and pred.min() < 0 and pred.max() > 1
        cases[name] = (pred, gt, eq)
        out[f"{name}__pred"], out[f"{name}__gt"] = pred, gt

    for name, (pred, gt, eq) in cases.items():
        n = pred.shape[0]
        ref, exact = np.empty((n, 3)), np.empty((n, 3))
        for i in range(n):
            gtf = G.gt_as_float(gt[i])
            o, g = torch.from_numpy(pred[i].copy()), torch.from_numpy(gtf)
            # myutils.py:237,240
            ref[i, 0] = myutils.calc_psnr(o, g)
            ref[i, 1] = float(myutils.ssim_matlab(o.unsqueeze(0).clamp(0, 1), g.unsqueeze(0).clamp(0, 1), val_range=1.))
            ref[i, 2] = float(myutils.ssim(o.unsqueeze(0).clamp(0, 1), g.unsqueeze(0).clamp(0, 1), val_range=1.))
            exact[i] = exact_values(pred[i], gtf)
            if i == eq:
                assert exact[i, 1] == 1.0 and exact[i, 2] == 1.0 and ref[i, 1] == 1.0 and ref[i, 2] == 1.0, (ref[i], exact[i])
            else:       # the reference alone: away from the degenerate ends
                assert 10 < ref[i, 0] < 60 and all(0.05 < ref[i, c] < 0.98 for c in (1, 2)), ref[i]
        diff = np.abs(ref - exact)
        assert diff[:, 1:].max() < 5e-5 and diff[:, 0].max() < 1e-5, (name, diff)
        out.update({f"{name}__ref": ref, f"{name}__exact": exact, f"{name}__diff": diff})
        print(name, "max |ref - exact| per column:", dict(zip(COLUMNS, diff.max(0))))
    out["columns"] = np.array(COLUMNS)
    path = os.path.join(HERE, "metrics_float.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 100 * 1024


if __name__ == "__main__":
    main()
