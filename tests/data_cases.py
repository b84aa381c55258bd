"""Shared inputs of the training-batch tests: the recorded reference collate (tests/golden/collate_a2.npz, written by
tests/golden/make_data_golden.py) and the frames it was recorded on, regenerated here."""
import functools
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "collate_a2.npz")
SIZES = ((720, 1280), (1280, 720))
GT_IDX = ([0, 3, 8], [1, 4, 5])
TIMES = [[k / 8 for k in ks] for ks in GT_IDX]


@functools.lru_cache(maxsize=None)
def golden():
    return dict(np.load(GOLDEN))


@functools.lru_cache(maxsize=None)
def reference_frames():
    """[2][5] uint8 BGR frames: frame j of item b is RandomState(5 b + j).randint(0, 256, (H, W, 3))."""
    out = []
    for b, (H, W) in enumerate(SIZES):
        out.append([np.random.RandomState(5 * b + j).randint(0, 256, (H, W, 3)).astype(np.uint8) for j in range(5)])
    return out


def params_of(D, seed):
    """The recorded draws of ``seed`` as data.CollateParams."""
    d, G, x, y, hf, vf, rot = golden()[f"s{seed}_draws"]
    return D.CollateParams(float(d), int(G), int(x), int(y), bool(hf), bool(vf), bool(rot))


def bound(P_lq, P_gt):
    """Outputs are in [0, 1], each two fp32 dot products of P taps with sum |w| < 1.5, on either side of the
    comparison: (2 P + 4) 2^-24 1.5, from the actual tap counts."""
    return tuple((2 * P + 4) * 2.0 ** -24 * 1.5 for P in (P_lq, P_gt))


def taps(stif, params):
    geo = params.geometry
    return (stif.video.resize_tables(params.G, geo.lq, geo.lq_scale)[0].shape[1],
            stif.video.resize_tables(params.G, geo.gt, geo.gt_scale)[0].shape[1])


def check_against_recorded(batch, seed, tol_lq, tol_gt):
    """batch (host tensors or numpy) against the recorded reference output of ``seed``; prints the figures first."""
    g = golden()
    lq = np.asarray(batch["LQs"])
    gt = np.asarray(batch["GT"])
    assert lq.shape == g[f"s{seed}_LQs"].shape
    assert tuple(batch["shape"]) == tuple(g[f"s{seed}_shape"]) == gt.shape[-2:]
    e_lq = float(np.abs(lq - g[f"s{seed}_LQs"]).max())
    print(f"seed {seed}: max|LQs - reference| = {e_lq:.3e} (bound {tol_lq:.3e})")
    assert e_lq <= tol_lq
    if f"s{seed}_GT" in g:
        assert gt.shape == g[f"s{seed}_GT"].shape
        e_gt = float(np.abs(gt - g[f"s{seed}_GT"]).max())
        print(f"seed {seed}: max|GT - reference| = {e_gt:.3e} (bound {tol_gt:.3e})")
        assert e_gt <= tol_gt
    else:
        k = 16
        c = np.stack([gt[..., :k, :k], gt[..., :k, -k:], gt[..., -k:, :k], gt[..., -k:, -k:]], axis=-3)
        e_gt = float(np.abs(c - g[f"s{seed}_GT_corners"]).max())
        sums = gt.astype(np.float64).sum((-1, -2))
        e_sum = float(np.abs(sums - g[f"s{seed}_GT_sums"]).max())
        n = gt.shape[-1] * gt.shape[-2]
        print(f"seed {seed}: max|GT corners - reference| = {e_gt:.3e} (bound {tol_gt:.3e}), "
              f"max|plane sum - reference| = {e_sum:.3e} (bound {n * tol_gt:.3e})")
        assert e_gt <= tol_gt
        assert e_sum <= n * tol_gt          # every one of the n pixels within the bound
    times = [np.asarray(t) for t in batch["time"]]
    assert len(times) == 3
    for t, r in zip(times, g[f"s{seed}_time"]):
        assert t.shape == r.shape and np.array_equal(t, r)
