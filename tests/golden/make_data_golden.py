"""Record the reference's training collate (``data/__init__.py:124-154`` collate_function2 with
``data/util.py`` augment_a2 and imresize_np) -> tests/golden/collate_a2.npz.

Run by hand where the reference is present (it skips otherwise); only plain data is written.  ``cv2`` and ``lmdb``
are stubbed as in make_golden.py: the data package imports them at module level and the collate uses neither.

The batch has two items, one of 720 x 1280 frames and one of 1280 x 720 (portrait) frames.  Frame j of item b is
``RandomState(5 b + j).randint(0, 256, (H, W, 3))`` as uint8 -- two inputs, then three ground truths; the tests
regenerate the frames, they are not stored.  The GT candidates sampled are [0, 3, 8] and [1, 4, 5], so the times are
k / 8.  ``collate_function2`` itself runs under ``random.seed(s)`` for s in SEEDS.  Stored per seed s:
  s{s}_draws   d, G, x, y, hflip, vflip, rot90 (float64), replayed here from ``random.Random(s)`` and asserted to
               reproduce the reference's output shapes
  s{s}_LQs     [2, 2, 3, 32, 32] in full
  s{s}_GT      in full for the seed with the smallest G only; for the others s{s}_GT_corners
               [2, 3, 3, 4, 16, 16] (top-left, top-right, bottom-left, bottom-right) and s{s}_GT_sums [2, 3, 3] (fp64)
  s{s}_shape, s{s}_time [3, 2, 1]

Usage: python tests/golden/make_data_golden.py
"""
import os
import random
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/codes"
SEEDS = (0, 1, 2, 3)
SIZES = ((720, 1280), (1280, 720))
GT_IDX = ([0, 3, 8], [1, 4, 5])


def frames_of(b):
    H, W = SIZES[b]
    return [np.random.RandomState(5 * b + j).randint(0, 256, (H, W, 3)).astype(np.uint8) for j in range(5)]


def replay(seed):
    """The draws of collate_function2 + augment_a2 from a fresh generator."""
    rng = random.Random(seed)
    d = rng.uniform(2, 4)
    G = int(np.floor(64 * d))
    x = rng.randint(0, max(0, 720 - G))
    y = rng.randint(0, max(0, 1280 - G))
    flags = [rng.random() < 0.5 for _ in range(3)]
    return d, G, x, y, flags


def corners(a, k=16):
    return np.stack([a[..., :k, :k], a[..., :k, -k:], a[..., -k:, :k], a[..., -k:, -k:]], axis=-3)


def main():
    if not os.path.isdir(REF):
        print("reference not present; nothing written")
        return
    import torch
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    sys.modules.setdefault("lmdb", types.ModuleType("lmdb"))
    sys.path.insert(0, REF)
    import data as refdata

    items = []
    for b in range(2):
        fr = frames_of(b)
        times = [torch.tensor([k / 8]) for k in GT_IDX[b]]
        items.append((fr[:2], fr[2:], times, None))
    draws = {s: replay(s) for s in SEEDS}
    small = min(SEEDS, key=lambda s: draws[s][1])
    res = {"seeds": np.array(SEEDS), "full_gt_seed": np.array(small)}
    for s in SEEDS:
        random.seed(s)
        out = refdata.collate_function2(items)
        d, G, x, y, flags = draws[s]
        lq, gt = out["LQs"].numpy(), out["GT"].numpy()
        side = int(np.ceil(G / 2))
        assert lq.shape == (2, 2, 3, 32, 32), lq.shape
        assert gt.shape == (2, 3, 3, side, side), (gt.shape, side)
        assert tuple(out["shape"]) == (side, side)
        res[f"s{s}_draws"] = np.array([d, G, x, y] + [float(f) for f in flags], np.float64)
        res[f"s{s}_LQs"] = lq
        if s == small:
            res[f"s{s}_GT"] = gt
        else:
            res[f"s{s}_GT_corners"] = corners(gt)
            res[f"s{s}_GT_sums"] = gt.astype(np.float64).sum((-1, -2))
        res[f"s{s}_shape"] = np.array(out["shape"])
        res[f"s{s}_time"] = np.stack([t.numpy() for t in out["time"]])
        print(f"seed {s}: d {d:.4f} G {G} x {x} y {y} flags {flags} GT {gt.shape}")
    path = os.path.join(HERE, "collate_a2.npz")
    np.savez(path, **res)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
