"""Training batches without a GPU (stif_amd.data): the draw order, the numpy batch builder
against the recorded reference collate (tests/golden/collate_a2.npz: collate_function2 itself, run on two items
of 720 x 1280 and 1280 x 720 frames under random.seed(0..3)), the window index, and what is rejected.

The tolerance against the reference is computed from the tap counts of the case (data_cases.bound), never a constant:
outputs are in [0, 1] and each is two fp32 dot products of P taps with sum |w| < 1.5."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

import data_cases as DC

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = (0, 1, 2, 3)


@pytest.fixture(scope="module")
def D(stif):
    return stif.data


def test_fixture_is_what_the_issue_describes():
    g = DC.golden()
    assert tuple(g["seeds"]) == SEEDS and int(g["full_gt_seed"]) == 1
    assert [int(g[f"s{s}_shape"][0]) for s in SEEDS] == [118, 73, 125, 79]
    assert g["s1_GT"].shape == (2, 3, 3, 73, 73)
    assert os.path.getsize(DC.GOLDEN) < 1 << 20


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("size", [(720, 1280), (1280, 720)])
def test_draw_order_matches_reference(D, seed, size):
    rec = DC.params_of(D, seed)
    got = D.draw_collate_params(random.Random(seed), *size)
    assert got == rec
    assert got.geometry.lq == 32 and got.geometry.gt == int(DC.golden()[f"s{seed}_shape"][0])
    # the crop is at (row x, col y) in the landscape frame and at (row y, col x) in the portrait one
    assert got.crop_origin(*size) == ((rec.x, rec.y) if size[0] == 720 else (rec.y, rec.x))
    assert got.flags == int(rec.hflip) + 2 * int(rec.vflip) + 4 * int(rec.rot90)


def test_all_three_flags_are_always_drawn(D):
    a, c = random.Random(5), random.Random(5)
    D.draw_collate_params(a, 720, 1280)
    G = int(np.floor(64 * c.uniform(2, 4)))
    c.randint(0, 720 - G), c.randint(0, 1280 - G), c.random(), c.random(), c.random()
    assert a.random() == c.random()          # the generator stands where the reference's would


def test_resize_geometry(D):
    assert D.resize_geometry(64, 3.0) == D.Geometry(192, 1 / 6, 0.5, 32, 96)
    for lq_size, lo, hi, side in ((8, 16, 32, 4), (16, 32, 64, 8), (64, 128, 256, 32)):
        for d in np.linspace(2, 4, 41):
            geo = D.resize_geometry(lq_size, float(d))
            assert lo <= geo.G <= hi and geo.lq == side and geo.gt == -(-geo.G // 2)
    assert D.resize_geometry().G == 128          # lq_size defaults to the reference's 64


@pytest.mark.parametrize("seed", SEEDS)
def test_build_batch_host_matches_reference(stif, D, seed):
    params = DC.params_of(D, seed)
    batch = D.build_batch_host(DC.reference_frames(), params, DC.TIMES)
    tol_lq, tol_gt = DC.bound(*DC.taps(stif, params))
    assert batch["LQs"].dtype == batch["GT"].dtype == batch["time"][0].dtype
    DC.check_against_recorded(batch, seed, tol_lq, tol_gt)


def test_build_batch_host_takes_crops_or_whole_frames(D):
    params = D.CollateParams(2.37, 37, 11, 40, True, False, True, 16)
    rng = np.random.RandomState(3)
    frames = [[rng.randint(0, 256, s + (3,)).astype(np.uint8) for _ in range(5)] for s in ((70, 90), (90, 70))]
    crops = []
    for item in frames:
        r, c = params.crop_origin(*item[0].shape[:2])
        crops.append([np.ascontiguousarray(f[r:r + 37, c:c + 37]) for f in item])
    a = D.build_batch_host(frames, params, [[0, 0.5, 1], [0.125, 0.25, 0.375]])
    b = D.build_batch_host(crops, params, [[0, 0.5, 1], [0.125, 0.25, 0.375]])
    assert tuple(a["LQs"].shape) == (2, 2, 3, 8, 8) and tuple(a["GT"].shape) == (2, 3, 3, 19, 19)
    assert a["shape"] == (19, 19)
    assert np.array_equal(a["LQs"].numpy(), b["LQs"].numpy()) and np.array_equal(a["GT"].numpy(), b["GT"].numpy())
    assert [t.flatten().tolist() for t in a["time"]] == [[0, 0.125], [0.5, 0.25], [1, 0.375]]


def _tree(root, counts, size=(24, 32), ext=".png"):
    from PIL import Image
    for v, n in counts.items():
        os.makedirs(os.path.join(root, v))
        for k in range(n):
            Image.fromarray(np.full(size + (3,), k, np.uint8)).save(os.path.join(root, v, f"{k}{ext}"))


def test_clip_index(D, tmp_path):
    root = str(tmp_path)
    _tree(root, {"a": 8, "b": 9, "c": 12})
    assert len(D.ClipIndex(root, ["a"])) == 0
    assert len(D.ClipIndex(root, ["b"])) == 1
    idx = D.ClipIndex(root, ["a", "b\n", "c"])
    assert len(idx) == 5
    stem = lambda p: int(os.path.splitext(os.path.basename(p))[0])
    # numeric order: 10.png and 11.png come after 9.png
    assert [[stem(p) for p in w] for w in idx.inputs[1:]] == [[0, 8], [1, 9], [2, 10], [3, 11]]
    assert [stem(p) for p in idx.candidates[4]] == list(range(3, 12))
    assert all(os.path.basename(os.path.dirname(p)) == "c" for p in idx.candidates[4])
    rng, replay = random.Random(9), random.Random(9)
    for i in range(5):
        paths, times = idx.sample(i, rng)
        ks = sorted(replay.sample(range(9), 3))
        assert len(paths) == 5 and paths[:2] == list(idx.inputs[i])
        assert paths[2:] == [idx.candidates[i][k] for k in ks]
        assert times == [k / 8 for k in ks] and times == sorted(times) and len(set(times)) == 3
        assert all(t in [j / 8 for j in range(9)] for t in times)


def test_rejections(stif, D, tmp_path):
    with pytest.raises(ValueError, match="multiple of 8"):
        D.resize_geometry(12, 2.0)
    with pytest.raises(ValueError, match="multiple of 8"):
        D.draw_collate_params(random.Random(0), 720, 1280, lq_size=12)
    params = D.CollateParams(2.0, 32, 0, 0, False, False, False, 16)
    ok = [[np.zeros((40, 48, 3), np.uint8)] * 5]
    D.build_batch_host(ok, params)
    with pytest.raises(ValueError, match="does not fit"):           # a crop larger than the frame
        D.build_batch_host([[np.zeros((30, 48, 3), np.uint8)] * 5], params)
    with pytest.raises(ValueError, match="does not fit"):
        D.build_batch_host(ok, D.CollateParams(2.0, 32, 9, 0, False, False, False, 16))
    with pytest.raises(ValueError, match="share a size"):           # mixed sizes within an item
        D.build_batch_host([[np.zeros((40, 48, 3), np.uint8)] * 4 + [np.zeros((48, 40, 3), np.uint8)]], params)
    with pytest.raises(ValueError, match="uint8"):
        D.build_batch_host([[np.zeros((40, 48, 3), np.float32)] * 5], params)
    with pytest.raises(ValueError, match=r"\[H, W, 3\]"):
        D.build_batch_host([[np.zeros((40, 48, 4), np.uint8)] * 5], params)
    with pytest.raises(ValueError, match=r"\[B\]\[5\]"):
        D.build_batch_host([[np.zeros((40, 48, 3), np.uint8)] * 4], params)
    # the loader: frames of one batch must share a size, and the message names the paths
    root = str(tmp_path)
    _tree(root, {"a": 9}, (40, 48))
    _tree(root, {"b": 9}, (48, 40))
    loader = D.BatchLoader(D.ClipIndex(root, ["a", "b"]), 2, seed=0, lq_size=8, workers=0, device=None)
    with pytest.raises(ValueError, match=r"share a size.*a.0\.png.*40 x 48"):
        loader.build(0)


def test_abi_rejects_before_any_launch(stif):
    """STIF_E_INVALID is returned before a launch, so the checks run without a GPU."""
    lib = stif._lib.lib()
    buf = (C.c_char * 64)()
    a = C.addressof(buf)

    def call(src=a, off=a, stride=a, out=a, n=1, G=8, o=4, w=a, idx=a, P=4, s0=2, flags=0):
        return lib.stif_build_batch(src, off, stride, out, n, G, o, w, idx, P, s0, flags, None)

    E = stif._lib.E_INVALID
    for kw in ({"src": None}, {"off": None}, {"stride": None}, {"out": None}, {"w": None}, {"idx": None},
               {"n": 0}, {"G": 0}, {"o": 0}, {"P": 0}, {"s0": 9}, {"flags": 8}, {"flags": 1 << 31}):
        assert call(**kw) == E, kw
        assert b"stif_build_batch" in lib.stif_last_error()


def test_header_and_binding_declare_the_builder(stif):
    hdr = open(os.path.join(REPO, "include", "stif.h")).read()
    assert re.search(r"^int\s+stif_build_batch\s*\(", hdr, re.M)
    assert "stif_build_batch" in stif._lib.EXPORTS
    assert (stif._lib.BATCH_HFLIP, stif._lib.BATCH_VFLIP, stif._lib.BATCH_ROT90) == (1, 2, 4)


def test_loader_is_a_pure_function_of_seed_and_index(D, tmp_path):
    from PIL import Image
    root = str(tmp_path)
    rng = np.random.RandomState(0)
    for v in ("u", "v"):
        os.makedirs(os.path.join(root, v))
        for k in range(11):
            Image.fromarray(rng.randint(0, 256, (40, 48, 3)).astype(np.uint8)).save(os.path.join(root, v, f"{k}.png"))
    index = D.ClipIndex(root, ["u", "v"])
    assert len(index) == 6

    def take(n, **kw):
        it = iter(D.BatchLoader(index, 2, seed=7, lq_size=8, device=None, **kw))
        out = [next(it) for _ in range(n)]
        it.close()
        return out

    a, b = take(5, workers=0), take(5, workers=3)
    for x, y in zip(a, b):
        assert np.array_equal(x["LQs"].numpy(), y["LQs"].numpy()) and np.array_equal(x["GT"].numpy(), y["GT"].numpy())
        assert x["shape"] == y["shape"] and all(np.array_equal(s, t) for s, t in zip(x["time"], y["time"]))
    # a loader started at batch 3 yields batch 3, and batch i is build_batch_host of the planned files and draws
    loader = D.BatchLoader(index, 2, seed=7, lq_size=8, workers=0, device=None, start=3)
    c = next(iter(loader))
    assert np.array_equal(c["GT"].numpy(), a[3]["GT"].numpy())
    paths, times, params = loader.plan(3)
    assert params == D.draw_collate_params(D.stream_rng(7, "batch", 3), 40, 48, 8)
    frames = [[np.asarray(Image.open(p).convert("RGB"))[:, :, ::-1] for p in item] for item in paths]
    ref = D.build_batch_host(frames, params, times)
    assert np.array_equal(ref["LQs"].numpy(), c["LQs"].numpy()) and np.array_equal(ref["GT"].numpy(), c["GT"].numpy())
    # two epochs of 3 batches each: every window is used once per epoch, in another order
    used = [[p[0] for p in loader.plan(i)[0]] for i in range(6)]
    assert sorted(sum(used[:3], [])) == sorted(sum(used[3:], [])) == sorted(w[0] for w in index.inputs)
    assert used[:3] != used[3:]


def test_training_script_names_the_criteria_it_does_not_build(stif):
    import importlib.util
    spec = importlib.util.spec_from_file_location("stif_tools_train", os.path.join(REPO, "tools", "train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert isinstance(mod.make_criterion(stif.train, {"pixel_criterion": "cb"}), stif.train.TimesLoss)
    for kind in ("l1", "l2", "lp"):
        with pytest.raises(NotImplementedError, match=f"pixel_criterion.*{kind}"):
            mod.make_criterion(stif.train, {"pixel_criterion": kind})
