"""Training batches on the GPU: stif_build_batch (csrc/resample.hip), data.build_batch, data.BatchLoader and
tools/train.py.

Engine against engine is bit for bit: the builder before augmentation is video.resize_frames of the crop (the same
fmaf order), so its output equals resize_frames + torch flips / transposes exactly; loader against build_batch and
run against run likewise.  Against the numpy restatement and the recorded reference the bound is
data_cases.bound: (2 P + 4) 2^-24 1.5 from the case's own tap count.  The shapes are the smallest at which the
kernel can go wrong -- lq_size 16 (LQ 8 x 8), G = 32 / 37 / 63, GT 16 / 19 (odd tails) / 32, crops at the frame's
corners -- plus the recorded 720 x 1280 case."""
import ctypes as C
import functools
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import data_cases as DC

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = ((70, 90), (90, 70))
DS = (2.0, 2.37, 3.99)                  # G = 32, 37, 63; GT 16, 19, 32
TIMES = [[0.0, 0.5, 1.0], [0.125, 0.25, 0.875]]


@pytest.fixture(scope="module")
def D(stif):
    return stif.data


@functools.lru_cache(maxsize=None)
def small_frames():
    rng = np.random.RandomState(11)
    host = [[rng.randint(0, 256, s + (3,)).astype(np.uint8) for _ in range(5)] for s in SIZES]
    return host, [[torch.from_numpy(f).cuda() for f in item] for item in host]


def positions(G):
    """(x, y) draws that put the crop at the four frame corners and in the interior (x: short side, y: long side)."""
    mx, my = 70 - G, 90 - G
    return [(0, 0), (0, my), (mx, 0), (mx, my), (mx // 2, my // 3 + 1)]


@functools.lru_cache(maxsize=None)
def resized_crops(stif, d, x, y):
    """video.resize_frames of every crop, before augmentation: (LQ [2, 2, 3, l, l], GT [2, 3, 3, g, g])."""
    p = stif.data.CollateParams(d, stif.data.resize_geometry(16, d).G, x, y, False, False, False, 16)
    geo = p.geometry
    _, dev = small_frames()
    lq, gt = [], []
    for item in dev:
        r, c = p.crop_origin(*item[0].shape[:2])
        crops = torch.stack([f[r:r + p.G, c:c + p.G] for f in item]).contiguous()
        lq.append(stif.video.resize_frames(crops[:2], geo.lq_scale))
        gt.append(stif.video.resize_frames(crops[2:], geo.gt_scale))
    return torch.stack(lq), torch.stack(gt)


def augment(t, flags):
    """augment_a2 on [..., H, W] planes with torch: flip W, flip H, then transpose."""
    if flags & 1:
        t = t.flip(-1)
    if flags & 2:
        t = t.flip(-2)
    if flags & 4:
        t = t.transpose(-1, -2)
    return t.contiguous()


@pytest.mark.parametrize("flags", range(8))
@pytest.mark.parametrize("d", DS)
def test_builder_is_resize_frames_plus_augmentation_bit_for_bit(stif, D, d, flags):
    host, dev = small_frames()
    G = D.resize_geometry(16, d).G
    for x, y in positions(G):
        p = D.CollateParams(d, G, x, y, bool(flags & 1), bool(flags & 2), bool(flags & 4), 16)
        assert p.flags == flags
        got = D.build_batch(dev, p, "cuda", TIMES)
        lq, gt = resized_crops(stif, d, x, y)
        assert got["shape"] == tuple(gt.shape[-2:]) == (-(-G // 2),) * 2 and tuple(got["LQs"].shape) == (2, 2, 3, 8, 8)
        assert torch.equal(got["LQs"], augment(lq, flags)), (d, flags, x, y)
        assert torch.equal(got["GT"], augment(gt, flags)), (d, flags, x, y)
        assert [t.cpu().flatten().tolist() for t in got["time"]] == [[0.0, 0.125], [0.5, 0.25], [1.0, 0.875]]
        assert all(tuple(t.shape) == (2, 1) and t.is_cuda for t in got["time"])
        ref = D.build_batch_host(host, p, TIMES)
        tol_lq, tol_gt = DC.bound(*DC.taps(stif, p))
        e_lq = float((got["LQs"].cpu() - ref["LQs"]).abs().max())
        e_gt = float((got["GT"].cpu() - ref["GT"]).abs().max())
        print(f"d {d} flags {flags} at ({x}, {y}): |LQ - host| {e_lq:.3e} (bound {tol_lq:.3e}), "
              f"|GT - host| {e_gt:.3e} (bound {tol_gt:.3e})")
        assert e_lq <= tol_lq and e_gt <= tol_gt
    # host frames (staged crops) and device frames (read in place) give the same bytes
    again = D.build_batch(host, p, "cuda", TIMES)
    assert torch.equal(again["LQs"], got["LQs"]) and torch.equal(again["GT"], got["GT"])


def test_no_byte_outside_the_crops_matters(D):
    """The symmetric padding mirrors at the crop's edge: whatever surrounds the crop, the batch is the same."""
    host, _ = small_frames()
    for d, (x, y) in ((2.37, (16, 20)), (3.99, (7, 0)), (2.0, (0, 58))):
        G = D.resize_geometry(16, d).G
        p = D.CollateParams(d, G, x, y, True, False, True, 16)
        outs = []
        for fill in (0, 255):
            frames = []
            for item in host:
                r, c = p.crop_origin(*item[0].shape[:2])
                new = []
                for f in item:
                    g = np.full_like(f, fill)
                    g[r:r + G, c:c + G] = f[r:r + G, c:c + G]
                    new.append(torch.from_numpy(g).cuda())
                frames.append(new)
            outs.append(D.build_batch(frames, p, "cuda"))
        assert torch.equal(outs[0]["LQs"], outs[1]["LQs"]) and torch.equal(outs[0]["GT"], outs[1]["GT"])
        assert float(outs[0]["GT"].std()) > 0.01


def _abi(stif, src, off, stride, out, n, G, o, w, idx, P, s0, flags):
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    stif._lib.check(stif._lib.lib().stif_build_batch(src.data_ptr(), off.data_ptr(), stride.data_ptr(), out.data_ptr(),
                                                     n, G, o, w.data_ptr(), idx.data_ptr(), P, s0, flags, st),
                    "stif_build_batch")


def test_guard_words_and_strided_source(stif, D):
    """Nothing is written outside [n][3][o][o], and a frame inside a wider buffer (row_stride > 3 W) gives the result
    of its packed copy."""
    host, dev = small_frames()
    d, flags = 2.37, 6
    p = D.CollateParams(d, 37, 30, 41, False, True, True, 16)
    geo = p.geometry
    base = D.build_batch(dev, p, "cuda")
    wide = []
    for item in host:
        new = []
        for f in item:
            H, W = f.shape[:2]
            buf = torch.full((H, W + 13, 3), 77, dtype=torch.uint8, device="cuda")
            buf[:, 5:5 + W] = torch.from_numpy(f).cuda()
            view = buf[:, 5:5 + W]
            assert view.stride(0) == 3 * (W + 13) > 3 * W
            new.append(view)
        wide.append(new)
    got = D.build_batch(wide, p, "cuda")
    assert torch.equal(got["LQs"], base["LQs"]) and torch.equal(got["GT"], base["GT"])
    # the ABI on output buffers with guard words either side
    GUARD, word = 64, -123456.5
    crops = torch.stack([f[p.crop_origin(*f.shape[:2])[0]:, p.crop_origin(*f.shape[:2])[1]:][:37, :37]
                         for item in dev for f in item]).contiguous()
    for o, scale, sel, want in ((geo.lq, geo.lq_scale, [0, 1, 5, 6], base["LQs"]),
                                (geo.gt, geo.gt_scale, [2, 3, 4, 7, 8, 9], base["GT"])):
        w, idx, s0 = stif.video.resize_tables(37, o, scale)
        n = len(sel)
        buf = torch.full((2 * GUARD + n * 3 * o * o,), word, device="cuda")
        out = buf[GUARD:GUARD + n * 3 * o * o]
        off = torch.tensor([k * 37 * 37 * 3 for k in sel], dtype=torch.int64, device="cuda")
        stride = torch.full((n,), 3 * 37, dtype=torch.int64, device="cuda")
        _abi(stif, crops, off, stride, out, n, 37, o, torch.from_numpy(w).cuda(), torch.from_numpy(idx).cuda(),
             w.shape[1], s0, flags)
        assert torch.equal(out.view(want.shape), want)
        assert bool((buf[:GUARD] == word).all()) and bool((buf[-GUARD:] == word).all())


def test_tables_wider_than_the_staged_window(stif):
    """A hand-made table whose taps jump across the whole padded crop does not fit the window the launch sizes from
    G / o: such tiles take the direct path, with the same sums.  s0 = G is the widest padding accepted."""
    G, o, P, s0, n = 40, 8, 4, 40, 2
    rng = np.random.RandomState(4)
    idx = np.array([0, 116, 3, 77, 116, 0, 41, 90], np.int32)            # padded domain [0, 120)
    w = rng.rand(o, P).astype(np.float32)
    w /= w.sum(1, keepdims=True)
    crops = rng.randint(0, 256, (n, G, G, 3)).astype(np.uint8)
    k = idx[:, None].astype(np.int64) + np.arange(P)[None, :] - s0
    src = np.where(k < 0, -k - 1, np.where(k >= G, 2 * G - 1 - k, k))
    assert src.min() >= 0 and src.max() < G
    wd = w.astype(np.float64)
    h = np.einsum("ip,nipxc->nixc", wd, crops.astype(np.float64)[:, src])
    ref = np.einsum("jp,nijpc->nijc", wd, h[:, :, src]) / 255.0           # [n, o, o, 3] BGR
    flags = 5
    ref = ref[:, :, ::-1].transpose(0, 2, 1, 3)[..., ::-1].transpose(0, 3, 1, 2)
    out = torch.full((n, 3, o, o), float("nan"), device="cuda")
    off = torch.tensor([0, G * G * 3], dtype=torch.int64, device="cuda")
    stride = torch.full((n,), 3 * G, dtype=torch.int64, device="cuda")
    _abi(stif, torch.from_numpy(crops).cuda(), off, stride, out, n, G, o, torch.from_numpy(w).cuda(),
         torch.from_numpy(idx).cuda(), P, s0, flags)
    err = float(np.abs(out.cpu().numpy() - ref).max())
    tol = (2 * P + 4) * 2.0 ** -24 * 1.5
    print(f"direct path: max|kernel - fp64| = {err:.3e} (bound {tol:.3e})")
    assert err <= tol


def test_recorded_reference_case_at_full_size(stif, D):
    """Seed 1 of the recorded collate: G = 145 out of 720 x 1280 and 1280 x 720 frames on the device."""
    p = DC.params_of(D, 1)
    assert p.G == 145
    frames = [[torch.from_numpy(f).cuda() for f in item] for item in DC.reference_frames()]
    got = D.build_batch(frames, p, "cuda", DC.TIMES)
    tol_lq, tol_gt = DC.bound(*DC.taps(stif, p))
    DC.check_against_recorded({"LQs": got["LQs"].cpu(), "GT": got["GT"].cpu(), "shape": got["shape"],
                               "time": [t.cpu() for t in got["time"]]}, 1, tol_lq, tol_gt)


@pytest.fixture(scope="module")
def footage(tmp_path_factory):
    """2 videos x 11 frames of 72 x 88, PNGs written with PIL."""
    from PIL import Image
    root = str(tmp_path_factory.mktemp("footage"))
    rng = np.random.RandomState(21)
    for v in ("clip_a", "clip_b"):
        os.makedirs(os.path.join(root, v))
        for k in range(11):
            Image.fromarray(rng.randint(0, 256, (72, 88, 3)).astype(np.uint8)).save(os.path.join(root, v, f"{k}.png"))
    return root


def _same(a, b):
    return (torch.equal(a["LQs"], b["LQs"]) and torch.equal(a["GT"], b["GT"]) and a["shape"] == b["shape"]
            and all(torch.equal(s, t) for s, t in zip(a["time"], b["time"])))


def test_batch_loader(D, footage):
    from PIL import Image
    index = D.ClipIndex(footage, ["clip_a", "clip_b"])
    assert len(index) == 6

    def take(n, **kw):
        it = iter(D.BatchLoader(index, 2, seed=5, lq_size=16, **kw))
        out = list(itertools.islice(it, n))
        it.close()
        torch.cuda.synchronize()
        return out

    a, b, c = take(4, workers=3), take(4, workers=3), take(4, workers=0)
    assert all(_same(x, y) for x, y in zip(a, b)), "two loaders with the same seed"
    assert all(_same(x, y) for x, y in zip(a, c)), "workers=3 against workers=0"
    loader = D.BatchLoader(index, 2, seed=5, lq_size=16, workers=0)
    for i, batch in enumerate(a):
        paths, times, params = loader.plan(i)
        assert params == D.draw_collate_params(D.stream_rng(5, "batch", i), 72, 88, 16)
        frames = [[np.ascontiguousarray(np.asarray(Image.open(q).convert("RGB"))[:, :, ::-1]) for q in item]
                  for item in paths]
        assert _same(batch, D.build_batch(frames, params, "cuda", times)), i
        assert tuple(batch["LQs"].shape) == (2, 2, 3, 8, 8) and batch["GT"].shape[-1] == batch["shape"][1]


OPT = """
name: tiny
model: VideoSR_base
distortion: sr
scale: 4
datasets:
  train:
    name: Adobe_a
    mode: Adobe_a
    dataroot_GT: {root}
    video_list: {root}/list.txt
    n_workers: 2
    batch_size: 2
    lq_size: 16
network_G:
  which_model_G: LIIF
  nf: 64
  nframes: 7
  groups: 8
  front_RBs: 1
  back_RBs: 1
path:
  pretrain_model_G: ~
  strict_load: true
  resume_state: {resume}
  models: {out}/models
  training_state: {out}/state
train:
  lr_G: !!float 2e-5
  lr_scheme: CosineAnnealingLR_Restart
  beta1: 0.9
  beta2: 0.99
  niter: 3
  warmup_iter: -1
  T_period: [10, 10]
  restarts: [10]
  restart_weights: [1]
  eta_min: !!float 1e-7
  pixel_criterion: cb
  pixel_weight: 1.0
  manual_seed: 0
logger:
  print_freq: 1
  save_checkpoint_freq: 1
"""


def _train(tmp, footage, out, resume="~"):
    with open(os.path.join(footage, "list.txt"), "w") as f:
        f.write("clip_a\nclip_b\n")
    yml = os.path.join(tmp, f"{os.path.basename(out)}_{'r' if resume != '~' else 'f'}.yml")
    with open(yml, "w") as f:
        f.write(OPT.format(root=footage, out=out, resume=resume))
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "train.py"), "--opt", yml, "--deterministic"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout


def test_training_script_checkpoints_and_resumes(stif, footage, tmp_path):
    import re
    tmp = str(tmp_path)
    one, two = os.path.join(tmp, "one"), os.path.join(tmp, "two")
    log = _train(tmp, footage, one)
    losses = [float(v) for v in re.findall(r"l_pix: (\S+)", log)]
    print(log)
    assert len(losses) == 3 and all(np.isfinite(v) and v > 0 for v in losses)
    load = lambda d, name: torch.load(os.path.join(d, "models", name), map_location="cpu", weights_only=True)
    sd = load(one, "3_G.pth")
    # the reference's 442 keys less the 4 keys of each residual block this tiny model leaves out (5 + 40 -> 1 + 1)
    assert len(sd) == 442 - 4 * (4 + 39) and all(not v.is_cuda for v in sd.values())
    spec = [k for k in stif.weights.state_dict_spec()
            if not any(k.startswith(f"{trunk}.{i}.") for trunk in ("feature_extraction", "recon_trunk")
                       for i in range(1, 40))]
    assert list(sd) == spec
    stif.train.LunaTokis(1, 1).load_state_dict(sd, strict=True)
    assert not torch.equal(sd["conv_first.weight"], load(one, "1_G.pth")["conv_first.weight"])
    state = torch.load(os.path.join(one, "state", "3.state"), map_location="cpu", weights_only=False)
    assert set(state) == {"epoch", "iter", "schedulers", "optimizers", "seed"} and state["iter"] == 3
    # a second run: the same bytes
    _train(tmp, footage, two)
    sd2 = load(two, "3_G.pth")
    assert list(sd2) == list(sd) and all(torch.equal(sd[k], sd2[k]) for k in sd)
    # resumed from iteration 2 of the second run: the same iteration 3, the same lr
    os.remove(os.path.join(two, "models", "3_G.pth"))
    os.remove(os.path.join(two, "state", "3.state"))
    log3 = _train(tmp, footage, two, resume=os.path.join(two, "state", "2.state"))
    assert "resuming training from epoch" in log3 and len(re.findall(r"l_pix: (\S+)", log3)) == 1
    sd3 = load(two, "3_G.pth")
    assert all(torch.equal(sd[k], sd3[k]) for k in sd)
    state3 = torch.load(os.path.join(two, "state", "3.state"), map_location="cpu", weights_only=False)
    lr = lambda s: [g["lr"] for g in s["optimizers"][0]["param_groups"]]
    assert lr(state3) == lr(state) and state3["iter"] == 3 and state3["seed"] == state["seed"]
    assert float(re.findall(r"l_pix: (\S+)", log3)[0]) == losses[2]
