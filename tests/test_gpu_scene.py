"""Scene cuts on the GPU: ops.scene_sad against a numpy restatement of its luma to the last bit (shapes, strides,
load paths, out-of-range values, 64-bit totals, rejected arguments), and the streaming renderer with the detector
on: the cut of a synthetic clip is found whatever the chunking, its pair repeats the degenerate-pair rendering of
a real frame bit for bit, every other pair is untouched, and render_y4m equals the stages composed by hand."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

F = np.float32
H, W = 14, 18                     # padded to 16 x 20; outputs 56 x 72 of the padded frame's 64 x 80 grid
_MODELS, _REF = {}, {}


# ----------------------------------------------------------------------------- the restatement
def luma8(v):
    """8-bit luma of fp32 RGB planes [..., 3, h, w], in np.float32 operations in the kernel's order"""
    v = np.asarray(v, F)
    c = np.fmin(np.fmax(v, F(0)), F(1))                           # fmax / fmin drop a NaN operand, like fmaxf / fminf
    y = (F(0.299) * c[..., 0, :, :] + F(0.587) * c[..., 1, :, :]) + F(0.114) * c[..., 2, :, :]
    assert y.dtype == F
    return np.minimum(np.rint(y * F(255)).astype(np.int64), 255)


def sad_ref(frames, h=None, w=None):
    q = luma8(frames.detach().cpu().numpy()[:, :, :h, :w])
    return torch.from_numpy(np.abs(q[1:] - q[:-1]).sum((1, 2)))


def check(stif, frames, h=None, w=None):
    got = stif.ops.scene_sad(frames, h, w)
    assert got.dtype == torch.int64 and got.is_cuda and tuple(got.shape) == (frames.shape[0] - 1,)
    assert torch.equal(got.cpu(), sad_ref(frames, h, w)), (got.cpu().tolist(), sad_ref(frames, h, w).tolist())
    return got


def rand(n, h, w, seed=0):
    return torch.rand(n, 3, h, w, generator=torch.Generator().manual_seed(seed)).cuda()


# ----------------------------------------------------------------------------- ops.scene_sad
@pytest.mark.parametrize("n", [2, 9])
@pytest.mark.parametrize("h, w", [(1, 1), (14, 18), (16, 20), (70, 131), (5, 1030)])
def test_sad_equals_the_restatement(stif, n, h, w):
    """1 x 1; widths that are and are not a multiple of 4 (18, 131: a ragged right edge on the scalar loads beside
    vector groups, or all scalar when the odd pitch breaks the alignment); 70 x 131 and 5 x 1030 span several
    workgroups with a ragged last one"""
    got = check(stif, rand(n, h, w, seed=n * 1000 + h))
    assert int(got.min()) > 0 or (h, w) == (1, 1)


def test_more_pairs_than_one_walk(stif):
    """n = 20: three walks of 8, 8 and 3 pairs, the frames between them read by both"""
    check(stif, rand(20, 14, 18, seed=7))


@pytest.mark.parametrize("h, w, hb, wb", [(14, 18, 16, 20), (70, 131, 72, 132)])
def test_rectangle_inside_a_padded_buffer(stif, h, w, hb, wb):
    """the h x w rectangle of a padded buffer whose padding holds garbage that must not count: vector loads (the
    pitch is a multiple of 4) with a ragged right edge on scalar ones"""
    buf = rand(9, hb, wb, seed=3)
    want = sad_ref(buf, h, w)
    buf[:, :, h:, :] = 1e30
    buf[:, :, :, w:] = float("nan")
    got = check(stif, buf, h, w)
    assert torch.equal(got.cpu(), want)
    assert torch.equal(stif.ops.scene_sad(buf[:, :, :h, :w]), got)        # the same view, passed as a crop


def test_scalar_path_of_a_misaligned_view(stif):
    """a view whose base pointer is off by one float: same values, scalar loads"""
    n, h, w = 9, 16, 20
    flat = torch.empty(n * 3 * h * w + 1, device="cuda")
    flat[1:] = rand(n, h, w, seed=4).reshape(-1)
    view = flat[1:].view(n, 3, h, w)
    assert view.data_ptr() % 16 == 4
    got = check(stif, view)
    assert torch.equal(got, stif.ops.scene_sad(view.clone()))             # the aligned copy takes the vector path


def test_out_of_range_values_and_nan(stif):
    x = (rand(9, 14, 18, seed=5) * 3.0 - 1.0)                             # a third below 0, a third above 1
    x[::2, 1, ::3, ::5] = float("nan")
    x[1, :, 0, 0] = float("inf")
    x[2, :, 0, 0] = float("-inf")
    got = check(stif, x)
    assert int(got.min()) > 0
    ones = torch.ones(2, 3, 4, 8, device="cuda")
    ones[1] = float("nan")                                                # NaN counts as 0: a white-to-black pair
    assert stif.ops.scene_sad(ones).tolist() == [255 * 32]


def test_repeated_calls_give_equal_bits(stif):
    x = rand(9, 70, 131, seed=6)
    a, b = stif.ops.scene_sad(x), stif.ops.scene_sad(x)
    assert torch.equal(a, b)


def test_8k_pair_sums_above_32_bits(stif):
    x = torch.zeros(2, 3, 4320, 7680, device="cuda")
    x[1] = 1.0
    got = stif.ops.scene_sad(x)
    del x
    assert got.tolist() == [8_460_288_000] and 8_460_288_000 == 255 * 4320 * 7680 > 2 ** 32


def test_cpu_tensor_raises(stif):
    with pytest.raises(ValueError):
        stif.ops.scene_sad(torch.zeros(2, 3, 4, 4))
    with pytest.raises(ValueError):
        stif.ops.scene_sad(torch.zeros(1, 3, 4, 4, device="cuda"))
    with pytest.raises(ValueError):
        stif.ops.scene_sad(torch.zeros(2, 3, 4, 4, device="cuda"), 5, 4)


def test_invalid_arguments_launch_nothing(stif):
    L = stif._lib
    lib = L.lib()
    n, h, w = 3, 6, 8
    x = rand(n, h, w)
    sad = torch.full((n,), -7, dtype=torch.int64, device="cuda")          # one spare element for the misaligned case
    need = lib.stif_scene_workspace_size(n, h, w)
    assert need > 0 and need % 8 == 0
    assert [lib.stif_scene_workspace_size(*a) for a in ((1, h, w), (n, 0, w), (n, h, 0))] == [0, 0, 0]
    ws = torch.zeros(need // 8 + 1, dtype=torch.int64, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    X, S, WS = x.data_ptr(), sad.data_ptr(), ws.data_ptr()
    dense = (3 * h * w, h * w, w)

    def call(rgb=X, strides=(0, 0, 0), dims=(n, h, w), out=S, wsp=WS, wsb=need):
        return lib.stif_scene_sad(rgb, *strides, *dims, out, wsp, wsb, st)

    cases = {
        "rgb null": (dict(rgb=None), L.E_INVALID),
        "sad null": (dict(out=None), L.E_INVALID),
        "n < 2": (dict(dims=(1, h, w)), L.E_INVALID),
        "H < 1": (dict(dims=(n, 0, w)), L.E_INVALID),
        "W < 1": (dict(dims=(n, h, 0)), L.E_INVALID),
        "pitch below W": (dict(strides=(3 * h * w, h * w, w - 1)), L.E_INVALID),
        "negative pitch": (dict(strides=(3 * h * w, h * w, -w)), L.E_INVALID),
        "overlapping planes": (dict(strides=(3 * h * w, h * w - 1, w)), L.E_INVALID),
        "overlapping items": (dict(strides=(3 * h * w - 1, h * w, w)), L.E_INVALID),
        "misaligned sad": (dict(out=S + 4), L.E_INVALID),
        "misaligned workspace": (dict(wsp=WS + 4), L.E_INVALID),
        "workspace null": (dict(wsp=None), L.E_WORKSPACE),
        "workspace short": (dict(wsb=need - 1), L.E_WORKSPACE),
    }
    for name, (kw, code) in cases.items():
        assert call(**kw) == code, name
        assert b"stif_scene_sad" in lib.stif_last_error(), name
    torch.cuda.synchronize()
    assert sad.tolist() == [-7] * n and int(ws.abs().sum()) == 0           # nothing ran
    assert call(strides=dense) == 0 and call() == 0                        # and the same call, valid, does
    assert torch.equal(sad[:n - 1].cpu(), sad_ref(x)) and int(sad[n - 1]) == -7


# ----------------------------------------------------------------------------- the renderer with the detector on
def model(stif, sd, mode):
    if mode not in _MODELS:
        m = stif.LunaTokis(64, 6, 8, 5, 40, mfma=mode)
        m.load_state_dict(sd, strict=True)
        _MODELS[mode] = m
    return _MODELS[mode]


def detection_clip():
    """7 frames: three of one random picture, four of another, each with its own +-2 % noise -- a cut at pair 2"""
    g = torch.Generator().manual_seed(2024)
    A, B = torch.rand(3, H, W, generator=g), torch.rand(3, H, W, generator=g)
    noise = torch.rand(7, 3, H, W, generator=g)
    return torch.stack([(A if i < 3 else B) + 0.04 * (noise[i] - 0.5) for i in range(7)])


def test_detection_clip_numbers(stif):
    """the clip's SADs and scores by the restatement: the cut scores twice the threshold 0.1, everything else a
    tenth of it; the device agrees to the last bit"""
    clip = detection_clip()
    sad = sad_ref(clip).tolist()
    scores, _ = stif.video.scene_scores(sad, H, W)
    print("SAD", sad, "scores", [round(s, 4) for s in scores])
    assert scores[2] > 0.2 and max(s for i, s in enumerate(scores) if i != 2) < 0.01
    assert sad == [604, 548, 13741, 543, 542, 542]                          # the issue's figures, as a cross-check
    assert torch.equal(stif.ops.scene_sad(clip.cuda()).cpu(), torch.tensor(sad))


def reference(stif, sd, mode, pair, t):
    """crop of run_sequence(model, detection clip, times=[t])[pair][0]"""
    key = (mode, float(t))
    if key not in _REF:
        _REF[key] = stif.video.run_sequence(model(stif, sd, mode), detection_clip().cuda(), times=[float(t)])
    return _REF[key][pair][0][:, :4 * H, :4 * W]


def held_reference(stif, sd, mode, f):
    """crop of the degenerate pair (f, f) at t = 0"""
    key = (mode, "held", f)
    if key not in _REF:
        fr = detection_clip()[f].cuda()
        _REF[key] = stif.video.run_sequence(model(stif, sd, mode), torch.stack([fr, fr]), times=[0.0])[0][0]
    return _REF[key][:, :4 * H, :4 * W]


@pytest.mark.parametrize("mode, chunk", [("f16x3", 1), ("f16x3", 3), ("f16x3", 8), ("f32", 3)])
def test_cut_is_held_and_the_rest_is_untouched(stif, sd, mode, chunk):
    V = stif.video
    cuts = []
    outs = list(V.render_stream(model(stif, sd, mode), iter(detection_clip().cuda()), 25, 50, scale=4,
                                chunk_pairs=chunk, scene_threshold=0.1, cuts=cuts))
    sched = list(V.frame_schedule(25, 50, 7))
    assert cuts == [2] and len(outs) == len(sched) == 13
    for o, (pair, t) in zip(outs, sched):
        assert tuple(o.shape) == (3, 4 * H, 4 * W) and o.is_cuda
        if pair == 2:
            f = 2 if t < Fraction(1, 2) else 3
            assert torch.equal(o, held_reference(stif, sd, mode, f)), (pair, t)
        else:
            assert torch.equal(o, reference(stif, sd, mode, pair, t)), (pair, t)
    assert not torch.equal(outs[4], outs[5])                               # frame 2 and frame 3: different pictures


def test_clip_without_a_cut_is_unchanged(stif, sd):
    """the 5-frame random clip of test_gpu_video_stream.py: nothing scores above 0.1, so the detector changes no
    frame"""
    V = stif.video
    m = model(stif, sd, "f16x3")
    clip = torch.rand(5, 3, H, W, generator=torch.Generator().manual_seed(2024)).cuda()
    scores, _ = V.scene_scores(sad_ref(clip).tolist(), H, W)
    assert max(scores) < 0.05
    cuts = []
    with_det = list(V.render_stream(m, iter(clip), 25, 50, chunk_pairs=3, scene_threshold=0.1, cuts=cuts))
    without = list(V.render_stream(m, iter(clip), 25, 50, chunk_pairs=3))
    assert cuts == [] and len(with_det) == len(without) == 9
    assert all(torch.equal(a, b) for a, b in zip(with_det, without))


@pytest.mark.parametrize("kw", [dict(hold_pairs=[2]), dict(scene_threshold=0.1)], ids=["hold_pairs", "threshold"])
def test_render_y4m_with_cuts_equals_the_stages_composed_by_hand(stif, sd, tmp_path, kw):
    y4m, ops, V = stif.y4m, stif.ops, stif.video
    m = model(stif, sd, "f16x3")
    fmt = y4m.YuvFormat(W, H, "420jpeg", 8, "bt601", False)
    payloads = ops.rgb_to_yuv(detection_clip().cuda(), fmt)
    src, dst = tmp_path / "in.y4m", tmp_path / "out.y4m"
    with y4m.Y4MWriter(str(src), fmt, Fraction(25)) as wr:
        for p in payloads.cpu().numpy():
            wr.write(p)
    rgb = ops.yuv_to_rgb(payloads, fmt)
    scores, _ = V.scene_scores(sad_ref(rgb).tolist(), H, W)                 # the cut survives the trip through YUV
    assert scores[2] > 0.15 and max(s for i, s in enumerate(scores) if i != 2) < 0.05
    cuts = []
    assert V.render_y4m(m, str(src), str(dst), multiplier=4, scale=4, chunk_pairs=3, cuts=cuts, **kw) == (7, 25)
    assert cuts == [2]
    with y4m.Y4MReader(str(dst)) as r:
        got = list(r)
    fmt_out = fmt.resized(4 * W, 4 * H)
    cuts2 = []
    want = [ops.rgb_to_yuv(o[None], fmt_out)[0].cpu().numpy()
            for o in V.render_stream(m, iter(rgb), 25, 100, scale=4, chunk_pairs=3, cuts=cuts2, **kw)]
    assert cuts2 == [2] and len(got) == len(want) == 25
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
    # pair 2 is outputs 8..11: two of frame 2, then two of frame 3
    assert np.array_equal(got[8], got[9]) and np.array_equal(got[10], got[11]) and not np.array_equal(got[9], got[10])
