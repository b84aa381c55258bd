"""Streaming a video through the engine on the GPU: render_stream's frames are bit-identical to run_sequence's
whatever the chunking and the schedule, render_y4m equals the three stages composed by hand, and streaming holds
less memory than the one-window driver."""
import gc
from fractions import Fraction

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

H, W = 14, 18                     # padded to 16 x 20; outputs 56 x 72 of the padded frame's 64 x 80 grid
_MODELS, _REF = {}, {}


def model(stif, sd, mode):
    if mode not in _MODELS:
        m = stif.LunaTokis(64, 6, 8, 5, 40, mfma=mode)
        m.load_state_dict(sd, strict=True)
        _MODELS[mode] = m
    return _MODELS[mode]


def clip(n, h=H, w=W):
    return torch.rand(n, 3, h, w, generator=torch.Generator().manual_seed(2024))[:n].cuda()


def reference(stif, sd, mode, n, pair, t):
    """crop of run_sequence(model, clip, times=[t])[pair][0], one run_sequence per (mode, clip, t)"""
    key = (mode, n, float(t))
    if key not in _REF:
        _REF[key] = stif.video.run_sequence(model(stif, sd, mode), clip(n), times=[float(t)])
    return _REF[key][pair][0][:, :4 * H, :4 * W]


def check_identity(stif, sd, mode, n, fi, fo, chunk):
    V = stif.video
    sched = list(V.frame_schedule(fi, fo, n))
    outs = list(V.render_stream(model(stif, sd, mode), iter(clip(n)), fi, fo, scale=4, chunk_pairs=chunk))
    assert len(outs) == len(sched)
    for o, (pair, t) in zip(outs, sched):
        assert tuple(o.shape) == (3, 4 * H, 4 * W) and o.is_cuda
        assert torch.equal(o, reference(stif, sd, mode, n, pair, t)), (pair, t)


@pytest.mark.parametrize("mode, chunk", [("f16x3", 1), ("f16x3", 3), ("f16x3", 8), ("f32", 3)])
def test_stream_is_bit_identical_to_run_sequence(stif, sd, mode, chunk):
    check_identity(stif, sd, mode, 5, 25, 50, chunk)


@pytest.mark.parametrize("chunk", [2, 8])
def test_variable_schedule(stif, sd, chunk):
    """fps ratio 5/2 over 4 frames: 3, 2, 3 outputs per pair, each at its own time (the last input instant, 7.5
    output periods in, is not an output instant)"""
    sched = list(stif.video.frame_schedule(2, 5, 4))
    assert [sum(1 for p, _ in sched if p == q) for q in range(3)] == [3, 2, 3]
    check_identity(stif, sd, "f16x3", 4, 2, 5, chunk)


def test_render_y4m_equals_the_stages_composed_by_hand(stif, sd, tmp_path):
    y4m, ops, V = stif.y4m, stif.ops, stif.video
    m = model(stif, sd, "f16x3")
    fmt = y4m.YuvFormat(W, H, "420jpeg", 8, "bt601", False)
    payloads = np.random.default_rng(8).integers(0, 256, (5, fmt.frame_bytes), dtype=np.uint8)
    src, dst = tmp_path / "in.y4m", tmp_path / "out.y4m"
    with y4m.Y4MWriter(str(src), fmt, Fraction(25)) as wr:
        for p in payloads:
            wr.write(p)
    assert V.render_y4m(m, str(src), str(dst), multiplier=2, scale=4, chunk_pairs=3) == (5, 9)
    with y4m.Y4MReader(str(dst)) as r:
        got = list(r)
        assert open(dst, "rb").readline() == b"YUV4MPEG2 W72 H56 F50:1 Ip C420jpeg\n"
        assert (r.fmt.width, r.fmt.height, r.fps, r.fmt.chroma) == (72, 56, Fraction(50), "420jpeg")
    assert len(got) == 9
    rgb = ops.yuv_to_rgb(torch.from_numpy(payloads).cuda(), fmt)
    fmt_out = fmt.resized(72, 56)
    want = [ops.rgb_to_yuv(o[None], fmt_out)[0].cpu().numpy()
            for o in V.render_stream(m, iter(rgb), 25, 50, scale=4, chunk_pairs=3)]
    assert len(want) == 9 and all(np.array_equal(a, b) for a, b in zip(got, want))
    assert len({a.tobytes() for a in got}) == 9                      # nine different frames, not one repeated


def test_streaming_holds_less_memory_than_one_window(stif, sd):
    """9 frames of 16 x 20 at x8 the frame rate: render_stream(chunk_pairs=2) holds 2 pairs where run_sequence
    holds 8, so its peak above the level before the call is strictly lower."""
    V = stif.video
    m = model(stif, sd, "f16x3")
    frames = clip(9, 16, 20)

    def streamed():
        n = 0
        for o in V.render_stream(m, iter(frames), 25, 200, scale=4, chunk_pairs=2):
            n += 1
            del o
        return n

    def windowed():
        return sum(len(row) for row in V.run_sequence(m, frames))

    peaks = {}
    for name, fn in (("stream", streamed), ("window", windowed)):
        fn()                                                          # tables and constant maps exist after this
        gc.collect()
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        count = fn()
        torch.cuda.synchronize()
        peaks[name] = torch.cuda.max_memory_allocated() - base
        assert count == (65 if name == "stream" else 64)             # the stream adds the closing t = 1 frame
        gc.collect()
    print("peak bytes above the level before the call:", peaks)
    assert peaks["stream"] < peaks["window"]
