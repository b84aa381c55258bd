"""Video I/O without a GPU: the YUV4MPEG2 reader / writer (header tags, rejected streams, non-seekable byte round
trips), the exact-rational frame schedule, and the streaming renderer's chunking logic on a recording fake model."""
import io
import weakref
from fractions import Fraction

import numpy as np
import pytest
import torch


class Pipe(io.BytesIO):
    """A byte stream that cannot seek or tell, like stdin / stdout of a pipe."""

    def seek(self, *a):
        raise io.UnsupportedOperation("seek")

    def tell(self):
        raise io.UnsupportedOperation("tell")

    def seekable(self):
        return False


def stream(header, nbytes, frames=1, frame_line=b"FRAME"):
    body = b"".join(frame_line + b"\n" + bytes((i + k) % 251 for k in range(nbytes)) for i in range(frames))
    return Pipe(header.encode() + b"\n" + body)


@pytest.fixture(scope="module")
def y4m(stif):
    import importlib
    return importlib.import_module(stif.__name__ + ".y4m")


# ----------------------------------------------------------------------------- reader / writer
@pytest.mark.parametrize("tag, sub, depth, nbytes", [
    ("420jpeg", (1, 1), 8, 13 * 11 + 2 * 7 * 6), ("420mpeg2", (1, 1), 8, 227), ("420paldv", (1, 1), 8, 227),
    ("420", (1, 1), 8, 227), ("422", (1, 0), 8, 13 * 11 + 2 * 7 * 11), ("444", (0, 0), 8, 3 * 13 * 11),
    ("420p10", (1, 1), 10, 454), ("422p12", (1, 0), 12, 2 * (143 + 154)), ("444p16", (0, 0), 16, 6 * 143),
    ("420p14", (1, 1), 14, 454)])
def test_header_c_tags(y4m, tag, sub, depth, nbytes):
    r = y4m.Y4MReader(stream(f"YUV4MPEG2 W13 H11 F30000:1001 Ip A1:1 C{tag}", nbytes, frames=2))
    f = r.fmt
    assert (f.width, f.height, f.sub_x, f.sub_y, f.depth) == (13, 11, *sub, depth)
    assert f.frame_bytes == nbytes and f.ctag == tag and not f.full_range
    assert r.fps == Fraction(30000, 1001) and r.aspect == "1:1" and r.interlace == "p"
    frames = list(r)
    assert len(frames) == 2 and all(x.dtype == np.uint8 and x.size == nbytes for x in frames)
    assert frames[1][0] == 1 and r.frames_read == 2
    y, u, v = f.planes(frames[0])
    assert y.shape == (11, 13) and u.shape == v.shape == f.chroma_size[::-1]
    assert y.dtype == (np.uint8 if depth == 8 else np.dtype("<u2"))


def test_header_defaults_frame_params_and_x_tags(y4m):
    r = y4m.Y4MReader(stream("YUV4MPEG2 W4 H2 F25:1 XYSCSS=420JPEG XCOLORRANGE=FULL XFOO=bar", 12, frames=2,
                             frame_line=b"FRAME Ip Xq=1"))
    assert r.fmt.chroma == "420" and r.fmt.depth == 8            # a missing C tag means 4:2:0
    assert r.fmt.full_range and r.range_tagged
    assert r.extra_tags == ["XYSCSS=420JPEG", "XFOO=bar"]        # kept, in order, for the writer
    assert len(list(r)) == 2                                     # FRAME lines with parameters are accepted
    r = y4m.Y4MReader(stream("YUV4MPEG2 W4 H2 F25:1 I? XCOLORRANGE=LIMITED", 12))
    assert not r.fmt.full_range and r.range_tagged and r.interlace == "?"


@pytest.mark.parametrize("header, word", [
    ("YUV4MPEG2 W4 H2 F25:1 It", "It"), ("YUV4MPEG2 W4 H2 F25:1 Ib", "Ib"), ("YUV4MPEG2 W4 H2 F25:1 Im", "Im"),
    ("YUV4MPEG2 W4 H2 F25:1 Cmono", "Cmono"), ("YUV4MPEG2 W4 H2 F25:1 C444alpha", "C444alpha"),
    ("YUV4MPEG2 W4 H2 F25:1 C411", "C411"), ("YUV4MPEG2 W4 H2 F25:1 C420p9", "C420p9"),
    ("YUV4MPEG2 W4 H2 F0:1", "F0:1"), ("YUV4MPEG2 W4 H2 Q7", "Q7"), ("YUV4MPEG W4 H2", "YUV4MPEG2")])
def test_rejected_headers_name_the_tag(y4m, header, word):
    with pytest.raises(ValueError, match=word.replace("?", r"\?")):
        y4m.Y4MReader(stream(header, 12))


def test_truncated_final_frame(y4m):
    s = stream("YUV4MPEG2 W4 H2 F25:1", 12, frames=2).getvalue()
    r = y4m.Y4MReader(Pipe(s[:-5]))
    assert r.read_frame() is not None
    with pytest.raises(ValueError, match="truncated FRAME 1"):
        r.read_frame()
    r = y4m.Y4MReader(Pipe(s + b"FRA"))                           # a cut FRAME line
    assert len([r.read_frame(), r.read_frame()]) == 2
    with pytest.raises(ValueError, match="truncated"):
        r.read_frame()
    r = y4m.Y4MReader(Pipe(s + b"JUNK\n"))
    r.read_frame(), r.read_frame()
    with pytest.raises(ValueError, match="FRAME line"):
        r.read_frame()


@pytest.mark.parametrize("w, h, chroma, depth", [(13, 11, "420jpeg", 8), (14, 9, "422", 10)])
def test_writer_reader_round_trip_without_seeking(y4m, w, h, chroma, depth):
    fmt = y4m.YuvFormat(w, h, chroma, depth, "bt709", True)
    cw, ch = fmt.chroma_size
    assert fmt.frame_bytes == (w * h + 2 * cw * ch) * (2 if depth > 8 else 1)
    rng = np.random.default_rng(5)
    payloads = [rng.integers(0, 256, fmt.frame_bytes, dtype=np.uint8) for _ in range(3)]
    out = Pipe()
    wr = y4m.Y4MWriter(out, fmt, Fraction(24000, 1001), extra_tags=["XFOO=bar"], aspect="1:1")
    wr.write(payloads[0])
    wr.write(payloads[1].tobytes())
    wr.write(payloads[2])
    wr.close()
    assert wr.frames_written == 3
    raw = out.getvalue()
    head = raw.split(b"\n", 1)[0].decode()
    assert head == f"YUV4MPEG2 W{w} H{h} F24000:1001 Ip A1:1 C{fmt.ctag} XCOLORRANGE=FULL XFOO=bar"
    assert len(raw) == len(head) + 1 + 3 * (6 + fmt.frame_bytes)
    r = y4m.Y4MReader(Pipe(raw), matrix="bt709")
    assert r.fmt == fmt and r.fps == Fraction(24000, 1001) and r.extra_tags == ["XFOO=bar"]
    got = list(r)
    assert len(got) == 3 and all(np.array_equal(a, b) for a, b in zip(got, payloads))
    with pytest.raises(ValueError, match="payload"):
        y4m.Y4MWriter(Pipe(), fmt, 25).write(payloads[0][:-1])


def test_matrix_auto_rule_and_header_propagation(y4m):
    assert [y4m.choose_matrix(w, h) for w, h in ((1279, 719), (1280, 2), (2, 720), (720, 576), (1920, 1080))] == \
        ["bt601", "bt709", "bt709", "bt601", "bt709"]
    for w, h, want in ((1280, 4, "bt709"), (720, 576, "bt601")):
        nb = w * h * 3 // 2
        assert y4m.Y4MReader(stream(f"YUV4MPEG2 W{w} H{h} F25:1", nb, frames=0)).fmt.matrix == want
        assert y4m.Y4MReader(stream(f"YUV4MPEG2 W{w} H{h} F25:1", nb, frames=0), matrix="bt601").fmt.matrix == "bt601"
    # the output format of a x4 render keeps the input's layout, depth, range and matrix, whatever its new size
    fmt = y4m.Y4MReader(stream("YUV4MPEG2 W640 H360 F25:1 C422p10 XCOLORRANGE=FULL", 4, frames=0)).fmt
    big = fmt.resized(2560, 1440)
    assert (big.width, big.height) == (2560, 1440)
    assert (big.chroma, big.depth, big.full_range, big.matrix) == ("422", 10, True, "bt601")


# ----------------------------------------------------------------------------- frame schedule
def count(n, fi, fo):
    return (n - 1) * Fraction(fo) / Fraction(fi) // 1 + 1


def test_schedule_times_eight_reproduces_the_harness(stif):
    V = stif.video
    n = 5
    s = list(V.frame_schedule(25, 200, n))
    want = [(p, Fraction(k, 8)) for p in range(n - 1) for k in range(8)] + [(n - 2, Fraction(1))]
    assert s == want and len(s) == count(n, 25, 200)
    assert [float(t) for p, t in s if p == 2 and t < 1] == V.HARNESS_TIMES


def test_schedule_24_to_60(stif):
    s = list(stif.video.frame_schedule(24, 60, 5))
    assert [sum(1 for p, _ in s if p == q) for q in range(4)] == [3, 2, 3, 3]       # 3, 2, 3, 2 and the final frame
    assert s[-1] == (3, Fraction(1)) and len(s) == count(5, 24, 60) == 11
    F = Fraction
    assert [t for _, t in s[:10]] == [F(0), F(2, 5), F(4, 5), F(1, 5), F(3, 5), F(0), F(2, 5), F(4, 5), F(1, 5), F(3, 5)]
    assert all(isinstance(t, Fraction) for _, t in s)


def test_schedule_ntsc_rates_and_downconversion(stif):
    V = stif.video
    a, b = Fraction(30000, 1001), Fraction(60000, 1001)
    s = list(V.frame_schedule(a, b, 4))
    assert s == [(0, 0), (0, Fraction(1, 2)), (1, 0), (1, Fraction(1, 2)), (2, 0), (2, Fraction(1, 2)), (2, 1)]
    assert len(s) == count(4, a, b)
    s = list(V.frame_schedule(60, 24, 8))                       # 2.5 input frames per output frame
    assert s == [(0, 0), (2, Fraction(1, 2)), (5, 0)] and len(s) == count(8, 60, 24)
    assert list(V.frame_schedule(60, 24, 6)) == [(0, 0), (2, Fraction(1, 2)), (4, 1)]
    for n, fi, fo in ((2, 25, 25), (9, 25, 50), (7, 50, 3), (6, Fraction(24000, 1001), 60), (3, 1, 1000)):
        s = list(V.frame_schedule(fi, fo, n))
        assert len(s) == count(n, fi, fo)
        assert all(0 <= p <= n - 2 and (0 <= t < 1 or (p, t) == (n - 2, 1)) for p, t in s)
        assert [p + t for p, t in s] == [j * Fraction(fi) / Fraction(fo) for j in range(len(s))]
    # endless form: the same entries, consumed as pairs become available
    g = V.frame_schedule(24, 60)
    assert [next(g) for _ in range(10)] == list(V.frame_schedule(24, 60, 5))[:10]
    with pytest.raises(ValueError):
        next(V.frame_schedule(0, 60))


# ----------------------------------------------------------------------------- render_stream on a fake model
class FakeModel:
    """Records what render_stream asks of the model.  A frame is tagged by its index (every pixel holds it); the
    'features' of a frame carry the index, the latent of a window the indices of its frames, and a decoded frame
    holds pair + t at every pixel."""
    device = "cpu"

    def __init__(self):
        self.encoded, self.windows, self.decodes = [], [], []
        self.latent = None

    def frame_features(self, frames):
        idx = frames[:, 0, 0, 0]
        self.encoded += [int(i) for i in idx]
        return tuple(idx.view(-1, 1, 1, 1).repeat(1, 2, 2, 3) * 10 + lv for lv in range(3))

    def gen_feat_window(self, frames, frame_feats=None):
        fr = [int(i) for i in frames[:, 0, 0, 0]]
        assert fr == list(range(fr[0], fr[0] + len(fr))) and len(fr) >= 2
        assert tuple(frames.shape[2:]) == (8, 8)                  # 6 x 7 frames arrive padded to a multiple of 4
        assert float(frames[:, :, 6:].abs().sum()) == 0 and float(frames[:, :, :, 7:].abs().sum()) == 0
        for lv, t in enumerate(frame_feats):                      # the features of exactly these frames, encoded before
            assert [int(v) for v in t[:, 0, 0, 0]] == [10 * i + lv for i in fr]
        self.windows.append(fr)
        self.latent = fr[:-1]

    def decoding_pairs(self, pairs, times, scale):
        assert len(set(len(t) for t in times)) == 1 and len(times[0]) == len(pairs)
        self.decodes.append(([self.latent[i] for i in pairs], len(times), tuple(scale)))
        return [torch.stack([torch.full((3, scale[0], scale[1]), self.latent[i] + float(t[j]))
                             for j, i in enumerate(pairs)]) for t in times]


class Source:
    """n tagged 6 x 7 frames, created one by one; counts how many of them are alive at any time."""

    def __init__(self, n):
        self.n, self.refs, self.peak = n, [], 0

    def alive(self):
        return sum(r() is not None for r in self.refs)

    def __iter__(self):
        for i in range(self.n):
            f = torch.full((3, 6, 7), float(i))
            self.refs.append(weakref.ref(f))
            yield f
            del f
            self.peak = max(self.peak, self.alive())


@pytest.mark.parametrize("chunk", [1, 3, 50])
@pytest.mark.parametrize("n, fi, fo", [(9, 25, 200), (8, 24, 60), (11, 60, 24), (6, 60, 24), (2, 25, 50)])
def test_render_stream_chunking(stif, chunk, n, fi, fo):
    V = stif.video
    m, src = FakeModel(), Source(n)
    got, held = [], 0
    for o in V.render_stream(m, src, fi, fo, scale=4, chunk_pairs=chunk):
        assert tuple(o.shape) == (3, 24, 28)                      # the top-left crop of the padded frame's 32 x 32 grid
        got.append(float(o[0, 0, 0]))
        held = max(held, src.alive())
        del o
    sched = list(V.frame_schedule(fi, fo, n))
    assert got == [float(np.float32(p) + np.float32(float(t))) for p, t in sched]      # display order, all frames
    assert m.encoded == list(range(n))                            # every frame encoded exactly once, in order
    assert max(held, src.peak) <= chunk + 1                       # frames pulled from the source and still alive
    used = sorted({p for p, _ in sched})
    ran = [p for w in m.windows for p in w[:-1]]
    assert sorted(set(ran)) == sorted(set(ran) | set(used))       # every pair with an output was fused ...
    # ... once, and a pair without one only where an output may still fall on its last frame (at most one per chunk)
    assert all(ran.count(p) == 1 for p in used) and len(set(ran) - set(used)) <= (n - 1 + chunk - 1) // chunk
    assert all(len(w) - 1 <= chunk for w in m.windows)
    assert all(sc == (32, 32) for _, _, sc in m.decodes)
    # no frame is decoded that is not yielded: the decode calls cover the schedule exactly
    assert sum(len(pairs) * k for pairs, k, _ in m.decodes) == len(sched)
    if (fi, fo) == (25, 200):                                     # a uniform schedule: one decode call per chunk
        assert [len(pairs) for pairs, _, _ in m.decodes[:-1]] == [len(w) - 1 for w in m.windows]


def test_render_stream_carries_the_last_frame(stif):
    """chunk_pairs = 3 over 8 frames: windows 0-3, 3-6, 6-7, each starting with the previous chunk's last frame
    and its features (FakeModel.gen_feat_window checks the features against the frames)."""
    m = FakeModel()
    list(stif.video.render_stream(m, Source(8), 25, 50, chunk_pairs=3))
    assert m.windows == [[0, 1, 2, 3], [3, 4, 5, 6], [6, 7]]
    assert m.encoded == list(range(8))
    m = FakeModel()
    out = list(stif.video.render_stream(m, Source(5), 24, 60, out_size=(10, 9), chunk_pairs=8))
    assert len(out) == 11 and tuple(out[0].shape) == (3, 10, 9)
    # the padded frame's grid: round(10 * 8 / 6) x round(9 * 8 / 7); pairs grouped by their number of queries
    assert [(p, k, sc) for p, k, sc in m.decodes] == [([0, 2], 3, (13, 10)), ([1, 3], 2, (13, 10)), ([3], 1, (13, 10))]
    with pytest.raises(ValueError, match="two frames"):
        list(stif.video.render_stream(FakeModel(), Source(1), 25, 50))
    with pytest.raises(ValueError, match="two frames"):
        list(stif.video.render_stream(FakeModel(), Source(0), 25, 50))
