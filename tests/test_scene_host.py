"""Scene cuts without a GPU: the cut score against hand-computed values, and the hold-instead-of-blend policy of
the streaming renderer on a recording fake model (forced cuts through hold_pairs; the detector's wiring through a
stand-in for ops.scene_sad)."""
from fractions import Fraction

import numpy as np
import pytest
import torch

AREA = 255 * 6 * 7                # SAD of a 6 x 7 pair whose mean luma change is 1


# ----------------------------------------------------------------------------- scene_scores
def test_scores_by_hand(stif):
    S = stif.video.scene_scores
    h, w = 4, 5                                                   # 255 h w = 5100
    scores, last = S([510, 1020, 4080, 1020], h, w)
    # m = 0.1, 0.2, 0.8, 0.2; the first pair has no predecessor and scores min(m, |m - m|) = 0
    assert scores == pytest.approx([0.0, 0.1, 0.6, 0.2], abs=1e-15) and last == pytest.approx(0.2, abs=1e-15)
    assert scores[0] == 0.0 and all(isinstance(s, float) for s in scores)
    scores, last = S([510], h, w, prev=0.5)                       # with a predecessor the first pair scores too
    assert scores == pytest.approx([0.1]) and last == pytest.approx(0.1)
    assert S([5100, 0], h, w) == ([0.0, 0.0], 0.0)                # m = 1 then 0: min(0, 1) = 0
    assert S([], h, w, prev=0.25) == ([], 0.25)
    t = torch.tensor([510, 1020], dtype=torch.int64)              # what ops.scene_sad returns, read back or not
    assert S(t, h, w) == S(t.tolist(), h, w) == S(np.array([510, 1020]), h, w)


def test_scores_carry_prev_across_a_split(stif):
    S = stif.video.scene_scores
    sad = [123, 4567, 89, 3021]
    whole, last = S(sad, 6, 7)
    first, mid = S(sad[:2], 6, 7)
    second, end = S(sad[2:], 6, 7, prev=mid)
    assert first + second == whole and end == last                # bit for bit, not approximately
    for cut in (1, 3):
        a, m = S(sad[:cut], 6, 7)
        b, _ = S(sad[cut:], 6, 7, prev=m)
        assert a + b == whole


def test_scores_flash_and_steady_motion(stif):
    S = stif.video.scene_scores
    # a one-frame flash: two large m in a row, only the first exceeds the threshold
    m = [0.01, 0.01, 0.6, 0.61, 0.01, 0.01]
    scores, _ = S([round(v * AREA) for v in m], 6, 7)
    assert [s > 0.1 for s in scores] == [False, False, True, False, False, False]
    assert scores[2] == pytest.approx(0.59, abs=1e-3) and scores[3] == pytest.approx(0.01, abs=1e-3)
    # steady fast motion: a large m throughout, nothing scores
    scores, _ = S([round(0.3 * AREA)] * 5, 6, 7)
    assert max(scores) == 0.0
    # a cut: one large m between small ones, detected once
    scores, _ = S([round(v * AREA) for v in (0.01, 0.5, 0.01)], 6, 7)
    assert [s > 0.1 for s in scores] == [False, True, False]


# ----------------------------------------------------------------------------- the hold policy on a fake model
class HoldModel:
    """Records what the renderer asks of the model.  A frame is tagged by its index (every pixel holds it); the
    'features' of a frame carry the index, the latent of a window the first frame of each of its pairs, and a
    decoded frame holds that index + t at every pixel.  A window is either consecutive frames or the degenerate
    pair [f, f] of a held frame, whose decode at t = 0 holds f."""
    device = "cpu"

    def __init__(self):
        self.encoded, self.windows, self.holds, self.decodes, self.hold_decodes = [], [], [], [], []
        self.latent, self.degenerate = None, False

    def frame_features(self, frames):
        idx = frames[:, 0, 0, 0]
        self.encoded += [int(i) for i in idx]
        return tuple(idx.view(-1, 1, 1, 1).repeat(1, 2, 2, 3) * 10 + lv for lv in range(3))

    def gen_feat_window(self, frames, frame_feats=None):
        fr = [int(i) for i in frames[:, 0, 0, 0]]
        assert tuple(frames.shape[1:]) == (3, 8, 8)               # 6 x 7 frames arrive padded to a multiple of 4
        for lv, t in enumerate(frame_feats):                      # the features of exactly these frames, encoded before
            assert [int(v) for v in t[:, 0, 0, 0]] == [10 * i + lv for i in fr]
        self.degenerate = len(fr) == 2 and fr[0] == fr[1]
        if self.degenerate:
            self.holds.append(fr[0])
        else:
            assert fr == list(range(fr[0], fr[0] + len(fr))) and len(fr) >= 2
            self.windows.append(fr)
        self.latent = fr[:-1]

    def decoding_pairs(self, pairs, times, scale):
        assert len(set(len(t) for t in times)) == 1 and len(times[0]) == len(pairs)
        if self.degenerate:
            assert list(pairs) == [0] and len(times) == 1 and float(times[0][0]) == 0.0
            self.hold_decodes.append(self.latent[0])
        else:
            self.decodes.append(([self.latent[i] for i in pairs], len(times), tuple(scale)))
        return [torch.stack([torch.full((3, scale[0], scale[1]), self.latent[i] + float(t[j]))
                             for j, i in enumerate(pairs)]) for t in times]


def source(n):
    return (torch.full((3, 6, 7), float(i)) for i in range(n))


def shown(p, t, cuts):
    """the value of output (p, t): the held frame's index in a cut pair, else what the fake decodes"""
    if p in cuts:
        return float(p if t < Fraction(1, 2) else p + 1)
    return float(np.float32(p) + np.float32(float(t)))


CASES = {
    "middle": (8, 24, 60, [3]),
    "adjacent": (8, 24, 60, [3, 4]),
    "first": (6, 25, 100, [0]),
    "last, with the closing frame": (5, 25, 50, [3]),
    "last, closing frame only after t = 0": (5, 25, 25, [3]),
    "no output in the cut pair": (11, 60, 24, [3, 4]),            # outputs fall in pairs 0, 2, 5, 7 and on frame 10
    "half-way output and a bare closing frame": (11, 60, 24, [2, 9]),
    "every pair": (4, 2, 5, [0, 1, 2]),
}


@pytest.mark.parametrize("chunk", [1, 3, 50])
@pytest.mark.parametrize("case", list(CASES))
def test_hold_policy(stif, case, chunk):
    V = stif.video
    n, fi, fo, hold = CASES[case]
    m, cuts = HoldModel(), []
    outs = list(V.render_stream(m, source(n), fi, fo, scale=4, chunk_pairs=chunk, hold_pairs=hold, cuts=cuts))
    sched = list(V.frame_schedule(fi, fo, n))
    assert len(outs) == len(sched)                                # the schedule does not change
    assert all(tuple(o.shape) == (3, 24, 28) for o in outs)
    assert [float(o[0, 0, 0]) for o in outs] == [shown(p, t, hold) for p, t in sched]
    assert all(bool((o == o[0, 0, 0]).all()) for o in outs)
    assert len({o.data_ptr() for o in outs}) == len(outs)         # every yielded frame is its own tensor
    assert cuts == hold                                           # exactly the held pairs, in order
    assert m.encoded == list(range(n))                            # every frame encoded once
    fused = [p for w in m.windows for p in w[:-1]]
    assert not set(fused) & set(hold)                             # a cut pair is never fused as (p, p + 1)
    used = {p for p, _ in sched} - set(hold)
    assert used <= set(fused) and all(fused.count(p) == 1 for p in used)
    assert all(len(w) - 1 <= chunk for w in m.windows)
    # a cut breaks the runs: no window spans a cut pair
    assert all(not (w[0] <= p < w[-1]) for w in m.windows for p in hold)
    # each held frame is fused and decoded once per pair, however many outputs repeat it
    want = []
    for p in hold:
        ts = [t for q, t in sched if q == p]
        want += [p] * any(t < Fraction(1, 2) for t in ts) + [p + 1] * any(t >= Fraction(1, 2) for t in ts)
    assert m.holds == want and m.hold_decodes == want
    # no frame is decoded that is not yielded
    assert sum(len(pairs) * k for pairs, k, _ in m.decodes) == sum(1 for p, _ in sched if p not in hold)


def test_defaults_record_what_they_recorded_before(stif, monkeypatch):
    """No new argument: the windows and decodes of the renderer as it was (the values test_y4m_host.py pins), no
    held frame and no scene_sad call; passing the defaults explicitly is the same."""
    V = stif.video

    def no_scene(*a, **k):
        raise AssertionError("scene_sad called with the detector off")
    monkeypatch.setattr(stif.ops, "scene_sad", no_scene)
    runs = []
    for kw in ({}, dict(scene_threshold=None, hold_pairs=(), cuts=[])):
        m = HoldModel()
        a = [float(o[0, 0, 0]) for o in V.render_stream(m, source(8), 25, 50, chunk_pairs=3, **kw)]
        assert m.windows == [[0, 1, 2, 3], [3, 4, 5, 6], [6, 7]] and m.holds == [] and m.hold_decodes == []
        assert m.encoded == list(range(8))
        m2 = HoldModel()
        b = list(V.render_stream(m2, source(5), 24, 60, out_size=(10, 9), chunk_pairs=8, **kw))
        assert len(b) == 11 and tuple(b[0].shape) == (3, 10, 9)
        assert m2.decodes == [([0, 2], 3, (13, 10)), ([1, 3], 2, (13, 10)), ([3], 1, (13, 10))] and m2.holds == []
        assert kw.get("cuts", []) == []
        runs.append((a, m.windows, m.decodes, [float(o[0, 0, 0]) for o in b], m2.windows, m2.decodes))
    assert runs[0] == runs[1]
    assert runs[0][0] == [shown(p, t, ()) for p, t in V.frame_schedule(25, 50, 8)]


@pytest.mark.parametrize("chunk", [1, 3, 50])
def test_detector_wiring(stif, monkeypatch, chunk):
    """The detector on a stand-in for ops.scene_sad (pair (i, i + 1) of the tagged frames has the SAD TABLE[i]): one
    call per chunk over exactly the chunk's pairs -- the carried last frame first -- scoring the unpadded rectangle;
    m is carried across chunks, so the cuts do not depend on the chunking: a cut at pair 2, a flash over pairs 5
    and 6 detected once, and a forced pair on top."""
    V = stif.video
    m_of = [0.01, 0.01, 0.5, 0.01, 0.01, 0.6, 0.61, 0.01, 0.01]
    table = [round(v * AREA) for v in m_of]
    calls = []

    def fake_sad(x, h, w):
        assert (h, w) == (6, 7) and tuple(x.shape[1:]) == (3, 8, 8)
        idx = [int(i) for i in x[:, 0, 0, 0]]
        assert idx == list(range(idx[0], idx[0] + len(idx))) and len(idx) >= 2
        calls.append(idx)
        return torch.tensor([table[i] for i in idx[:-1]], dtype=torch.int64)
    monkeypatch.setattr(stif.ops, "scene_sad", fake_sad)
    m, cuts = HoldModel(), []
    outs = list(V.render_stream(m, source(10), 25, 50, chunk_pairs=chunk, scene_threshold=0.1, hold_pairs=[7],
                                cuts=cuts))
    assert cuts == [2, 5, 7]
    sched = list(V.frame_schedule(25, 50, 10))
    assert [float(o[0, 0, 0]) for o in outs] == [shown(p, t, cuts) for p, t in sched]
    assert [p for c in calls for p in c[:-1]] == list(range(9))   # every pair scored once, in order
    assert all(a[-1] == b[0] for a, b in zip(calls, calls[1:]))   # each chunk starts with the carried frame
    assert len(calls) == -(-9 // chunk) and m.encoded == list(range(10))
