"""Deterministic training, the host side (no GPU): stif_segsum, stif_dcn_bwd_contrib and stif_dec_x3_bwd_contrib are
declared, exported and bound; every invalid argument is rejected with its reason before any launch (fake pointers that
are never dereferenced, one changed argument at a time, as tests/test_dcn_bwd_host.py); segsum.hip is built like every
other kernel object and holds no floating-point atomic; the numpy emulation of the ordered sum (tests/segsum_ref.py)
is pinned; and the switch of the train module behaves."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import segsum_ref as S

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "stif-continuous-video-representation_amd", "csrc")
A = 4096
SIGS = {"stif_segsum": 12, "stif_dcn_bwd_contrib": 2, "stif_dec_x3_bwd_contrib": 10}
CONTRIB_FIELDS = ["in", "offmask", "w", "gout", "out", "g_om", "cm", "wgt", "words", "in_item", "om_item", "gout_item",
                  "out_item", "gom_item", "n", "H", "W", "epi"]


def rejected(L, name, args, text, why):
    lib = L.lib()
    lib.stif_dec_blend4(None, None, None, 0, 0, 0, None)   # another text sits in the error slot first
    rc = getattr(lib, name)(*args)
    err = lib.stif_last_error().decode()
    assert rc == L.E_INVALID, (name, why, rc, err)         # anything else would have launched
    assert err.startswith(name + ": ") and text in err, (name, why, text, err)


def test_the_symbols_are_declared_exported_and_bound(stif):
    L = stif._lib
    hdr = open(os.path.join(REPO, "include", "stif.h")).read()
    for name, nargs in SIGS.items():
        m = re.search(r"^\s*int\s+%s\s*\(([^;]*)\);" % name, hdr, re.M)
        assert m, name
        assert len(m.group(1).split(",")) == nargs, (name, m.group(1))
        assert hasattr(L.lib(), name), name
        res, args = L.EXPORTS[name]
        assert res is C.c_int and len(args) == nargs, name
    body = re.search(r"typedef struct \{([^}]*)\} stif_dcn_bwd_contrib_args;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+)\s*[,;]", body) == CONTRIB_FIELDS
    assert [f for f, _ in L.DcnBwdContribArgs._fields_] == ["inp"] + CONTRIB_FIELDS[1:]
    assert [t for _, t in L.DcnBwdContribArgs._fields_] == [C.c_void_p] * 9 + [C.c_longlong] * 5 + [C.c_int] * 4
    assert callable(stif.ops.segsum)
    nopk = re.search(r"^NOPK_SRC := (.*)$", open(os.path.join(REPO, "Makefile")).read(), re.M).group(1).split()
    assert "segsum" in nopk and os.path.exists(os.path.join(CSRC, "segsum.hip"))


def test_the_new_source_has_no_floating_point_atomics():
    src = open(os.path.join(CSRC, "segsum.hip")).read()
    code = re.sub(r"//[^\n]*|/\*.*?\*/", "", src, flags=re.S)
    assert not re.search(r"atomic", code, re.I), "segsum.hip must not use atomics of any kind"
    # the contribution branches of the two shared kernels store and never add: every atomic of those files sits in
    # the scatter code the atomic path had before
    for name, count in (("dcn_bwd.hip", 3), ("dec_train.hip", 4)):
        code = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, name)).read())
        assert len(re.findall(r"unsafeAtomicAdd|atomicAdd", code)) == count, name


# ---- rejections ----

def segsum_args(**changed):
    a = dict(dst=A, src=A, row_stride=576, K=72, col0=0, w=A, sorted=A, seg=A, D=560, E=20160, C=8, stream=None)
    a.update(changed)
    return list(a.values())


SEGSUM_BAD = [
    (dict(dst=None), "null pointer"), (dict(src=None), "null pointer"), (dict(w=None), "null pointer"),
    (dict(sorted=None), "null pointer"), (dict(seg=None), "null pointer"),
    (dict(C=16), "C must be 8, 64 or 192"), (dict(C=0), "C must be 8, 64 or 192"),
    (dict(D=0), "D, E, K must be >= 1"), (dict(E=0), "D, E, K must be >= 1"), (dict(K=0), "D, E, K must be >= 1"),
    (dict(E=2 ** 31), "E must be < 2^31"), (dict(D=2 ** 31), "D must be < 2^31"),
    (dict(col0=-4), "col0 must be >= 0"), (dict(col0=2, row_stride=580), "multiples of 4"),
    (dict(row_stride=578), "multiples of 4"), (dict(row_stride=572), "row_stride < K * C + col0"),
    (dict(col0=4), "row_stride < K * C + col0"),
    (dict(dst=A + 4), "16-byte aligned"), (dict(src=A + 8), "16-byte aligned"),
    (dict(w=A + 2), "8-byte aligned"), (dict(sorted=A + 4), "8-byte aligned"), (dict(seg=A + 4), "8-byte aligned"),
]


@pytest.mark.parametrize("changed,text", SEGSUM_BAD, ids=[f"{list(c)[0]}-{i}" for i, (c, _) in enumerate(SEGSUM_BAD)])
def test_segsum_rejections(stif, changed, text):
    rejected(stif._lib, "stif_segsum", segsum_args(**changed), text, changed)


def contrib_args(L, **changed):
    """A valid call on fake pointers: 2 x 5 x 7, g_om asked for, epi LRELU with its out."""
    a = L.DcnBwdContribArgs()
    a.inp, a.offmask, a.w, a.gout, a.out, a.g_om, a.cm, a.wgt, a.words = (A,) * 9
    a.in_item = a.gout_item = a.out_item = 5 * 7 * 64
    a.om_item, a.gom_item = 5 * 7 * 216, 5 * 7 * 256
    a.n, a.H, a.W, a.epi = 2, 5, 7, L.EPI_LRELU
    for k, v in changed.items():
        setattr(a, k, v)
    return a


CONTRIB_BAD = [
    (dict(inp=None), "null pointer (in, offmask, w, gout)"), (dict(offmask=None), "null pointer (in, offmask, w, gout)"),
    (dict(w=None), "null pointer (in, offmask, w, gout)"), (dict(gout=None), "null pointer (in, offmask, w, gout)"),
    (dict(cm=None), "null pointer (cm, wgt, words)"), (dict(wgt=None), "null pointer (cm, wgt, words)"),
    (dict(words=None), "null pointer (cm, wgt, words)"),
    (dict(epi=7), "epilogue must be NONE or LRELU"), (dict(out=None), "null pointer (out with STIF_EPI_LRELU)"),
    (dict(n=0), "n, H, W must be >= 1"), (dict(H=0), "n, H, W must be >= 1"), (dict(W=-1), "n, H, W must be >= 1"),
    (dict(in_item=-4), "negative item stride"), (dict(gom_item=-4), "negative item stride"),
    (dict(H=1 << 11, W=1 << 10), "item larger than 2 GB"),
    (dict(n=3000, H=50, W=50), "E = n * H * W * 288 must be < 2^31"),
    (dict(inp=A + 4), "16-byte aligned"), (dict(g_om=A + 8), "16-byte aligned"), (dict(cm=A + 4), "16-byte aligned"),
    (dict(wgt=A + 4), "16-byte aligned"), (dict(words=A + 8), "16-byte aligned"), (dict(om_item=5 * 7 * 216 + 2), "16-byte aligned"),
    (dict(gom_item=5 * 7 * 256 - 4), "g_om items overlap"),
]


@pytest.mark.parametrize("changed,text", CONTRIB_BAD, ids=[f"{list(c)[0]}-{i}" for i, (c, _) in enumerate(CONTRIB_BAD)])
def test_dcn_bwd_contrib_rejections(stif, changed, text):
    L = stif._lib
    rejected(L, "stif_dcn_bwd_contrib", (C.byref(contrib_args(L, **changed)), None), text, changed)


def test_dcn_bwd_contrib_rejects_null_args(stif):
    rejected(stif._lib, "stif_dcn_bwd_contrib", (None, None), "null args", "args")


def geom(L, **changed):
    g = L.DecTrainGeom()
    g.B, g.H, g.W, g.HH, g.WW = 2, 8, 12, 16, 24
    for name, _ in L.DecTrainGeom._fields_[5:]:
        setattr(g, name, A)
    for k, v in changed.items():
        setattr(g, k, v)
    return g


X3_PTRS = ("hrfeat", "flow", "g_x3", "g_flow", "w_hr", "words_hr", "w_lr", "words_lr")
X3_BAD = [(None, {k: None}, "null pointer (hrfeat, flow, g_x3, g_flow)") for k in X3_PTRS[:4]]
X3_BAD += [(None, {k: None}, "null pointer (w_hr, words_hr, w_lr, words_lr)") for k in X3_PTRS[4:]]
X3_BAD += [(None, dict(words_hr=A + 4), "8-byte aligned"), (None, dict(words_lr=A + 4), "8-byte aligned"),
           (dict(feat=None), {}, "null pointer (feat, frames, t)"), (dict(HH=1), {}, "HH and WW must be >= 2"),
           (dict(B=0), {}, "B, H, W must be >= 1"), (dict(lin_x=None), {}, "null table pointer"),
           (dict(bx1_first=None), {}, "null inverse table pointer"),
           (dict(B=1, H=1, W=1, HH=1 << 13, WW=1 << 12), {}, "more than 2^31 - 1 float4 of a matrix")]


@pytest.mark.parametrize("gchanged,pchanged,text", X3_BAD, ids=[str(i) for i in range(len(X3_BAD))])
def test_dec_x3_bwd_contrib_rejections(stif, gchanged, pchanged, text):
    L = stif._lib
    ptrs = dict.fromkeys(X3_PTRS, A)
    ptrs.update(pchanged)
    rejected(L, "stif_dec_x3_bwd_contrib", (C.byref(geom(L, **(gchanged or {}))), *ptrs.values(), None), text,
             (gchanged, pchanged))


def test_dec_x3_bwd_contrib_rejects_a_null_geometry(stif):
    rejected(stif._lib, "stif_dec_x3_bwd_contrib", (None,) + (A,) * 8 + (None,), "null geometry", "g")


# ---- the emulation ----

def random_scatter(seed, D=560, C=8, K=72, E=20160):
    rng = np.random.default_rng(seed)
    key = rng.integers(0, D + 1, E)                      # D: the sentinel
    w = rng.random(E, dtype=np.float32)
    src = rng.standard_normal(((E // 4 + K - 1) // K) * K * C).astype(np.float32)
    return key, w, S.sub_rows(src, E, K * C, K, C, 0)


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def test_the_emulation_is_a_sequential_sum_in_entry_order():
    key, w, rows = random_scatter(1)
    D = 560
    got = S.emulate(S.pack(key), w, rows, D)
    for d in (0, 17, D - 1):
        acc = np.zeros(8, np.float32)
        for e in np.flatnonzero(key == d):               # ascending e; far fewer than 512 of them
            acc = acc + np.float32(w[e]) * rows[e >> 2]
            assert acc.dtype == np.float32
        assert np.array_equal(bits(got[d]), bits(acc)), d
    key[key == 5] = 6                                    # an empty row is +0.0
    assert np.array_equal(bits(S.emulate(S.pack(key), w, rows, D)[5]), np.zeros(8, np.int32))


def test_the_emulation_cuts_long_lists_into_chunks_of_512():
    rng = np.random.default_rng(2)
    E = 4 * 300
    key = np.zeros(E, np.int64)                          # one list of 1200 entries: chunks of 512, 512, 176
    w, rows = rng.random(E, dtype=np.float32), rng.standard_normal((E // 4, 8)).astype(np.float32)
    parts = []
    for lo in range(0, E, S.CHUNK):
        acc = np.zeros(8, np.float32)
        for e in range(lo, min(lo + S.CHUNK, E)):
            acc = acc + np.float32(w[e]) * rows[e >> 2]
        parts.append(acc)
    want = (parts[0] + parts[1]) + parts[2]
    got = S.emulate(S.pack(key), w, rows, 1)[0]
    assert np.array_equal(bits(got), bits(want))
    flat = np.zeros(8, np.float32)
    for e in range(E):
        flat = flat + np.float32(w[e]) * rows[e >> 2]
    assert not np.array_equal(bits(flat), bits(want)), "the chunk rule must be visible in the value"


def test_a_permutation_of_equal_key_entries_changes_the_value_unless_the_words_are_sorted():
    key, w, rows = random_scatter(3)
    D, words = 560, S.pack(key)
    ref = S.emulate(words, w, rows, D)
    shuffled = np.random.default_rng(4).permutation(words)
    assert np.array_equal(bits(S.emulate(shuffled, w, rows, D)), bits(ref))
    unsorted = S.emulate(shuffled, w, rows, D, sort=False)
    assert float((bits(unsorted) != bits(ref)).mean()) > 0.5
    np.testing.assert_allclose(unsorted, ref, rtol=0, atol=1e-4)
    # every list walked backwards: the same terms in another order
    changed = float((bits(S.emulate(words, w, rows, D, reverse=True)) != bits(ref)).mean())
    print(f"reversal changes {100 * changed:.0f} % of the elements")
    assert changed > 0.5
    srt, seg = S.sorted_segments(words, D)
    assert seg[0] == 0 and seg[D] == int((key < D).sum()) and np.array_equal(np.diff(seg), np.bincount(key, minlength=D + 1)[:D])


# ---- the switch ----

def test_the_train_switch_is_off_by_default_and_the_context_manager_restores(stif):
    TR = stif.train
    assert TR.is_deterministic() is False
    with TR.deterministic():
        assert TR.is_deterministic() is True
        with TR.deterministic(False):
            assert TR.is_deterministic() is False
            with TR.deterministic():
                assert TR.is_deterministic() is True
            assert TR.is_deterministic() is False
        assert TR.is_deterministic() is True
    assert TR.is_deterministic() is False
    TR.set_deterministic(True)
    try:
        assert TR.is_deterministic() is True
        with TR.deterministic(False):
            assert TR.is_deterministic() is False
        assert TR.is_deterministic() is True
        with pytest.raises(KeyError):
            with TR.deterministic(False):
                raise KeyError("the state comes back after an exception too")
        assert TR.is_deterministic() is True
    finally:
        TR.set_deterministic(False)
    assert "use_deterministic_algorithms" in TR.set_deterministic.__doc__
