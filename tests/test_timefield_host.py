"""Host side of time fields (a query time per output pixel): the reference fixture against the oracle composite,
the sensitivity of the test inputs, the classification of time queries, and the two C-ABI entry points (exported,
declared, validating before any launch -- the fake pointers are never dereferenced).  Nothing here needs a GPU."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import stage2_inputs as S
import timefield_inputs as TF
from oracle import stif_oracle as O

F32 = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(HERE, "golden", "timefield_16x20.npz"))


@pytest.fixture(scope="module")
def latent(golden):
    g = golden["model_16x20"]
    return g["feat"][None], g["x"]                       # [1,3,64,16,20], [1,2,3,16,20]


@pytest.mark.parametrize("case", ["random", "ramp"])
def test_oracle_composite_matches_the_reference_field_decode(fixture, latent, sd, case):
    """The reference's own decoding with times[c] of shape [1, HH*WW] against the composite of the unchanged oracle
    stages (one call per distinct value), within 1e-5 max|ref| -- the bound tests/test_oracle.py uses for its
    decoder variants.  random: four values at 64 x 80; ramp: 37 values (one per row) at 37 x 45."""
    feat, inp = latent
    field, ref = fixture[f"{case}_field"], fixture[f"{case}_out"]
    _, HH, WW = field.shape
    assert ref.shape == (1, 3, HH, WW)
    if case == "random":
        assert np.array_equal(field, TF.random_field(1, 64, 80)) and set(np.unique(field)) == set(TF.VALUES)
    else:
        assert np.array_equal(field, TF.row_ramp(37, 45))
    rgb = TF.decode_composite(feat, inp, field, sd, HH, WW)[2]
    err, tol = float(np.abs(rgb - ref).max()), 1e-5 * float(np.abs(ref).max())
    print(f"{case}: max|composite - reference| = {err:.3e} (tol {tol:.3e})")
    assert err <= tol


def test_the_field_inputs_expose_every_misindexing(latent, sd):
    """About the reference (through the oracle) and the inputs only.  At 37 x 45 with the random four-valued field:
    reading the field one column or one row off, or with the rows flipped, breaks the project bound
    |d| <= 1e-4 |ref| + 1e-6 by at least 10x at every pixel whose value changed, on HRfeat, on the flow and on the
    RGB; and stage 2 run with the field's mean as one scalar time breaks it by at least 10x at every pixel."""
    feat, inp = latent
    HH, WW = 37, 45
    field = TF.random_field(1, HH, WW)
    per = TF.stage1_per_value(feat, inp, TF.VALUES, sd, HH, WW)
    hrf, flow, rgb = TF.decode_composite(feat, inp, field, sd, HH, WW, per)

    def pixel_ratio(got, ref, axis):                     # the worst channel of every pixel
        return S.bound_ratio(got, ref).max(axis=axis)

    for name, wrong in (("column", np.roll(field, 1, 2)), ("row", np.roll(field, 1, 1)), ("flip", field[:, ::-1])):
        changed = wrong != field
        assert 0.7 <= changed.mean() <= 0.8, (name, changed.mean())
        h2, f2, r2 = TF.decode_composite(feat, inp, wrong, sd, HH, WW, per)
        worst = [float(pixel_ratio(g, r, ax)[changed].min()) for g, r, ax in ((h2, hrf, -1), (f2, flow, -1), (r2, rgb, 1))]
        print(f"field read with the {name} wrong: least bound ratio at a changed pixel: hrfeat {worst[0]:.0f}, "
              f"flow {worst[1]:.0f}, rgb {worst[2]:.0f}")
        assert min(worst) >= 10, (name, worst)
    mean = O.decode_stage2(feat, inp, hrf, flow, np.full(1, field.mean(), F32), sd, HH, WW)
    r = pixel_ratio(mean, rgb, 1)
    print(f"stage 2 with the field's mean: least bound ratio {float(r.min()):.0f}, median {float(np.median(r)):.0f}")
    assert float(r.min()) >= 10


# ----------------------------------------------------------------------------- classification of time queries
def test_time_query_classification(stif):
    cls = stif.coords.classify_time_query
    B, HH, WW = 3, 37, 45
    for shape in [(), (1,), (1, 1), (B,), (B, 1), (1, B), (B, 1, 1)]:
        assert cls(shape, B, HH, WW) == ("vector", None), shape
    fields = {(HH, WW): (1, HH, WW), (B, HH, WW): (B, HH, WW), (1, HH, WW): (1, HH, WW),
              (B, 1, HH, WW): (B, HH, WW), (1, 1, HH, WW): (1, HH, WW),
              (B, HH, 1): (B, HH, 1), (HH, 1): (1, HH, 1), (1, WW): (1, 1, WW), (WW,): (1, 1, WW),
              (B, 1, WW): (B, 1, WW), (B, 1, HH, 1): (B, HH, 1),
              (B, HH * WW): (B, HH, WW), (1, HH * WW): (1, HH, WW)}
    for shape, s3 in fields.items():
        assert cls(shape, B, HH, WW) == ("field", s3), shape
    for shape in [(HH,), (HH * WW,), (WW, HH), (2, HH, WW), (B, 2, HH, WW), (B, HH, WW, 1), (HH, WW, B), (2,),
                  (B + 1, HH * WW), (B, HH * WW + 1)]:
        with pytest.raises(ValueError, match="neither 1 or 3 values nor a field"):
            cls(shape, B, HH, WW)
    # a tensor of B elements keeps its meaning even where it could be read as a field
    assert cls((37, 1), 37, 37, 45) == ("vector", None)
    assert cls((HH, WW), 1, HH, WW) == ("field", (1, HH, WW))


def test_row_time_field(stif):
    f = stif.coords.row_time_field(5, 0.5, 0.2)
    assert f.shape == (5, 1) and f.dtype == np.float32
    assert np.array_equal(f[:, 0], np.array([0.4, 0.45, 0.5, 0.55, 0.6], np.float64).astype(np.float32))
    assert stif.coords.classify_time_query(f.shape, 2, 5, 7) == ("field", (1, 5, 1))


def test_fields_are_refused_where_they_have_no_meaning(stif, sd):
    """ensemble=True, decoding_test, decoding_fasttest and decoding_localensemble with a field raise ValueError
    before anything is launched (a CPU module with a stand-in latent: the checks come first)."""
    m = stif.LunaTokis(64, 6, 8, 5, 40, device="cpu")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    m._feat = torch.zeros(3, 1, 16, 20, 64)
    m.inp = torch.zeros(1, 2, 3, 16, 20)
    field = torch.zeros(64, 80)
    with pytest.raises(ValueError, match="time field is not supported with ensemble=True"):
        m._decoding([field], None, ensemble=True)
    with pytest.raises(ValueError, match="time field is not supported in decoding_test"):
        m._decoding_test([field], None)
    with pytest.raises(ValueError, match="time field is not supported in decoding_fasttest"):
        m._decoding_fasttest([field], None)
    with pytest.raises(ValueError, match="time field is not supported in decoding_localensemble"):
        m._decoding_localensemble([field], None)
    with pytest.raises(ValueError, match="neither 1 or 1 values nor a field"):
        m._decoding([torch.zeros(63, 80)], None)


# ----------------------------------------------------------------------------- the C ABI
def test_timefield_symbols_are_exported_and_declared(stif):
    lib = stif._lib.lib()
    for name in ("stif_dec_stage1_tf", "stif_dec_stage2_tf"):
        assert hasattr(lib, name), name
        assert name in stif._lib.EXPORTS
    T = stif._lib.DecTimeField                           # a pointer and three long long strides
    assert C.sizeof(T) == 32 and (T.t.offset, T.item.offset, T.row.offset, T.col.offset) == (0, 8, 16, 24)


def test_timefield_entry_points_validate_before_launching(stif):
    """An image, tables with hr_y / hr_x, a null t and a negative stride are STIF_E_INVALID with a message naming
    the reason, for both entry points, whole grid and window."""
    L = stif._lib
    lib = L.lib()
    A = 4096                                             # a fake address: validation comes first
    p = C.c_void_p(A)
    tab, tab_hr = L.DecTables(*[A] * 14), L.DecTables(*[A] * 16)
    img = L.DecImage(A, 64, 80, *[A] * 8)
    HH, WW = 37, 45
    good = L.DecTimeField(A, HH * WW, WW, 1)
    win = L.DecWindow(9, 11, 13, 17)

    def s1(t=good, tab=tab, img=None, win=None):
        return lib.stif_dec_stage1_tf(p, p, C.byref(tab), C.byref(img) if img is not None else None,
                                      C.byref(t) if t is not None else None, p, p, 1, 16, 20, HH, WW, 0, None, None,
                                      C.byref(win) if win is not None else None)

    def s2(t=good, tab=tab, img=None, win=None):
        return lib.stif_dec_stage2_tf(p, p, p, p, C.byref(tab), C.byref(img) if img is not None else None,
                                      C.byref(t) if t is not None else None, p, 1, 16, 20, HH, WW, 0, None, None,
                                      C.byref(win) if win is not None else None)

    def rejected(rc, text, me):
        err = lib.stif_last_error().decode()
        assert rc == L.E_INVALID, (text, err)
        assert err.startswith(me + ": ") and text in err, (text, err)

    for fn, me in ((s1, "stif_dec_stage1_tf"), (s2, "stif_dec_stage2_tf")):
        for w in (None, win):
            rejected(fn(img=img, win=w), "high-resolution image", me)
            rejected(fn(tab=tab_hr, win=w), "hr_y / hr_x", me)
            rejected(fn(t=None, win=w), "null time field", me)
            rejected(fn(t=L.DecTimeField(None, 1, 0, 0), win=w), "null time field", me)
            for bad in ((-1, 0, 0), (0, -WW, 1), (HH * WW, WW, -1)):
                rejected(fn(t=L.DecTimeField(A, *bad), win=w), "negative time-field stride", me)
        # the window rules are those of the windowed entry points
        rejected(fn(win=L.DecWindow(30, 11, 13, 17)), "not inside the HH x WW grid", me)
    rejected(s1(win=L.DecWindow(9, 11, 13, 17, 10, 11, 12, 17)), "does not contain the query rectangle",
             "stif_dec_stage1_tf")
