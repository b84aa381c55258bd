"""Host side of the windowed local ensemble: the two C-ABI entry points (exported, declared, and validating every
argument before any launch -- the fake pointers are never dereferenced) and the remap rectangle the host derives
from the monotone hr_y / hr_x tables."""
import ctypes as C

import numpy as np

from test_gpu_window import windows


def test_ensemble_symbols_are_exported_and_declared(stif):
    lib = stif._lib.lib()
    for name in ("stif_dec_flow_win", "stif_dec_stage2_blend_win"):
        assert hasattr(lib, name), name
        assert name in stif._lib.EXPORTS
    # the ctypes struct has the C layout: two ints, then 4 + 4 pointers
    B = stif._lib.DecBlend
    assert C.sizeof(B) == 72 and (B.k.offset, B.accumulate.offset, B.rel_y.offset, B.rel_x.offset) == (0, 4, 8, 40)


def test_ensemble_entry_points_validate_before_launching(stif):
    """Every rejected call returns STIF_E_INVALID with a message that names the cause."""
    L = stif._lib
    lib = L.lib()
    A = 4096                                 # a fake address: validation comes first
    p = C.c_void_p(A)
    tab = L.DecTables(*[A] * 14)             # hr_y / hr_x stay NULL
    tab_hr = L.DecTables(*[A] * 16)
    tab_hr_y = L.DecTables(*[A] * 15)        # hr_y without hr_x
    tab_hole = L.DecTables(*[A] * 16)
    tab_hole.lin_x = None
    img = L.DecImage(A, 64, 80, *[A] * 8)
    HH, WW = 37, 45
    W = L.DecWindow

    def blend(k=0, accumulate=0):
        b = L.DecBlend()
        b.k, b.accumulate = k, accumulate
        for j in range(4):
            b.rel_y[j], b.rel_x[j] = A, A
        return b

    def fl(win, tab=tab_hr, img=None, hrf=p, flow=p, t=p, proj=p, mlp=p, n=1):
        return lib.stif_dec_flow_win(proj, mlp, C.byref(tab) if tab is not None else None,
                                     C.byref(img) if img is not None else None, t, hrf, flow, n, 16, 20, HH, WW, 0,
                                     None, None, C.byref(win) if win is not None else None)

    def s2(win, bl=blend(), tab=tab_hr, img=None, out=p, hrf=p, flow=p, n=1):
        return lib.stif_dec_stage2_blend_win(p, p, hrf, flow, C.byref(tab) if tab is not None else None,
                                             C.byref(img) if img is not None else None, p, out, n, 16, 20, HH, WW, 0,
                                             None, None, C.byref(bl) if bl is not None else None,
                                             C.byref(win) if win is not None else None)

    def rejected(rc, text, me):
        err = lib.stif_last_error().decode()
        assert rc == L.E_INVALID, (text, err)
        assert err.startswith(me + ": ") and text in err, (text, err)

    ok = W(9, 11, 13, 17)
    # the window rules of window_resolve, for both entry points
    for text, win in [("query rectangle", W(30, 0, 13, 17)), ("query rectangle", W(0, 40, 3, 6)),
                      ("query rectangle", W(0, 0, 0, 5)), ("F rectangle", W(9, 11, 13, 17, 7, 9, 31, 21)),
                      ("null window", None)]:
        rejected(fl(win), text, "stif_dec_flow_win")
        rejected(s2(win), text, "stif_dec_stage2_blend_win")
    rejected(s2(W(9, 11, 13, 17, 0, 0, 0, 0, 3 * 13 * 16, 13 * 16, 16)), "out_pitch", "stif_dec_stage2_blend_win")
    # the flow stage: remap tables are required, an image is not taken, null pointers
    rejected(fl(ok, tab=tab), "hr_y", "stif_dec_flow_win")
    rejected(fl(ok, tab=tab_hr_y), "hr_y", "stif_dec_flow_win")
    rejected(fl(ok, img=img), "img", "stif_dec_flow_win")
    for kw in (dict(hrf=None), dict(flow=None), dict(t=None), dict(proj=None), dict(mlp=None), dict(tab=None),
               dict(tab=tab_hole), dict(n=0)):
        rejected(fl(ok, **kw), "bad arguments", "stif_dec_flow_win")
    # F need not hold the query rectangle here (stage 1's rule does not apply): only the launch is left, which a
    # rejected call never reaches -- so this one is checked on the GPU (tests/test_gpu_ensemble.py)
    # the blending stage 2: the blend descriptor, no image, null pointers
    rejected(s2(ok, bl=None), "null blend", "stif_dec_stage2_blend_win")
    for k in (-1, 4, 7):
        rejected(s2(ok, bl=blend(k)), "k outside 0..3", "stif_dec_stage2_blend_win")
    for acc in (-1, 2):
        rejected(s2(ok, bl=blend(1, acc)), "accumulate must be 0 or 1", "stif_dec_stage2_blend_win")
    for field, j in (("rel_y", 0), ("rel_y", 3), ("rel_x", 1), ("rel_x", 2)):
        b = blend(2)
        getattr(b, field)[j] = None
        rejected(s2(ok, bl=b), "null rel_y / rel_x", "stif_dec_stage2_blend_win")
    rejected(s2(ok, img=img), "img", "stif_dec_stage2_blend_win")
    for kw in (dict(out=None), dict(hrf=None), dict(flow=None), dict(tab=None), dict(tab=tab_hole), dict(n=0)):
        rejected(s2(ok, **kw), "bad arguments", "stif_dec_stage2_blend_win")
    # the existing windowed stage 1 still refuses remap tables
    assert lib.stif_dec_stage1_win(p, p, C.byref(tab_hr), None, p, p, p, 1, 16, 20, HH, WW, 0, None, None,
                                   C.byref(ok)) == L.E_INVALID
    assert b"hr_y" in lib.stif_last_error()


def test_remap_rectangle_agrees_with_the_tables(stif):
    """ops.remap_rect (what the host sizes the first feat-only pass by) is the bounding box of hr_y x hr_x over the
    window, the tables are monotone (so the two corner entries are that box), and the remap moves a pixel by at
    most 2 at 4x and at most 1 at the other grids."""
    for HH, WW in [(64, 80), (37, 45), (40, 50), (12, 15)]:
        bound = 2 if (HH, WW) == (64, 80) else 1
        for shift in stif.ops.ENSEMBLE_SHIFTS:
            t = stif.coords.dec_tables(16, 20, HH, WW, shift)
            hy, hx = t["hr_y"], t["hr_x"]
            assert (np.diff(hy) >= 0).all() and (np.diff(hx) >= 0).all()
            assert np.abs(hy - np.arange(HH)).max() <= bound and np.abs(hx - np.arange(WW)).max() <= bound
            for name, (y0, x0, hh, ww) in windows(HH, WW).items():
                if y0 < 0 or x0 < 0 or y0 + hh > HH or x0 + ww > WW:
                    continue                 # the list is written for grids of at least 13 x 17 / 19 x 23
                ry0, rx0, rh, rw = stif.ops.remap_rect(hy, hx, (y0, x0, hh, ww))
                ys, xs = hy[y0:y0 + hh], hx[x0:x0 + ww]
                assert (ry0, rx0) == (ys.min(), xs.min()), (HH, WW, shift, name)
                assert (ry0 + rh - 1, rx0 + rw - 1) == (ys.max(), xs.max()), (HH, WW, shift, name)
                assert 0 <= ry0 and ry0 + rh <= HH and 0 <= rx0 and rx0 + rw <= WW


def test_blend_descriptor_points_at_the_four_shifts_rel_tables(stif):
    """The epilogue's weight formula on the host tables is coords.ensemble_weights bit for bit (the kernel evaluates
    the same fp32 expression per pixel: tests/test_gpu_ensemble.py compares its output)."""
    F32 = np.float32
    for HH, WW in [(64, 80), (37, 45)]:
        tabs = [stif.coords.dec_tables(16, 20, HH, WW, s) for s in stif.ops.ENSEMBLE_SHIFTS]
        a = [(np.abs(np.outer(t["rel_y"], t["rel_x"])) + F32(1e-9)).astype(F32) for t in tabs]
        assert all(x.dtype == F32 for x in a)
        tot = ((a[0] + a[1]) + a[2]) + a[3]
        ref = stif.coords.ensemble_weights(16, 20, HH, WW)
        for k in range(4):
            assert np.array_equal(a[3 - k] / tot, ref[k])
