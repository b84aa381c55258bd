"""Host side of windowed decoding: the zoom rectangle arithmetic, the window checks of the Python layer (before any
device call) and the C ABI's new symbols and argument validation (which returns before any launch)."""
import ctypes as C

import numpy as np
import pytest


def test_window_from_center_hand_worked(stif):
    f = stif.coords.window_from_center
    # 1024 x 1024, 512 x 512: centre pixel int((c + 1) / 2 * 1024), start 256 before it
    assert f((0, 0), 1024, 1024, (512, 512)) == (256, 256, 512, 512)
    # rows: centre 51, 51 - 256 < 0 -> shifted to 0; cols: centre 998, 998 + 256 = 1254 > 1024 -> back by 230
    assert f((-0.9, 0.95), 1024, 1024, (512, 512)) == (0, 512, 512, 512)
    # odd size 7 x 5 on 100 x 100 at (0.5, -0.5): centres int(75.0) = 75 and int(25.0) = 25; 7 // 2 = 3 -> rows
    # 72:79 (75 + 7 - 3 = 79); 5 // 2 = 2 -> cols 23:28
    assert f((0.5, -0.5), 100, 100, (7, 5)) == (72, 23, 7, 5)
    # non-square 37 x 45 grid, 13 x 17 at (0.9, -1): rows int(1.9 / 2 * 37) = int(35.15) = 35 -> 29:42 > 37 ->
    # back by 5 -> 24:37; cols int(0) = 0 -> -8:9 -> shifted to 0:17
    assert f((0.9, -1.0), 37, 45, (13, 17)) == (24, 0, 13, 17)
    # the whole frame is its own window wherever the centre is
    assert f((0.3, -0.7), 37, 45, (37, 45)) == (0, 0, 37, 45)
    with pytest.raises(ValueError):
        f((0, 0), 37, 45, (38, 45))


def test_windows_outside_the_grid_are_rejected_on_the_host(stif):
    cw = stif.coords.check_window
    assert cw((0, 0, 37, 45), 37, 45) == (0, 0, 37, 45)
    assert cw([36, 44, 1, 1], 37, 45) == (36, 44, 1, 1)
    for bad in [(-1, 0, 3, 3), (0, -1, 3, 3), (0, 0, 0, 3), (0, 0, 3, 0), (35, 0, 3, 3), (0, 43, 3, 3), (0, 0, 38, 1),
                (1, 2, 3), "window"]:
        with pytest.raises(ValueError):
            cw(bad, 37, 45)
        if len(bad) == 4 and not isinstance(bad, str):
            with pytest.raises(ValueError):       # the ctypes descriptor is never built for it
                stif.ops.dec_window(bad, 37, 45)
    with pytest.raises(ValueError):
        stif.ops.dec_window((0, 0, 3, 3), 37, 45, frect=(0, 0, 38, 45))
    w = stif.ops.dec_window((9, 11, 13, 17), 37, 45, frect=(7, 9, 17, 21))
    assert (w.y0, w.x0, w.hh, w.ww, w.fy0, w.fx0, w.fh, w.fw) == (9, 11, 13, 17, 7, 9, 17, 21)
    assert (w.out_item, w.out_plane, w.out_pitch) == (0, 0, 0)


def test_tile_windows_cover_the_region_once(stif):
    tiles = stif.coords.tile_windows((2, 3, 37, 45), (16, 16))
    assert len(tiles) == 9 and tiles[0] == (2, 3, 16, 16) and tiles[-1] == (34, 35, 5, 13)
    seen = np.zeros((39, 48), int)
    for y0, x0, hh, ww in tiles:
        seen[y0:y0 + hh, x0:x0 + ww] += 1
    assert (seen[2:, 3:] == 1).all() and seen[:2].sum() == 0 and seen[:, :3].sum() == 0
    with pytest.raises(ValueError):
        stif.coords.tile_windows((0, 0, 4, 4), (0, 4))


def test_window_symbols_are_exported_and_declared(stif):
    lib = stif._lib.lib()
    for name in ("stif_dec_stage1_win", "stif_dec_stage2_win", "stif_dec_bounds"):
        assert hasattr(lib, name), name
        assert name in stif._lib.EXPORTS
    # the ctypes struct has the C layout: 8 ints, two 64-bit strides, the pitch (padded to 8 bytes)
    W = stif._lib.DecWindow
    assert C.sizeof(W) == 56 and W.out_item.offset == 32 and W.out_plane.offset == 40 and W.out_pitch.offset == 48


def test_window_entry_points_validate_before_launching(stif):
    """Every rejected call returns STIF_E_INVALID with a message and without touching the (fake) pointers."""
    L = stif._lib
    lib = L.lib()
    p = C.c_void_p(4096)                     # never dereferenced: validation comes first
    tab = L.DecTables(*[4096] * 14)          # hr_y / hr_x stay NULL
    HH, WW = 37, 45

    def s1(win, tab=tab, flow=p, hrf=p):
        return lib.stif_dec_stage1_win(p, p, C.byref(tab), None, p, hrf, flow, 1, 16, 20, HH, WW, 0, None, None,
                                       C.byref(win) if win is not None else None)

    def s2(win, out=p):
        return lib.stif_dec_stage2_win(p, p, p, p, C.byref(tab), None, p, out, 1, 16, 20, HH, WW, 0, None, None,
                                       C.byref(win) if win is not None else None)

    def bd(win, box=p):
        return lib.stif_dec_bounds(p, C.byref(tab), box, 1, HH, WW, None, C.byref(win) if win is not None else None)

    W = L.DecWindow
    bad = [
        ("query rectangle", W(30, 0, 13, 17)),                          # rows 30:43 of 37
        ("query rectangle", W(0, 40, 3, 6)),
        ("query rectangle", W(0, 0, 0, 5)),
        ("F rectangle", W(9, 11, 13, 17, 7, 9, 31, 21)),                # F rows 7:38 of 37
        ("out_pitch", W(9, 11, 13, 17, 0, 0, 0, 0, 3 * 13 * 16, 13 * 16, 16)),
    ]
    for what, win in bad:
        for fn in (s1, s2, bd):
            if what == "out_pitch" and fn is not s2:
                continue
            assert fn(win) == L.E_INVALID, (what, fn.__name__)
            assert what in lib.stif_last_error().decode(), (what, lib.stif_last_error())
    for fn in (s1, s2, bd):
        assert fn(None) == L.E_INVALID and b"null window" in lib.stif_last_error()
    # stage 1 stores every pixel's HRfeat row into the F layout: F must hold the query rectangle
    assert s1(W(9, 11, 13, 17, 10, 11, 13, 17)) == L.E_INVALID
    assert b"does not contain" in lib.stif_last_error()
    # the local ensemble's remap tables have no windowed form
    tab_hr = L.DecTables(*[4096] * 16)
    assert s1(W(9, 11, 13, 17), tab=tab_hr) == L.E_INVALID and b"hr_y" in lib.stif_last_error()
    # null buffers
    assert s1(W(9, 11, 13, 17), hrf=None) == L.E_INVALID
    assert s2(W(9, 11, 13, 17), out=None) == L.E_INVALID
    assert bd(W(9, 11, 13, 17), box=None) == L.E_INVALID


def test_whole_grid_entry_points_validate_before_launching(stif):
    """The whole-grid stage entry points (_ex and plain) reject every bad argument with STIF_E_INVALID and their one
    text before any launch; the (fake) pointers are never touched."""
    L = stif._lib
    lib = L.lib()
    A = 4096                                 # a fake address: validation comes first
    tab = L.DecTables(*[A] * 14)             # hr_y / hr_x stay NULL
    shape = dict(n=1, h=16, w=20, HH=37, WW=45)

    def s1(ex, tab=tab, img=None, **kw):
        a = dict(proj=A, mlp=A, t=A, hrfeat=A, flow=A, **shape)
        a.update(kw)
        head = (a["proj"], a["mlp"], C.byref(tab) if tab is not None else None,
                C.byref(img) if img is not None else None, a["t"], a["hrfeat"], a["flow"],
                a["n"], a["h"], a["w"], a["HH"], a["WW"])
        return lib.stif_dec_stage1_ex(*head, 0, None, None) if ex else lib.stif_dec_stage1(*head, None)

    def s2(ex, tab=tab, img=None, **kw):
        a = dict(proj=A, mlp=A, hrfeat=A, flow=A, t=A, out=A, **shape)
        a.update(kw)
        head = (a["proj"], a["mlp"], a["hrfeat"], a["flow"], C.byref(tab) if tab is not None else None,
                C.byref(img) if img is not None else None, a["t"], a["out"], a["n"], a["h"], a["w"], a["HH"], a["WW"])
        return lib.stif_dec_stage2_ex(*head, 0, None, None) if ex else lib.stif_dec_stage2(*head, None)

    def rejected(fn, text, ex, **kw):
        lib.stif_dec_blend4(None, None, None, 0, 0, 0, None)      # another text in the error slot first
        assert fn(ex, **kw) == L.E_INVALID, (text, ex, kw)
        assert lib.stif_last_error() == text, (lib.stif_last_error(), ex, kw)

    img_bad = L.DecImage(A, 64, 80, *[A] * 8)
    img_bad.wx0 = None                       # one null table
    img_noimg = L.DecImage(None, 64, 80, *[A] * 8)
    tab_hr_y = L.DecTables(*[A] * 15)        # hr_y without hr_x
    tab_hr_x = L.DecTables(*[A] * 14)
    tab_hr_x.hr_x = A                        # hr_x without hr_y
    tab_hole = L.DecTables(*[A] * 14)
    tab_hole.lin_x = None                    # one null table
    for fn, text, ptrs in ((s1, b"stif_dec_stage1: bad arguments", ("proj", "mlp", "t", "hrfeat", "flow")),
                           (s2, b"stif_dec_stage2: bad arguments", ("proj", "mlp", "hrfeat", "flow", "t", "out"))):
        for ex in (True, False):
            for name in ptrs:                # each null pointer in turn (a null flow included)
                rejected(fn, text, ex, **{name: None})
            rejected(fn, text, ex, tab=None)
            rejected(fn, text, ex, tab=tab_hole)
            for kw in (dict(n=0), dict(h=0), dict(w=0), dict(HH=1), dict(WW=1)):
                rejected(fn, text, ex, **kw)
            rejected(fn, text, ex, img=img_bad)
            rejected(fn, text, ex, img=img_noimg)
    for ex in (True, False):
        rejected(s1, b"stif_dec_stage1: bad arguments", ex, tab=tab_hr_y)
        rejected(s1, b"stif_dec_stage1: bad arguments", ex, tab=tab_hr_x)
    # the windowed stage 1 takes a null flow (the feat-only pass): its argument check passes and the window is
    # looked at next; a null hrfeat is still its own rejection
    W = L.DecWindow

    def s1w(win, flow, hrf=A):
        return lib.stif_dec_stage1_win(A, A, C.byref(tab), None, A, hrf, flow, 1, 16, 20, 37, 45, 0, None, None,
                                       C.byref(win) if win is not None else None)

    assert s1w(None, None) == L.E_INVALID
    assert lib.stif_last_error() == b"stif_dec_stage1_win: null window"
    assert s1w(W(30, 0, 13, 17), None) == L.E_INVALID
    assert lib.stif_last_error() == b"stif_dec_stage1_win: the query rectangle is not inside the HH x WW grid"
    assert s1w(W(9, 11, 13, 17), None, hrf=None) == L.E_INVALID
    assert lib.stif_last_error() == b"stif_dec_stage1_win: bad arguments (null pointer or empty shape)"
