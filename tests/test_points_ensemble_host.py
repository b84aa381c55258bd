"""Point queries of the local ensemble, the host side (no GPU): the three entry points are declared, exported and
bound, each rejects every invalid argument before any launch -- fake pointers (4096) that are never dereferenced, in
the manner of tests/dec_reject_cases.py -- ``return_flow`` with ``ensemble=True`` is a ValueError, and the plain point
entry points still reject the tables of a shifted query."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = 4096
NEW = ("stif_dec_remap_pts", "stif_dec_flow_pts", "stif_dec_stage2_blend_pts")
EX = ["flags", "status", "stream"]
ENTRIES = {
    "stif_dec_remap_pts": ["tab", "pts", "ry", "rx", "n", "HH", "WW", "status", "stream"],
    "stif_dec_flow_pts": ["proj", "mlp", "tab", "pts", "hrfeat", "flow", "n", "h", "w", "HH", "WW"] + EX,
    "stif_dec_stage2_blend_pts": ["proj", "mlp", "hrfeat", "flow", "tab", "pts", "out", "n", "h", "w", "HH", "WW"] + EX
    + ["blend"],
}
POINTERS = ("proj", "mlp", "hrfeat", "flow", "out", "ry", "rx")
NEEDS_REMAP = ("stif_dec_remap_pts", "stif_dec_flow_pts")


def base(L, name):
    """A valid value of argument ``name``: fake addresses, the 16 x 20 -> 37 x 45 shape, the tables of a shifted query."""
    if name in POINTERS:
        return A
    if name in ("status", "stream"):
        return None
    if name == "flags":
        return 0
    if name == "tab":
        return L.DecTables(*[A] * 16)
    if name == "pts":
        return L.DecPointList(A, A, A, 17, 17, 17, 1, 17)
    if name == "blend":
        return L.DecBlend(0, 0, (C.c_void_p * 4)(*[A] * 4), (C.c_void_p * 4)(*[A] * 4))
    return dict(n=2, h=16, w=20, HH=37, WW=45)[name]


def call(L, entry, **changed):
    """(return code, message) of ``entry`` with the valid arguments but for ``changed``; another text sits in the
    error slot first."""
    lib = L.lib()
    a = {name: base(L, name) for name in ENTRIES[entry]}
    for k, v in changed.items():
        assert k in a, (entry, k)
        a[k] = v
    argv = [C.byref(v) if isinstance(v, C.Structure) else v for v in a.values()]
    lib.stif_dec_blend4(None, None, None, 0, 0, 0, None)
    rc = getattr(lib, entry)(*argv)
    return rc, lib.stif_last_error().decode()


def rejected(L, entry, text, **changed):
    rc, err = call(L, entry, **changed)
    assert rc == L.E_INVALID, (entry, changed, rc, err)            # anything else would have launched
    assert err.startswith(entry + ": ") and text in err, (entry, changed, text, err)


def test_the_symbols_are_declared_exported_and_bound(stif):
    L = stif._lib
    hdr = open(os.path.join(REPO, "include", "stif.h")).read()
    declared = set(re.findall(r"^\s*int\s+(stif_\w+)\s*\(", hdr, re.M))
    for name in NEW:
        assert name in declared, name
        assert hasattr(L.lib(), name), name
        assert name in L.EXPORTS and L.EXPORTS[name][0] is C.c_int, name
        assert len(L.EXPORTS[name][1]) == len(ENTRIES[name]), name
    for name in ("dec_remap_pts", "dec_flow_pts", "dec_stage2_blend_pts"):
        assert callable(getattr(stif.ops, name)), name


@pytest.mark.parametrize("entry", NEW)
def test_entry_points_validate_before_launching(stif, entry):
    L = stif._lib
    args = ENTRIES[entry]
    for p in POINTERS:
        if p in args:
            rejected(L, entry, "null pointer", **{p: None})
    rejected(L, entry, "null pointer", tab=None)
    for field in ("near_y", "rel_x", "lin_x"):
        tab = base(L, "tab")
        setattr(tab, field, None)
        rejected(L, entry, "null pointer", tab=tab)
    rejected(L, entry, "n < 1" if entry == "stif_dec_remap_pts" else "empty shape", n=0)
    # the point list
    rejected(L, entry, "null point list", pts=None)
    for k in range(3):
        ptrs = [A, A, A]
        ptrs[k] = None
        rejected(L, entry, "null point list", pts=L.DecPointList(*ptrs, 17, 17, 17, 1, 17))
    for npts in (0, -3):
        rejected(L, entry, "npts < 1", pts=L.DecPointList(A, A, A, 17, 17, 17, 1, npts))
    rejected(L, entry, "exceeds INT_MAX", pts=L.DecPointList(A, A, A, 0, 0, 0, 0, 2 ** 27), n=2)
    rejected(L, entry, "exceeds INT_MAX", pts=L.DecPointList(A, A, A, 0, 0, 0, 0, 2 ** 30), n=1)
    for k in range(4):
        strides = [17, 17, 17, 1]
        strides[k] = -1
        rejected(L, entry, "negative point stride", pts=L.DecPointList(A, A, A, *strides, 17))
    for size in (dict(HH=1), dict(WW=1)):              # checked after the tables: the shifted ones were accepted
        rejected(L, entry, "bad virtual grid size", **size)
    # the remap tables, where they are required
    if entry in NEEDS_REMAP:
        rejected(L, entry, "hr_y / hr_x", tab=L.DecTables(*[A] * 14))
        rejected(L, entry, "hr_y / hr_x", tab=L.DecTables(*[A] * 15))
        only_x = L.DecTables(*[A] * 16)
        only_x.hr_y = None
        rejected(L, entry, "hr_y / hr_x", tab=only_x)
    else:                                               # the blending stage 2 takes either kind and reads neither
        rejected(L, entry, "bad virtual grid size", tab=L.DecTables(*[A] * 14), HH=1)
    # the blend
    if "blend" in args:
        rejected(L, entry, "null blend", blend=None)
        for k in (-1, 4):
            b = base(L, "blend")
            b.k = k
            rejected(L, entry, "blend k outside 0..3", blend=b)
        for acc in (-1, 2):
            b = base(L, "blend")
            b.accumulate = acc
            rejected(L, entry, "accumulate must be 0 or 1", blend=b)
        for tbl in ("rel_y", "rel_x"):
            for j in range(4):
                b = base(L, "blend")
                getattr(b, tbl)[j] = None
                rejected(L, entry, "null rel_y / rel_x", blend=b)


def test_return_flow_with_the_ensemble_is_refused_before_any_launch(stif, sd):
    """A CPU module with a stand-in latent: the check comes before anything touches the device."""
    m = stif.LunaTokis(64, 6, 8, 5, 40, device="cpu")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    m._feat = torch.zeros(3, 1, 16, 20, 64)
    m.inp = torch.zeros(1, 2, 3, 16, 20)
    with pytest.raises(ValueError, match="return_flow"):
        m.decoding_points(np.array([1, 2]), np.array([3, 4]), 0.5, ensemble=True, return_flow=True)
    with pytest.raises(ValueError, match="return_flow"):
        m.decoding_points(np.array([1, 2]), np.array([3, 4]), 0.5, pairs=[0], ensemble=True, return_flow=True)


def test_the_plain_point_entry_points_still_reject_shifted_tables(stif):
    L = stif._lib
    lib = L.lib()
    p = C.c_void_p(A)
    q = L.DecPointList(A, A, A, 17, 17, 17, 1, 17)
    for tab in (L.DecTables(*[A] * 16), L.DecTables(*[A] * 15)):
        calls = {
            "stif_dec_stage1_pts": lambda: lib.stif_dec_stage1_pts(p, p, C.byref(tab), C.byref(q), p, p, 2, 16, 20, 37,
                                                                   45, 0, None, None),
            "stif_dec_corners_pts": lambda: lib.stif_dec_corners_pts(p, C.byref(tab), C.byref(q), p, p, p, 2, 37, 45,
                                                                     None, None),
            "stif_dec_stage2_pts": lambda: lib.stif_dec_stage2_pts(p, p, p, p, C.byref(tab), C.byref(q), p, 2, 16, 20,
                                                                   37, 45, 0, None, None),
        }
        for me, fn in calls.items():
            lib.stif_dec_blend4(None, None, None, 0, 0, 0, None)
            assert fn() == L.E_INVALID, me
            err = lib.stif_last_error().decode()
            assert err.startswith(me + ": ") and "hr_y / hr_x" in err, err


def test_the_wrappers_refuse_the_wrong_kind_of_tables(stif):
    """ops.dec_remap_pts / dec_flow_pts need the tables of a shifted query, the plain point wrappers refuse them: both
    are decided from the host copy of the tables before anything is launched."""
    ops = stif.ops

    class Tab:
        shape = (16, 20, 37, 45)

        def __init__(self, shifted):
            self.shifted = shifted

    class Pts:
        n, npts = 2, 17

    with pytest.raises(ValueError, match="shifted query"):
        ops.dec_remap_pts(Tab(False), Pts(), 2, None, None)
    with pytest.raises(ValueError, match="shifted query"):
        ops.dec_flow_pts(torch.zeros(2, 16, 20, 256), None, Tab(False), Pts(), None, None)
    with pytest.raises(ValueError, match="no local-ensemble form"):
        ops.dec_stage1_pts(torch.zeros(2, 16, 20, 256), None, Tab(True), Pts(), None, None)
