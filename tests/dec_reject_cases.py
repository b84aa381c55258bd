"""The rejection matrix of the decoder's C entry points: every stage entry point, stif_dec_bounds and
stif_dec_corners_pts, called with fake pointers under every single defect of a fixed list and every pair of two
defects that can be applied together.  ``record`` returns the return code and stif_last_error() text of every case;
tests/golden/make_dec_reject_golden.py writes that to dec_reject_matrix.json and tests/test_dec_reject_host.py replays
it.  Every case has to be rejected before any launch: the pointers (4096) are never dereferenced.

Which defects an entry gets is decided from its argument list (``needs``) and from the forms include/stif.h documents
as valid (``VALID``), never from what the library answers."""
import ctypes as C
import itertools

A = 4096
WIN = (9, 11, 13, 17)                       # of the 37 x 45 grid, as tests/test_window_host.py
S1 = ["proj", "mlp", "tab", "img", "t", "hrfeat", "flow", "n", "h", "w", "HH", "WW"]
S2 = ["proj", "mlp", "hrfeat", "flow", "tab", "img", "t", "out", "n", "h", "w", "HH", "WW"]
EX = ["flags", "status", "stream"]


def _sub(args, old, new):
    return [new if a == old else a for a in args]


# entry key -> argument names in call order.  "tf" / "pts": a stif_dec_time / stif_dec_points in the time slot;
# "nowin": the window argument of a time-field entry left NULL (its whole-grid form, keyed "<entry>:grid").
ENTRIES = {
    "stif_dec_stage1": S1 + ["stream"],
    "stif_dec_stage1_ex": S1 + EX,
    "stif_dec_stage1_win": S1 + EX + ["win"],
    "stif_dec_flow_win": S1 + EX + ["win"],
    "stif_dec_stage1_tf": _sub(S1, "t", "tf") + EX + ["win"],
    "stif_dec_stage1_tf:grid": _sub(S1, "t", "tf") + EX + ["nowin"],
    "stif_dec_stage1_pts": ["proj", "mlp", "tab", "pts", "hrfeat", "flow", "n", "h", "w", "HH", "WW"] + EX,
    "stif_dec_stage2": S2 + ["stream"],
    "stif_dec_stage2_ex": S2 + EX,
    "stif_dec_stage2_win": S2 + EX + ["win"],
    "stif_dec_stage2_blend_win": S2 + EX + ["blend", "win"],
    "stif_dec_stage2_tf": _sub(S2, "t", "tf") + EX + ["win"],
    "stif_dec_stage2_tf:grid": _sub(S2, "t", "tf") + EX + ["nowin"],
    "stif_dec_stage2_pts": ["proj", "mlp", "hrfeat", "flow", "tab", "pts", "out", "n", "h", "w", "HH", "WW"] + EX,
    "stif_dec_bounds": ["flow", "tab", "box", "n", "HH", "WW", "stream", "win"],
    "stif_dec_corners_pts": ["flow", "tab", "pts", "cy", "cx", "ct", "n", "HH", "WW", "status", "stream"],
}
POINTERS = ("proj", "mlp", "hrfeat", "flow", "t", "out", "box", "cy", "cx", "ct")
STRUCTS = ("tab", "img", "tf", "pts", "blend", "win")


def _base(L, name):
    """A valid value of argument ``name``: a fake address, the 16 x 20 -> 37 x 45 shape, or a descriptor of fakes."""
    if name in POINTERS:
        return A
    if name in ("img", "status", "stream", "nowin"):
        return None
    if name == "flags":
        return 0
    if name == "tab":
        return L.DecTables(*[A] * 14)            # hr_y / hr_x stay NULL
    if name == "tf":
        return L.DecTimeField(A, 37 * 45, 45, 1)
    if name == "pts":
        return L.DecPointList(A, A, A, 5, 5, 5, 1, 5)
    if name == "win":
        return L.DecWindow(*WIN)
    if name == "blend":
        return L.DecBlend(0, 0, (C.c_void_p * 4)(*[A] * 4), (C.c_void_p * 4)(*[A] * 4))
    return dict(n=1, h=16, w=20, HH=37, WW=45)[name]


def _set(name, value):
    def f(L, a):
        a[name] = value(L) if callable(value) else value
    return f


def _field(name, field, value, index=None):
    def f(L, a):
        if index is None:
            setattr(a[name], field, value)
        else:
            getattr(a[name], field)[index] = value
    return f


def _img_hole(L):
    im = L.DecImage(A, 64, 80, *[A] * 8)
    im.wx0 = None
    return im


def _hr(both):
    def f(L, a):
        a["tab"].hr_y = A
        a["tab"].hr_x = A if both else None
    return f


# (name, slot, the argument it needs, mutation).  Two defects whose slots are equal, or one a prefix of the other
# ("tab" and "tab.hr"), touch the same thing and are never paired.
DEFECTS = [(f"{p}=NULL", p, p, _set(p, None)) for p in POINTERS] + [
    ("tab=NULL", "tab", "tab", _set("tab", None)),
    ("tab.lin_x=NULL", "tab.lin_x", "tab", _field("tab", "lin_x", None)),
    ("n=0", "n", "n", _set("n", 0)),
    ("h=0", "h", "h", _set("h", 0)),
    ("w=0", "w", "w", _set("w", 0)),
    ("HH=1", "HH", "HH", _set("HH", 1)),
    ("WW=1", "WW", "WW", _set("WW", 1)),
    ("img with a null table", "img", "img", _set("img", _img_hole)),
    ("tab.hr_y only", "tab.hr", "tab", _hr(False)),
    ("tab.hr_y and hr_x", "tab.hr", "tab", _hr(True)),
    # the five bad windows of tests/test_window_host.py, a null one, an F that misses the query rectangle
    ("win rows 30:43", "win", "win", _set("win", lambda L: L.DecWindow(30, 0, 13, 17))),
    ("win cols 40:46", "win", "win", _set("win", lambda L: L.DecWindow(0, 40, 3, 6))),
    ("win hh=0", "win", "win", _set("win", lambda L: L.DecWindow(0, 0, 0, 5))),
    ("win F rows 7:38", "win", "win", _set("win", lambda L: L.DecWindow(9, 11, 13, 17, 7, 9, 31, 21))),
    ("win out_pitch<ww", "win", "win",
     _set("win", lambda L: L.DecWindow(9, 11, 13, 17, 0, 0, 0, 0, 3 * 13 * 16, 13 * 16, 16))),
    ("win=NULL", "win", "win", _set("win", None)),
    ("win F misses the query", "win", "win", _set("win", lambda L: L.DecWindow(9, 11, 13, 17, 10, 11, 13, 17))),
    ("blend=NULL", "blend", "blend", _set("blend", None)),
    ("blend.k=4", "blend.k", "blend", _field("blend", "k", 4)),
    ("blend.accumulate=2", "blend.accumulate", "blend", _field("blend", "accumulate", 2)),
    ("blend.rel_x[2]=NULL", "blend.rel_x", "blend", _field("blend", "rel_x", None, 2)),
    ("tf=NULL", "tf", "tf", _set("tf", None)),
    ("tf.t=NULL", "tf.t", "tf", _field("tf", "t", None)),
    ("tf.row=-1", "tf.row", "tf", _field("tf", "row", -1)),
    ("pts=NULL", "pts", "pts", _set("pts", None)),
    ("pts.y=NULL", "pts.y", "pts", _field("pts", "y", None)),
    ("pts.npts=0", "pts.npts", "pts", _field("pts", "npts", 0)),
    ("pts.x_item=-1", "pts.x_item", "pts", _field("pts", "x_item", -1)),
    ("pts.npts=2^28 (n * 8 * npts > INT_MAX)", "pts.npts", "pts", _field("pts", "npts", 1 << 28)),
]

# Forms stif.h documents as valid, so no defect of that entry point (by its C name):
_STAGE2 = ("stif_dec_stage2", "stif_dec_stage2_ex", "stif_dec_stage2_win", "stif_dec_stage2_blend_win")
VALID = {
    # flow = NULL is the feat-only pass of the windowed, time-field and point stage 1
    "flow=NULL": ("stif_dec_stage1_win", "stif_dec_stage1_tf", "stif_dec_stage1_pts"),
    # the remap is the whole-grid local ensemble's and what stif_dec_flow_win asks for; stage 2 with a scalar time
    # and stif_dec_bounds take a shifted query's tables and never read hr_y / hr_x
    "tab.hr_y and hr_x": ("stif_dec_stage1", "stif_dec_stage1_ex", "stif_dec_flow_win", "stif_dec_bounds") + _STAGE2,
    "tab.hr_y only": ("stif_dec_bounds",) + _STAGE2,
    # a time-field stage without a window is its whole-grid form (the ":grid" entries)
    "win=NULL": ("stif_dec_stage1_tf", "stif_dec_stage2_tf"),
    # only stage 1 stores into F; the others read what the flow asks for (status bit 1 / 2 reports a miss)
    "win F misses the query": ("stif_dec_flow_win", "stif_dec_stage2_win", "stif_dec_stage2_blend_win",
                               "stif_dec_stage2_tf", "stif_dec_bounds"),
}


def defects_of(key):
    fn = key.split(":")[0]
    return [d for d in DEFECTS if d[2] in ENTRIES[key] and fn not in VALID.get(d[0], ())]


def _clash(a, b):
    return a == b or a.startswith(b + ".") or b.startswith(a + ".")


def cases(key):
    """(names, defects) of every case of entry ``key``: the single defects, then the pairs, in list order."""
    ds = defects_of(key)
    for d in ds:
        yield (d[0],), (d,)
    for d, e in itertools.combinations(ds, 2):
        if not _clash(d[1], e[1]):
            yield (d[0], e[0]), (d, e)


def call(L, key, defects):
    """(return code, message) of entry ``key`` under ``defects``; another text sits in the error slot first."""
    lib = L.lib()
    a = {name: _base(L, name) for name in ENTRIES[key]}
    for d in defects:
        d[3](L, a)
    argv = [C.byref(v) if isinstance(v, C.Structure) else v for v in a.values()]
    lib.stif_dec_blend4(None, None, None, 0, 0, 0, None)
    rc = getattr(lib, key.split(":")[0])(*argv)
    return rc, lib.stif_last_error().decode()


def record(L, expect=None):
    """{"messages": [[rc, text], ...], "entries": {key: {" + ".join(names): index into messages}}}.  ``expect``: a
    matrix recorded earlier -- no case outside it, and none it records as anything but a rejection, is ever called."""
    messages, entries = [], {}
    for key in ENTRIES:
        out = entries[key] = {}
        for names, ds in cases(key):
            name = " + ".join(names)
            if expect is not None:
                assert expect["messages"][expect["entries"][key][name]][0] == L.E_INVALID, (key, name)
            got = list(call(L, key, ds))
            assert got[0] == L.E_INVALID, (key, name, got)       # anything else would have launched
            if got not in messages:
                messages.append(got)
            out[name] = messages.index(got)
    return {"messages": messages, "entries": entries}
