"""Host-side query-grid tables of the implicit decoder, in the reference's fp32.

``LunaTokis.decoding`` (Sakuya_arch_test.py:364-459) samples the LR maps at
``coord_highres = make_coord((HH, WW)).clamp(-1+1e-6, 1-1e-6)`` (:373): a
separable meshgrid, so every discrete decision (nearest index with
round-half-to-even, bilinear corners) and every coordinate-derived value
(``rel_coord``, the ``warpgrid`` linspace base) depends on the HR row or column
only.  They are computed here once per (h, w, HH, WW) in float32 with the same
operation order as the reference (make_coord :1233-1248, grid_sample's
``((x + 1) * size - 1) / 2`` unnormalisation, torch.linspace), then uploaded;
the kernels only look them up.  This is what makes non-integer scales (2.5x,
where nearest-rounding ties occur) match the reference exactly.
"""
from __future__ import annotations

import numpy as np

F32 = np.float32
LO = F32(-1 + 1e-6)
HI = F32(1 - 1e-6)


def make_coord_1d(n: int) -> np.ndarray:
    """One axis of make_coord: fp32(-1 + r) + fp32(2r) * arange(n).float(), r = 1/n."""
    r = 2.0 / (2 * n)
    return (F32(2 * r) * np.arange(n, dtype=F32)).astype(F32) + F32(-1 + r)


def linspace_f32(n: int) -> np.ndarray:
    """torch.linspace(-1, 1, n) in fp32 (the warpgrid base grid, warplayer.py:27-31)."""
    if n == 1:
        return np.array([-1.0], F32)
    step = F32(2.0 / (n - 1))
    i = np.arange(n)
    lo = (F32(-1.0) + step * i.astype(F32)).astype(F32)
    hi = (F32(1.0) - step * (n - 1 - i).astype(F32)).astype(F32)
    return np.where(i < n // 2, lo, hi).astype(F32)


def _unnorm(c: np.ndarray, size: int) -> np.ndarray:
    return ((c + F32(1)) * F32(size) - F32(1)) / F32(2)


def axis_table(n_lr: int, n_hr: int, shift: float = 0.0) -> dict:
    """Per-HR-index sampling data along one axis (rows: n = H, HH; cols: n = W, WW).
    shift: the local ensemble's query offset v * (2 / n_lr / 2) + 1e-6 (Sakuya_arch_test.py:
    994-998), added in fp32 and re-clamped; rel_coord keeps the unshifted query (:1000-1002) and
    ``hr`` is the HR pixel nearest to the shifted query (grid_sample nearest of HRfeat, :1022)."""
    c = np.clip(make_coord_1d(n_hr), LO, HI)
    s = c if shift == 0.0 else np.clip((c + F32(shift)).astype(F32), LO, HI)
    lr_c = make_coord_1d(n_lr)
    src = _unnorm(s, n_lr)
    near = np.clip(np.rint(src), 0, n_lr - 1).astype(np.int32)      # nearest (round half even)
    rel = ((c - lr_c[near]) * F32(n_lr)).astype(F32)                  # rel_coord (:394-396)
    f0 = np.floor(src)
    i0 = f0.astype(np.int64)
    i1 = i0 + 1
    w1 = (src - f0).astype(F32)
    w0 = ((f0 + F32(1)) - src).astype(F32)
    v0 = (i0 >= 0) & (i0 < n_lr)
    v1 = (i1 >= 0) & (i1 < n_lr)
    return dict(
        near=near, rel=rel,
        b0=np.clip(i0, 0, n_lr - 1).astype(np.int32), b1=np.clip(i1, 0, n_lr - 1).astype(np.int32),
        w0=np.where(v0, w0, F32(0)).astype(F32), w1=np.where(v1, w1, F32(0)).astype(F32),
        lin=linspace_f32(n_hr),
        hr=np.clip(np.rint(_unnorm(s, n_hr)), 0, n_hr - 1).astype(np.int32),
    )


def dec_tables(h: int, w: int, HH: int, WW: int, shift=None, shift_grid=None) -> dict:
    """Tables of one decode; shift = (vx, vy) of the local ensemble (rows move by vx/h, cols by vy/w).
    shift_grid = (h0, w0): the grid whose half pixel the shift is (the latent's), where the map sampled is not the
    latent -- decoding_test's s-times upsampled image, sampled at the same shifted query as the latent."""
    h0, w0 = (h, w) if shift_grid is None else shift_grid
    sy, sx = (0.0, 0.0) if shift is None else (shift[0] * (2 / h0 / 2) + 1e-6, shift[1] * (2 / w0 / 2) + 1e-6)
    ty = axis_table(h, HH, sy)
    tx = axis_table(w, WW, sx)
    out = {}
    for k, v in ty.items():
        out[("near" if k == "near" else k) + "_y"] = v
    for k, v in tx.items():
        out[k + "_x"] = v
    return out


def first_index(table: np.ndarray, n: int) -> np.ndarray:
    """The inverse of a monotone index table for the gather-form adjoints of the training decoder: n + 1 entries,
    entry i the first position whose table value is >= i, so the positions that hold i are
    [first[i], first[i + 1])."""
    table = np.asarray(table)
    if table.size > 1 and (np.diff(table) < 0).any():
        raise ValueError("first_index: the table is not monotone")
    return np.searchsorted(table, np.arange(n + 1), side="left").astype(np.int32)


def dec_train_tables(h: int, w: int, HH: int, WW: int) -> dict:
    """The tables of a training decode under the field names of stif.h's stif_dec_train_geom: ``dec_tables`` without
    a shift (near_y, rel_y, by0, by1, wy0, wy1, lin_y and the same along x) plus the inverse tables of the nearest
    index and of the two bilinear corner indices per axis (near_y_first, by0_first, by1_first, ...)."""
    t = dec_tables(h, w, HH, WW)
    out = {}
    for ax, n in (("y", h), ("x", w)):
        for k in ("near", "rel", "lin"):
            out[f"{k}_{ax}"] = t[f"{k}_{ax}"]
        for k in ("b0", "b1", "w0", "w1"):
            out[f"{k[0]}{ax}{k[1]}"] = t[f"{k}_{ax}"]
        for name in (f"near_{ax}", f"b{ax}0", f"b{ax}1"):
            out[name + "_first"] = first_index(out[name], n)
    return out


TABLE_ORDER = ["near_y", "rel_y", "b0_y", "b1_y", "w0_y", "w1_y", "lin_y",
               "near_x", "rel_x", "b0_x", "b1_x", "w0_x", "w1_x", "lin_x"]


def ensemble_weights(h: int, w: int, HH: int, WW: int) -> list:
    """Per-HR-pixel blend weights of decoding_localensemble (:1003-1004, 1075-1084), in fp32 and the
    reference's order: area_k = |rel_y rel_x| + 1e-9 for shifts (vx, vy) in (-1,-1), (-1,1), (1,-1),
    (1,1); tot = sum of the four; decode k is weighted by the diagonally opposite area / tot."""
    areas = []
    for vx in (-1, 1):
        for vy in (-1, 1):
            t = dec_tables(h, w, HH, WW, (vx, vy))
            areas.append((np.abs(np.outer(t["rel_y"], t["rel_x"]).astype(F32)) + F32(1e-9)).astype(F32))
    tot = (((areas[0] + areas[1]).astype(F32) + areas[2]).astype(F32) + areas[3]).astype(F32)
    return [(areas[3 - k] / tot).astype(F32) for k in range(4)]


def classify_time_query(shape, B: int, HH: int, WW: int) -> tuple:
    """What an entry of ``times`` of this shape means for a latent of ``B`` items decoded at HH x WW:
    ``("vector", None)`` -- 1 or B elements, of any shape: one time for all items or one per item; or
    ``("field", (b, hh, ww))`` -- a time per output pixel: the tensor, reshaped to (b, hh, ww) (each 1 or the full
    size), broadcasts to [B, HH, WW].  Fields are [HH, WW], [B, HH, WW], [B, 1, HH, WW], any shape of up to three
    dims that broadcasts to [B, HH, WW] ([HH, 1], [B, HH, 1], [WW], ...) and the reference's own [B, HH * WW] (or
    [1, HH * WW]).  Anything else is a ValueError."""
    shape = tuple(int(s) for s in shape)
    numel = int(np.prod(shape, dtype=np.int64)) if shape else 1
    if numel in (1, B):
        return "vector", None
    full = (B, HH, WW)
    if len(shape) == 2 and shape[0] in (1, B) and shape[1] == HH * WW:   # times[c] of Sakuya_arch_test.py:397
        return "field", (shape[0], HH, WW)
    s3 = shape
    if len(s3) == 4 and s3[1] == 1:
        s3 = (s3[0],) + s3[2:]
    if len(s3) <= 3:
        s3 = (1,) * (3 - len(s3)) + s3
        if all(s in (1, f) for s, f in zip(s3, full)):
            return "field", s3
    raise ValueError(f"a time query of shape {shape} is neither 1 or {B} values nor a field that broadcasts to "
                     f"[{B}, {HH}, {WW}]")


def classify_point_query(y_shape, x_shape, t_shape, B: int) -> tuple:
    """What the arguments of ``decoding_points`` of these shapes mean for a latent of ``B`` items:
    ``(n, ys, xs, ts)`` -- n points per item, and for ``y``, ``x`` and ``times`` the two-dim shape (items, points)
    to view each as, a dim of 1 broadcasting: ys / xs are (1, n) for an [n] list shared by every item or (B, n) for
    a list per item; ts is (1, 1) for one value, (B, 1) for [B] (a time per item), (1, n) for [n] (a time per
    point, shared by the items) or (B, n).  A one-dim ``times`` of B elements is [B], also when B == n: a time per
    point that all items share has then to be given as [B, n] (or expanded).  Anything else is a ValueError."""
    B = int(B)

    def coord(shape, name):
        shape = tuple(int(s) for s in shape)
        if len(shape) == 1 and shape[0] >= 1:
            return (1, shape[0])
        if len(shape) == 2 and shape[0] == B and shape[1] >= 1:
            return shape
        raise ValueError(f"{name} of shape {shape} is neither [n] nor [{B}, n] with n >= 1")

    ys, xs = coord(y_shape, "y"), coord(x_shape, "x")
    n = ys[1]
    if xs[1] != n:
        raise ValueError(f"y holds {n} points per item, x {xs[1]}")
    t_shape = tuple(int(s) for s in t_shape)
    numel = int(np.prod(t_shape, dtype=np.int64)) if t_shape else 1
    if numel == 1:
        ts = (1, 1)
    elif t_shape == (B,):
        ts = (B, 1)
    elif t_shape == (n,):
        ts = (1, n)
    elif t_shape == (B, n):
        ts = (B, n)
    else:
        raise ValueError(f"times of shape {t_shape} is neither one value, [{B}], [{n}] nor [{B}, {n}]")
    return n, ys, xs, ts


def point_strides(shape2, strides) -> tuple:
    """(item, point) element strides of a tensor viewed as ``shape2`` (``classify_point_query``) with ``strides``:
    a dim of size 1 broadcasts (stride 0)."""
    return tuple(0 if s == 1 else int(st) for s, st in zip(shape2, strides))


def check_points(y, x, HH: int, WW: int) -> None:
    """IndexError unless every row of ``y`` is in [0, HH) and every column of ``x`` in [0, WW) (host arrays)."""
    for name, v, size in (("y", y, HH), ("x", x, WW)):
        v = np.asarray(v)
        if v.size and (int(v.min()) < 0 or int(v.max()) >= size):
            bad = v[(v < 0) | (v >= size)].reshape(-1)[0]
            raise IndexError(f"point {name} = {int(bad)} is outside the virtual grid axis of {size}")


def point_passes(B: int, n: int, chunk_px: int) -> tuple:
    """The passes of a point decode whose compact HRfeat (8 corner rows per point) stays within ``chunk_px`` rows
    per pass: ``(items, ranges)`` -- at most ``items`` items per pass, and the point ranges [p0, p1) of at most
    ``max(1, chunk_px // 8)`` points that cover [0, n)."""
    pp = max(1, int(chunk_px) // 8)
    ranges = [(p0, min(n, p0 + pp)) for p0 in range(0, n, pp)]
    return max(1, min(int(B), int(chunk_px) // (8 * min(n, pp)))), ranges


def row_time_field(HH: int, t: float, skew: float) -> np.ndarray:
    """A rolling-shutter style time field, [HH, 1] fp32: row y is decoded at t + skew * (y / (HH - 1) - 0.5)."""
    y = np.arange(HH, dtype=np.float64) / max(HH - 1, 1)
    return (float(t) + float(skew) * (y - 0.5)).astype(F32).reshape(HH, 1)


def check_window(window, HH: int, WW: int) -> tuple:
    """A window ``(y0, x0, hh, ww)`` of the virtual HH x WW grid as four ints; ValueError unless it is a
    non-empty rectangle inside the grid."""
    try:
        y0, x0, hh, ww = (int(v) for v in window)
    except (TypeError, ValueError):
        raise ValueError(f"window must be (y0, x0, hh, ww), got {window!r}") from None
    if y0 < 0 or x0 < 0 or hh < 1 or ww < 1 or y0 + hh > HH or x0 + ww > WW:
        raise ValueError(f"window {(y0, x0, hh, ww)} is not a non-empty rectangle of the {HH} x {WW} grid")
    return y0, x0, hh, ww


def tile_windows(region, tile) -> list:
    """The windows of at most ``tile = (th, tw)`` pixels that cover ``region = (y0, x0, hh, ww)``, row-major
    (the last tile of a row / column is ragged)."""
    y0, x0, hh, ww = region
    try:
        th, tw = (int(v) for v in tile)
    except (TypeError, ValueError):
        raise ValueError(f"tile must be (th, tw), got {tile!r}") from None
    if th < 1 or tw < 1:
        raise ValueError(f"tile must be at least 1 x 1, got {(th, tw)}")
    return [(y0 + i, x0 + j, min(th, hh - i), min(tw, ww - j)) for i in range(0, hh, th) for j in range(0, ww, tw)]


def window_from_center(center, HH: int, WW: int, size) -> tuple:
    """The reference zoom demo's rectangle (decoding_memory, Sakuya_arch_test.py:639-652) as a window
    ``(y0, x0, hh, ww)``: ``center`` is (row, col) in [-1, 1]^2, ``size`` the rectangle's (rows, cols).  Per
    axis the centre pixel is ``int((c + 1) / 2 * n)`` (truncation), the rectangle starts ``size // 2`` before it,
    and a rectangle that sticks out of the frame is shifted back inside (the low edge is tested first)."""
    out = []
    for c, n, s in zip(center, (HH, WW), size):
        n, s = int(n), int(s)
        if s < 1 or s > n:
            raise ValueError(f"window size {s} does not fit the grid axis of {n}")
        mid = int((float(c) + 1) / 2 * n)
        lo, hi = mid - s // 2, mid + s - s // 2
        if lo < 0:
            lo, hi = 0, hi - lo
        elif hi > n:
            lo, hi = lo - (hi - n), n
        out.append((lo, hi))
    (r0, r1), (c0, c1) = out
    return check_window((r0, c0, r1 - r0, c1 - c0), HH, WW)
