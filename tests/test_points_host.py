"""Point queries, the host side: the shape / stride rule of decoding_points' arguments, the point-pass planner and the
index check of host data (no GPU)."""
import numpy as np
import pytest


def test_shapes_of_points_and_times(stif):
    cq = stif.coords.classify_point_query
    B, n = 3, 7
    assert cq((n,), (n,), (), B) == (n, (1, n), (1, n), (1, 1))            # shared points, one time
    assert cq((B, n), (n,), (1,), B) == (n, (B, n), (1, n), (1, 1))        # y per item, x shared
    assert cq((B, n), (B, n), (B,), B) == (n, (B, n), (B, n), (B, 1))      # a time per item
    assert cq((n,), (n,), (n,), B) == (n, (1, n), (1, n), (1, n))          # a time per point
    assert cq((n,), (B, n), (B, n), B) == (n, (1, n), (B, n), (B, n))
    assert cq((1,), (1,), (), 1) == (1, (1, 1), (1, 1), (1, 1))
    assert cq((n,), (n,), (n,), 1) == (n, (1, n), (1, n), (1, n))          # B = 1: [n] is per point


def test_a_vector_of_B_times_is_per_item_when_B_equals_n(stif):
    cq = stif.coords.classify_point_query
    assert cq((4,), (4,), (4,), 4) == (4, (1, 4), (1, 4), (4, 1))
    assert cq((4,), (4,), (4, 4), 4)[3] == (4, 4)                          # per point needs the explicit [B, n]


@pytest.mark.parametrize("ys,xs,ts", [
    ((7,), (6,), ()),            # y and x disagree
    ((2, 7), (7,), ()),          # a leading dim that is not B
    ((3, 7, 1), (7,), ()),       # three dims
    ((0,), (0,), ()),            # no points
    ((7,), (7,), (5,)),          # neither B nor n times
    ((7,), (7,), (7, 3)),        # [n, B]
    ((7,), (7,), (1, 7)),        # only [B, n] has two dims
])
def test_rejected_shapes(stif, ys, xs, ts):
    with pytest.raises(ValueError):
        stif.coords.classify_point_query(ys, xs, ts, 3)


def test_strides_with_broadcasts(stif):
    ps = stif.coords.point_strides
    assert ps((1, 7), (7, 1)) == (0, 1)
    assert ps((3, 7), (7, 1)) == (7, 1)
    assert ps((3, 7), (0, 1)) == (0, 1)          # an expanded item dim
    assert ps((3, 1), (1, 1)) == (1, 0)          # [B] times: no point stride
    assert ps((1, 1), (1, 1)) == (0, 0)
    assert ps((3, 7), (20, 2)) == (20, 2)        # a strided view (times only: y / x need unit point stride)


def test_point_passes_for_a_small_chunk(stif):
    pp = stif.coords.point_passes
    assert pp(2, 437, 2 ** 25) == (2, [(0, 437)])                           # everything in one pass
    items, ranges = pp(2, 437, 8 * 64)                                       # 64 points per pass, one item each
    assert items == 1
    assert ranges == [(0, 64), (64, 128), (128, 192), (192, 256), (256, 320), (320, 384), (384, 437)]
    assert pp(5, 10, 8 * 25) == (2, [(0, 10)])                               # 2 items x 10 points x 8 rows <= 200
    assert pp(3, 5, 1) == (1, [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5)])      # never less than a point
    for B, n, chunk in ((2, 437, 512), (7, 100, 4096), (3, 5, 1), (4, 9, 8 * 9 * 4)):
        items, ranges = pp(B, n, chunk)
        assert 1 <= items <= B
        assert [r[0] for r in ranges] == [0] + [r[1] for r in ranges[:-1]] and ranges[-1][1] == n
        m = max(p1 - p0 for p0, p1 in ranges)
        assert items * m * 8 <= max(chunk, 8 * m)                            # the bound, but for one item's one pass


def test_host_indices_are_checked(stif):
    cp = stif.coords.check_points
    cp([0, 36], [0, 44], 37, 45)
    cp(np.array([[0, 36], [5, 6]]), np.array([44, 0]), 37, 45)
    cp((), (), 37, 45)
    with pytest.raises(IndexError, match="y = 37"):
        cp([0, 37], [0, 0], 37, 45)
    with pytest.raises(IndexError, match="x = -1"):
        cp([0, 1], np.array([3, -1]), 37, 45)
    with pytest.raises(IndexError, match="x = 45"):
        cp(np.zeros((2, 3), np.int64), np.array([[0, 1, 2], [3, 45, 5]]), 37, 45)


def test_the_abi_has_the_point_entry_points(stif):
    import ctypes as C
    L = stif._lib
    for name in ("stif_dec_stage1_pts", "stif_dec_corners_pts", "stif_dec_stage2_pts"):
        assert name in L.EXPORTS and hasattr(L.lib(), name)
    # stif_dec_points: three pointers, four 64-bit strides, one int (padded to 8)
    assert C.sizeof(L.DecPointList) == 3 * 8 + 4 * 8 + 8
    assert L.DecPointList.npts.offset == 56
