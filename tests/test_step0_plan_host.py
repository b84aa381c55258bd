"""The planner of the BiConvLSTM's per-frame first step (model.step0_plan) and the per-set item table of the launch
structs, without a GPU: which frames a chunk's two recurrences continue from, which weight sets every launch
around step 0 carries and how many items each set holds -- for chunks of 1, 2 and 6 pairs of a window and for a
batch of unrelated pairs."""
import ctypes as C

import pytest


@pytest.fixture(scope="module")
def plan(stif):
    return stif.model.step0_plan


@pytest.mark.parametrize("pairs", [1, 2, 6])
def test_window_chunk_runs_step0_once_per_frame(plan, pairs):
    p = plan(pairs, True)
    B, F = pairs, pairs + 1
    assert p["frames"] == F
    # pair b: forward from frame b, reversed from frame b + 1
    assert p["fwd"] == (0, B) and p["rev"] == (1, F)
    assert [range(*p["fwd"])[b] for b in range(B)] == list(range(B))
    assert [range(*p["rev"])[b] for b in range(B)] == list(range(1, F))
    la = p["launches"]
    assert list(la) == ["first_pcd", "first_fusion", "input_pyramid", "step0_pcd", "step0_fusion", "step0_cell",
                        "step1_pyramid"]
    assert la["first_pcd"] == [B, B] and la["first_fusion"] == [B]
    assert la["input_pyramid"] == [F, F]                    # (pcd_h, pcd_c) of the frames
    assert la["step0_pcd"] == [F] * 4                       # (pcd, alignment direction)
    assert p["zero_l1"] == (1, 3)                           # the alignments whose L1 input is the zero state
    assert la["step0_fusion"] == [F, F] and la["step0_cell"] == [F]
    assert la["step1_pyramid"] == [F, F, B, B]              # h0, c0 per frame; the middle latent per pair
    assert all(0 < len(c) <= 16 and min(c) >= 1 for c in la.values())


@pytest.mark.parametrize("pairs", [1, 2, 6])
def test_unrelated_pairs_keep_the_per_pair_step0(plan, pairs):
    p = plan(pairs, False)
    B = pairs
    assert p["frames"] is None and p["fwd"] is None and p["rev"] is None
    la = p["launches"]
    assert la["first_pcd"] == [B, B] and la["first_fusion"] == [B]
    assert la["input_pyramid"] == [B] * 6                   # (pcd, input)
    assert la["step0_pcd"] == [B] * 8                       # (pcd, direction, alignment direction)
    assert p["zero_l1"] == (1, 3, 5, 7)
    assert la["step0_fusion"] == [B] * 4 and la["step0_cell"] == [B, B]
    assert la["step1_pyramid"] == [B] * 4


def test_step0_items_window_against_pairs(plan):
    """What the window form saves, in items: step 0's sets hold pairs + 1 items where the per-pair form holds
    2 pairs per (pcd, alignment direction)."""
    for B in (1, 2, 6):
        w, q = plan(B, True)["launches"], plan(B, False)["launches"]
        for name in ("step0_pcd", "step0_fusion", "step0_cell"):
            assert sum(q[name]) == 2 * B * len(w[name]) and sum(w[name]) == (B + 1) * len(w[name])
        assert sum(q["input_pyramid"]) + sum(q["step1_pyramid"]) == 10 * B
        assert sum(w["input_pyramid"]) + sum(w["step1_pyramid"]) == 4 * (B + 1) + 2 * B


def test_plan_rejects_empty_chunk(plan):
    with pytest.raises(ValueError):
        plan(0, True)


def test_structs_carry_sixteen_sets_and_a_prefix_table(stif):
    L = stif._lib
    assert L.MAXG == 16
    for S, ptrs in ((L.ConvArgs, 7), (L.DcnArgs, 5), (L.DcnSepArgs, 7)):
        a = S()
        assert len(a.item_base) == 17 and not any(a.item_base)          # all zeros: the uniform form
        assert 0 <= C.sizeof(S) - (S.item_base.offset + 17 * 4) < 8     # the struct's last field
        assert C.sizeof(S) >= ptrs * 16 * 8 + 17 * 4


def test_set_items_fills_uniform_or_prefix_form(stif):
    L, ops = stif._lib, stif.ops
    a = L.ConvArgs()
    assert ops._set_items(a, [3, 3, 3]) == 9
    assert (a.ngroups, a.nitems) == (3, 3) and not any(a.item_base)
    b = L.DcnSepArgs()
    assert ops._set_items(b, [6, 6, 7, 7]) == 26
    assert b.ngroups == 4 and list(b.item_base)[:6] == [0, 6, 12, 19, 26, 0]
