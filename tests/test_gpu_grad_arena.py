"""stif_grad_pack and stif_rank_sum on the GPU, bit for bit against numpy.

grad_pack: every segment lands at its offset, the gap up to the next multiple of 4 floats and the arena's tail come out
as +0.0 (the arena starts as NaN), and the guard words around the arena keep their bits.  Sources sit at 0, 4, 8 and 12
bytes from a 16-byte boundary, so both the 16-byte and the dword load paths run; the sizes straddle the float4 (3, 4,
5), the wave (63, 64, 65), the chunk of 1024 (1025), many chunks (124416) and more chunks than the grid has workgroups
(more than 2 x 2^21 floats: every workgroup walks several chunks, and the 434-tensor case walks across segments).
rank_sum: a sequential float32 sum in rank order, on inputs where the order matters, up to more float4s than the grid
has lanes."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 4
GUARD_BITS = 0x7FC12345          # a NaN with a payload: any write would change it
GRID_PASS = 2048 * 1024          # floats the 2048 workgroups of both kernels cover with one chunk / one float4 each


def bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.int32)


def guarded(n):
    """[GUARD | n | GUARD] floats: the guards hold GUARD_BITS, the middle NaN; returns (buffer, middle view)."""
    buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=torch.float32, device="cuda")
    g = torch.tensor([GUARD_BITS] * GUARD, dtype=torch.int32, device="cuda").view(torch.float32)
    buf[:GUARD] = g
    buf[-GUARD:] = g
    return buf, buf[GUARD:GUARD + n]


def guards_intact(buf):
    b = bits(buf)
    return bool((b[:GUARD] == GUARD_BITS).all() and (b[-GUARD:] == GUARD_BITS).all())


def sources(sizes, seed):
    """One tensor per size, tensor i a view 4 * (i % 4) bytes past a 16-byte boundary (i % 4 == 0: aligned), with a
    few special values whose bits a copy must keep."""
    rng = np.random.default_rng(seed)
    out = []
    for i, n in enumerate(sizes):
        host = rng.standard_normal(n + 8).astype(np.float32)
        host[rng.integers(0, n + 8, 3)] = [-0.0, np.inf, np.float32(1e-42)]
        base = torch.from_numpy(host).cuda()
        assert base.data_ptr() % 16 == 0
        v = base[i % 4:i % 4 + n]
        assert v.data_ptr() % 16 == 4 * (i % 4) and v.is_contiguous()
        out.append(v)
    return out


def expected(srcs, total):
    ref = np.zeros(total, np.float32)
    off, offs = 0, []
    for s in srcs:
        n = s.numel()
        ref[off:off + n] = s.cpu().numpy()
        offs.append(off)
        off += (n + 3) // 4 * 4
    assert off <= total
    return ref, offs, off


def check_pack(stif, sizes, tail, seed):
    srcs = sources(sizes, seed)
    used = sum((n + 3) // 4 * 4 for n in sizes)
    total = used + tail
    buf, arena = guarded(total)
    table = stif.ops.grad_pack(srcs, arena)
    ref, offs, end = expected(srcs, total)
    assert table.offsets == offs and table.floats == end == used
    got = bits(arena)
    assert np.array_equal(got, ref.view(np.int32)), f"{int((got != ref.view(np.int32)).sum())} words differ"
    for o, n in zip(offs, sizes):                            # +0.0, sign bit included
        assert not got[o + n:o + (n + 3) // 4 * 4].any()
    assert not got[used:].any() and guards_intact(buf)
    return srcs, arena, buf, table, ref


def test_grad_pack_sizes_alignments_gaps_and_tail(stif):
    sizes = [1, 3, 4, 5, 63, 64, 65, 1025, 124416, 2 * GRID_PASS + 1028 + 1, 7, 1024, 2]
    srcs, arena, buf, table, ref = check_pack(stif, sizes, tail=2 * 1024 + 8, seed=1)
    # the table is built once per layout: the same tensors again upload nothing, new tensors of the same sizes only
    # their pointers
    arena.fill_(float("nan"))
    ptrs = table.ptrs
    again = stif.ops.grad_pack(srcs, arena, table)
    assert again is table and table.ptrs is ptrs
    assert np.array_equal(bits(arena), ref.view(np.int32)) and guards_intact(buf)
    moved = [s.clone() for s in srcs]
    arena.fill_(float("nan"))
    assert stif.ops.grad_pack(moved, arena, table) is table and table.ptrs != ptrs
    assert np.array_equal(bits(arena), ref.view(np.int32))
    other = stif.ops.grad_pack(moved[:3], arena, table)      # another layout: another table
    assert other is not table and other.sizes == (1, 3, 4)


def test_grad_pack_the_models_434_tensors(stif):
    spec = stif.weights.state_dict_spec()
    unused = ("upconv1.", "upconv2.", "HRconv.", "conv_last.")
    sizes = [int(np.prod(s)) for k, s in spec.items() if not k.startswith(unused)]
    assert len(sizes) == 434
    check_pack(stif, sizes, tail=0, seed=2)


def test_grad_pack_4096_one_float_segments(stif):
    check_pack(stif, [1] * 4096, tail=4, seed=3)


def test_grad_pack_refuses_what_it_cannot_pack(stif):
    a = torch.zeros(16, device="cuda")
    with pytest.raises(ValueError, match="needs 20 floats"):
        stif.ops.grad_pack([torch.zeros(17, device="cuda")], a)
    with pytest.raises(ValueError, match="tensor 0 must be a contiguous float32"):
        stif.ops.grad_pack([torch.zeros(4, 4, device="cuda").t()], a)
    with pytest.raises(ValueError, match="arena must be"):
        stif.ops.grad_pack([torch.zeros(4)], torch.zeros(16))
    with pytest.raises(stif._lib.StifError, match="arena must be 16-byte aligned"):
        stif.ops.grad_pack([torch.zeros(4, device="cuda")], torch.zeros(17, device="cuda")[1:])


def slab_case(R, n, row, seed):
    """Standard normal rows: terms of one scale and both signs, so that about a third of the three-term sums (and
    more of the longer ones) round differently in the reverse order."""
    rng = np.random.default_rng(seed)
    host = rng.standard_normal((R, row)).astype(np.float32)
    ref = host[0, :n].copy()
    for r in range(1, R):
        ref = ref + host[r, :n]
    rev = host[R - 1, :n].copy()
    for r in range(R - 2, -1, -1):
        rev = rev + host[r, :n]
    assert ref.dtype == np.float32
    return host, ref, rev


SUM_SIZES = [4, 1020, 1024, 1028, 1_000_004, GRID_PASS + 1028]


@pytest.mark.parametrize("R", [1, 2, 3, 8])
def test_rank_sum_is_the_sequential_sum_in_rank_order(stif, R):
    for n in SUM_SIZES:
        row = n + (8 if n == 1028 else 0)                    # once with rows wider than the sum
        host, ref, rev = slab_case(R, n, row, seed=100 * R + n % 97)
        if R >= 3:
            changed = float((ref.view(np.int32) != rev.view(np.int32)).mean()) if n >= 1020 else None
            if changed is not None:
                print(f"R {R} n {n}: reversing the rank order changes {100 * changed:.0f} % of the elements")
                assert changed > 0.25
        slab = torch.from_numpy(host).cuda()
        buf, dst = guarded(n)
        out = stif.ops.rank_sum(slab[:, :n], dst)
        assert out is dst
        first = bits(dst).copy()
        assert np.array_equal(first, ref.view(np.int32)), (R, n, int((first != ref.view(np.int32)).sum()))
        assert guards_intact(buf)
        dst.fill_(float("nan"))
        stif.ops.rank_sum(slab[:, :n], dst)
        assert np.array_equal(bits(dst), first), "two calls, the same bytes"
        assert np.array_equal(bits(slab), host.view(np.int32)), "the slab is only read"


def test_rank_sum_refuses_an_overlapping_destination(stif):
    slab = torch.zeros(3, 1024, device="cuda")
    with pytest.raises(stif._lib.StifError, match="dst overlaps slab"):
        stif.ops.rank_sum(slab, slab[1])
    with pytest.raises(ValueError, match="a slab row 1024"):
        stif.ops.rank_sum(slab, torch.zeros(1028, device="cuda"))
    with pytest.raises(stif._lib.StifError, match="multiple of 4"):
        stif.ops.rank_sum(slab, torch.zeros(1022, device="cuda"))
