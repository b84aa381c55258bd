"""Data-parallel training, the host side (no GPU): data.rank_items and the rank slices of BatchLoader, the GradArena
layout of the 442-key model, the argument checks of stif_grad_pack / stif_rank_sum (fake pointers that are never
dereferenced, one changed argument at a time, as tests/test_deterministic_host.py), DataParallel's reduction with the
``dist`` calls captured -- staged through host memory under gloo, unstaged under nccl, all_reduce for "sum" and
all_gather + rank_sum for "ordered" -- and the first step's covered-set comparison, which must raise and name the keys
where ranks disagree."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest
import torch

import ddp_cases as DC

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = 4096


# ---- data ----

@pytest.mark.parametrize("batch,world", [(18, 8), (18, 4), (3, 2), (2, 2)])
def test_rank_items_cover_the_batch_exactly_once(stif, batch, world):
    D = stif.data
    spans = [D.rank_items(batch, world, r) for r in range(world)]
    assert list(itertools.chain.from_iterable(range(a, b) for a, b in spans)) == list(range(batch))
    sizes = [b - a for a, b in spans]
    assert max(sizes) - min(sizes) <= 1 and sizes == sorted(sizes, reverse=True)
    assert sizes[:batch % world] == [batch // world + 1] * (batch % world)


def test_rank_items_refuses_more_ranks_than_items(stif):
    with pytest.raises(ValueError, match="3 ranks cannot share a batch of 2"):
        stif.data.rank_items(2, 3, 0)
    with pytest.raises(ValueError):
        stif.data.rank_items(4, 2, 2)


@pytest.fixture(scope="module")
def footage(tmp_path_factory):
    return DC.write_footage(str(tmp_path_factory.mktemp("footage")))


@pytest.mark.parametrize("batch,world", [(3, 2), (4, 4)])
def test_a_ranks_batches_are_the_rows_of_the_single_process_batches(stif, footage, batch, world):
    D = stif.data
    index = D.ClipIndex(footage, ["clip_a", "clip_b"])
    assert len(index) == 6
    whole = D.BatchLoader(index, batch, seed=5, lq_size=16, workers=0, device=None)
    n = whole.per_epoch + 2                                  # across the boundary of the first two epochs
    ref = [whole.build(i) for i in range(n)]
    for rank in range(world):
        a, b = D.rank_items(batch, world, rank)
        mine = D.BatchLoader(index, batch, seed=5, lq_size=16, workers=0, device=None, rank=rank, world=world)
        assert mine.per_epoch == whole.per_epoch and mine.batch_size == batch
        for i in range(n):
            assert mine.plan(i) == whole.plan(i)
            got = mine.build(i)
            assert got["shape"] == ref[i]["shape"]
            for key in ("LQs", "GT"):
                assert got[key].shape[0] == b - a
                assert got[key].numpy().tobytes() == ref[i][key][a:b].contiguous().numpy().tobytes(), (key, i, rank)
            for s, t in zip(got["time"], ref[i]["time"]):
                assert s.numpy().tobytes() == t[a:b].contiguous().numpy().tobytes()
    # the threaded iterator yields the same bytes as build()
    it = iter(D.BatchLoader(index, batch, seed=5, lq_size=16, workers=2, device=None, rank=world - 1, world=world))
    first = next(it)
    it.close()
    a, b = D.rank_items(batch, world, world - 1)
    assert torch.equal(first["LQs"], ref[0]["LQs"][a:b])


def test_the_plan_of_one_process_is_unchanged(stif, footage):
    D = stif.data
    index = D.ClipIndex(footage, ["clip_a", "clip_b"])
    loader = D.BatchLoader(index, 2, seed=5, lq_size=16, workers=0, device=None)
    assert (loader.rank, loader.world, loader.items) == (0, 1, (0, 2))
    for i in range(4):
        paths, times, params = loader.plan(i)
        rng = D.stream_rng(5, "batch", i)
        assert params == D.draw_collate_params(rng, 72, 88, 16)
        perm = list(range(6))
        D.stream_rng(5, "epoch", i // 3).shuffle(perm)
        items = perm[(i % 3) * 2:(i % 3) * 2 + 2]
        want = [index.sample(k, rng) for k in items]
        assert paths == [p for p, _ in want] and times == [t for _, t in want]
    with pytest.raises(ValueError, match="ranks cannot share"):
        D.BatchLoader(index, 2, seed=5, lq_size=16, rank=0, world=3, device=None)


# ---- the arena's layout ----

def test_grad_arena_layout_of_the_442_key_model(stif):
    TR = stif.train
    net = TR.LunaTokis(5, 40)
    spec = stif.weights.state_dict_spec()
    arena = TR.GradArena(net.named_parameters())
    assert arena.names == list(spec) and len(arena.names) == 442
    sizes = [int(np.prod(s)) for s in spec.values()]
    assert arena.sizes == sizes
    assert all(o % 4 == 0 for o in arena.offsets) and arena.offsets[0] == 0
    assert all(b - a == (n + 3) // 4 * 4 for a, b, n in zip(arena.offsets, arena.offsets[1:], sizes))
    assert arena.total == sum((n + 3) // 4 * 4 for n in sizes) == arena.arena.numel()
    assert arena.arena.dtype == torch.float32 and not bool(arena.arena.any())
    views = arena.views()
    base = arena.arena.data_ptr()
    for v, o, (k, p) in zip(views, arena.offsets, net.named_parameters()):
        assert v.shape == p.shape and v.is_contiguous() and v.data_ptr() == base + 4 * o, k
    views[3].fill_(2.0)
    assert float(arena.arena[arena.offsets[3]]) == 2.0
    arena.assign()
    assert all(p.grad.data_ptr() == v.data_ptr() for p, v in zip(net.parameters(), views))
    # the chunk prefix of the device table: ceil(n / 1024) chunks per segment
    chunk0 = arena.table.host[:, 3].tolist()
    assert chunk0[0] == 0 and all(b - a == -(-n // 1024) for a, b, n in zip(chunk0, chunk0[1:], sizes))
    assert arena.table.host[:, 1].tolist() == arena.offsets and arena.table.host[:, 2].tolist() == sizes


def test_pack_names_a_covered_parameter_without_a_gradient(stif):
    TR = stif.train
    ps = [("a", torch.nn.Parameter(torch.zeros(5))), ("b", torch.nn.Parameter(torch.zeros(3)))]
    arena = TR.GradArena(ps)
    assert arena.offsets == [0, 8] and arena.total == 12
    ps[0][1].grad = torch.ones(5)
    with pytest.raises(RuntimeError, match="received no gradient.*: b"):
        arena.pack()


# ---- the C ABI ----

def rejected(L, name, args, text):
    lib = L.lib()
    lib.stif_dec_blend4(None, None, None, 0, 0, 0, None)   # another text sits in the error slot first
    rc = getattr(lib, name)(*args)
    err = lib.stif_last_error().decode()
    assert rc == L.E_INVALID, (name, args, rc, err)        # anything else would have launched
    assert err.startswith(name + ": ") and text in err, (name, text, err)


def test_the_symbols_are_declared_exported_and_bound(stif):
    L = stif._lib
    hdr = open(os.path.join(REPO, "include", "stif.h")).read()
    for name, nargs in (("stif_grad_pack", 5), ("stif_rank_sum", 6)):
        m = re.search(r"^\s*int\s+%s\s*\(([^;]*)\);" % name, hdr, re.M)
        assert m and len(m.group(1).split(",")) == nargs, name
        assert hasattr(L.lib(), name) and len(L.EXPORTS[name][1]) == nargs and L.EXPORTS[name][0] is C.c_int
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct \{([^}]*)\} stif_grad_seg;", hdr).group(1), flags=re.S)
    assert re.findall(r"(\w+)\s*;", body) == ["src", "dst", "n", "chunk0"]
    assert int(re.search(r"#define STIF_GRAD_CHUNK (\d+)", hdr).group(1)) == L.GRAD_CHUNK
    assert L.GRAD_MAX_SEGS >= 4096 and L.RANK_SUM_MAX_RANKS == 64
    assert callable(stif.ops.grad_pack) and callable(stif.ops.rank_sum)
    src = open(os.path.join(REPO, "stif-continuous-video-representation_amd", "csrc", "grad_arena.hip")).read()
    code = re.sub(r"//[^\n]*|/\*.*?\*/", "", src, flags=re.S)
    assert not re.search(r"atomic|__shared__|asm", code, re.I), "plain loads, adds and stores only"


def pack_args(**changed):
    a = dict(segs=A, nseg=434, arena=A, arena_floats=1 << 20, stream=None)
    a.update(changed)
    return list(a.values())


PACK_BAD = [(dict(segs=None), "null pointer"), (dict(arena=None), "null pointer"), (dict(nseg=0), "nseg must be >= 1"),
            (dict(nseg=-3), "nseg must be >= 1"), (dict(nseg=(1 << 20) + 1), "STIF_GRAD_MAX_SEGS"),
            (dict(arena=A + 4), "arena must be 16-byte aligned"), (dict(arena=A + 8), "arena must be 16-byte aligned"),
            (dict(segs=A + 4), "8-byte aligned"), (dict(arena_floats=0), "positive multiple of 4"),
            (dict(arena_floats=1022), "positive multiple of 4"), (dict(arena_floats=-4), "positive multiple of 4"),
            (dict(arena_floats=2 ** 31), "<= 2^31 - 1")]


@pytest.mark.parametrize("changed,text", PACK_BAD, ids=[f"{list(c)[0]}-{i}" for i, (c, _) in enumerate(PACK_BAD)])
def test_grad_pack_rejections(stif, changed, text):
    rejected(stif._lib, "stif_grad_pack", pack_args(**changed), text)


def sum_args(**changed):
    a = dict(slab=A, row=1024, R=3, dst=A + 4 * 4096, n=1024, stream=None)
    a.update(changed)
    return list(a.values())


SUM_BAD = [(dict(slab=None), "null pointer"), (dict(dst=None), "null pointer"), (dict(R=0), "R must be in 1 .. 64"),
           (dict(R=65), "R must be in 1 .. 64"), (dict(n=0), "positive multiple of 4"), (dict(n=1022), "positive multiple of 4"),
           (dict(n=1028), "row_floats < n"), (dict(row=1026, n=1024), "row_floats must be a multiple of 4"),
           (dict(n=2 ** 31, row=2 ** 31), "<= 2^31 - 1"), (dict(slab=A + 4), "16-byte aligned"),
           (dict(dst=A + 4 * 4096 + 8), "16-byte aligned"),
           (dict(dst=A), "dst overlaps slab"), (dict(dst=A + 4 * 2048), "dst overlaps slab"),
           (dict(dst=A + 4 * 3068), "dst overlaps slab"), (dict(dst=A - 4 * 1020), "dst overlaps slab")]


@pytest.mark.parametrize("changed,text", SUM_BAD, ids=[f"{list(c)[0]}-{i}" for i, (c, _) in enumerate(SUM_BAD)])
def test_rank_sum_rejections(stif, changed, text):
    rejected(stif._lib, "stif_rank_sum", sum_args(**changed), text)


def test_rank_sum_overlap_is_exact_at_both_ends(stif):
    """dst ending where the slab begins, or beginning where the last row's n floats end, does not overlap: those calls
    pass the checks (they would launch, so only the complementary cases are called here)."""
    rejected(stif._lib, "stif_rank_sum", sum_args(dst=A - 4 * 1024 + 16), "dst overlaps slab")
    rejected(stif._lib, "stif_rank_sum", sum_args(dst=A + 4 * (2 * 1024 + 1024) - 16), "dst overlaps slab")


# ---- the reduction, with dist captured ----

class FakeDist:
    """The calls DataParallel makes, recorded; ``peers`` holds what the other ranks contribute (rank -> 1-d tensor)."""

    def __init__(self, TR, monkeypatch, backend, rank, world, peers=None):
        self.calls, self.rank, self.world, self.peers = [], rank, world, peers or {}
        d = TR.dist
        monkeypatch.setattr(d, "is_initialized", lambda: True)
        monkeypatch.setattr(d, "get_backend", lambda group=None: backend)
        monkeypatch.setattr(d, "get_world_size", lambda group=None: world)
        monkeypatch.setattr(d, "get_rank", lambda group=None: rank)
        monkeypatch.setattr(d, "barrier", lambda group=None: self.calls.append(("barrier", None)))
        monkeypatch.setattr(d, "broadcast", self.broadcast)
        monkeypatch.setattr(d, "all_reduce", self.all_reduce)
        monkeypatch.setattr(d, "all_gather", self.all_gather)
        monkeypatch.setattr(d, "all_gather_into_tensor", self.all_gather_into_tensor)
        monkeypatch.setattr(d, "all_gather_object", self.all_gather_object)
        monkeypatch.setattr(TR.dist.distributed_c10d, "_get_default_group", lambda: self)

    def broadcast(self, t, src, group=None):
        self.calls.append(("broadcast", t))

    def all_reduce(self, t, op=None, group=None):
        self.calls.append(("all_reduce", t))
        for r in sorted(self.peers):
            t += self.peers[r]

    def _row(self, r, mine):
        return mine if r == self.rank else self.peers[r].to(mine.dtype).reshape(mine.shape)

    def all_gather(self, outs, t, group=None):
        self.calls.append(("all_gather", t, outs))
        for r, o in enumerate(outs):
            o.copy_(self._row(r, t))

    def all_gather_into_tensor(self, out, t, group=None):
        self.calls.append(("all_gather_into_tensor", t, out))
        for r in range(self.world):
            out[r].copy_(self._row(r, t))

    def all_gather_object(self, outs, obj, group=None):
        self.calls.append(("all_gather_object", obj))
        for r in range(self.world):
            outs[r] = obj if r == self.rank else self.peers[r]


def tiny(TR):
    net = torch.nn.Sequential(torch.nn.Linear(3, 5), torch.nn.Linear(5, 2))      # 15 + 5 + 10 + 2 floats
    opt = torch.optim.SGD(net.parameters(), lr=0.5)
    return net, opt


def sequential_rank_sum(slab, dst):
    acc = slab[0].clone()
    for r in range(1, slab.shape[0]):
        acc = acc + slab[r]
    dst.copy_(acc)
    return dst


@pytest.mark.parametrize("backend", ["gloo", "nccl"])
@pytest.mark.parametrize("mode", ["sum", "ordered"])
def test_the_reduction_is_staged_under_gloo_and_unstaged_under_nccl(stif, monkeypatch, backend, mode):
    TR = stif.train
    net, opt = tiny(TR)
    world, rank = 3, 1
    N = 16 + 8 + 12 + 4
    g = torch.Generator().manual_seed(3)
    peers = {0: torch.randn(N, generator=g), 2: torch.randn(N, generator=g)}
    fake = FakeDist(TR, monkeypatch, backend, rank, world, peers)
    monkeypatch.setattr(TR.ops, "rank_sum", sequential_rank_sum)
    dp = TR.DataParallel(net, opt, reduce=mode)
    assert (dp.world, dp.rank) == (3, 1)
    kinds = [c[0] for c in fake.calls]
    assert kinds.count("broadcast") == 4                    # rank 0's parameters, per tensor
    assert (kinds[0] == "barrier") == (backend == "nccl")   # warm_group before the first collective, nccl only
    fake.calls.clear()
    dp.arena = TR.GradArena(net.named_parameters())
    assert dp.arena.total == N
    mine = torch.randn(N, generator=g)
    dp.arena.arena.copy_(mine)
    dp._reduce()
    a = dp.arena.arena
    assert len(fake.calls) == 1                             # one exchange for all gradients
    call = fake.calls[0]
    if mode == "sum":
        assert call[0] == "all_reduce"
        want = (mine + peers[0]) + peers[2]
    else:
        assert call[0] == ("all_gather" if backend == "gloo" else "all_gather_into_tensor")
        want = (peers[0] + mine) + peers[2]                 # rank order, whatever this rank's number
        out = call[2]
        rows_ = out if torch.is_tensor(out) else torch.stack(list(out))
        assert tuple(rows_.shape) == (world, N)
    assert torch.equal(a, want)
    sent = call[1]
    assert sent.numel() == N and sent.dtype == torch.float32 and sent.is_contiguous()
    if backend == "nccl":
        assert sent.data_ptr() == a.data_ptr()              # the arena itself: no copy
        if mode == "ordered":
            assert call[2].data_ptr() == dp._slab.data_ptr()
    else:
        assert sent.data_ptr() != a.data_ptr() and sent.device.type == "cpu" and sent.data_ptr() == dp._host.data_ptr()
    # the default follows the switch
    dp.reduce = None
    assert dp._mode() == "sum"
    with TR.deterministic():
        assert dp._mode() == "ordered"
    with pytest.raises(ValueError, match="reduce must be"):
        TR.DataParallel(net, opt, reduce="mean")


def test_world_one_needs_no_process_group(stif):
    TR = stif.train
    net, opt = tiny(TR)
    dp = TR.DataParallel(net, opt)
    assert (dp.world, dp.rank, dp.distributed) == (1, 0, False)
    with pytest.raises(RuntimeError, match="no step taken"):
        dp.global_loss()


def test_global_loss_adds_in_rank_order(stif, monkeypatch):
    TR = stif.train
    net, opt = tiny(TR)
    vals = {0: torch.tensor([1e8]), 2: torch.tensor([-1e8])}
    FakeDist(TR, monkeypatch, "gloo", 1, 3, vals)
    dp = TR.DataParallel(net, opt)
    dp._loss = torch.tensor(3.0)
    want = (np.float32(1e8) + np.float32(3.0)) + np.float32(-1e8)
    assert dp.global_loss() == float(want) and float(want) != 3.0


# ---- the first step's covered set ----

def test_a_covered_set_mismatch_raises_and_names_the_keys(stif, monkeypatch):
    TR = stif.train
    net, opt = tiny(TR)
    every = [k for k, _ in net.named_parameters()]
    assert every == ["0.weight", "0.bias", "1.weight", "1.bias"]
    # the other rank froze 0.bias: its hash differs, and it reports that key as left out
    frozen = [k for k in every if k != "0.bias"]
    fake = FakeDist(TR, monkeypatch, "gloo", 0, 2, {1: torch.tensor([TR._names_hash(every)])})
    TR.check_covered_set(every, every)                       # agreement first: rank 1 sends the same hash
    assert [c[0] for c in fake.calls] == ["all_gather"] and fake.calls[0][1].numel() == 1
    # disagreement
    fake.peers[1] = torch.tensor([TR._names_hash(frozen)])
    fake.calls.clear()
    orig = fake.all_gather_object
    monkeypatch.setattr(TR.dist, "all_gather_object",
                        lambda outs, obj, group=None: (orig(outs, obj), outs.__setitem__(1, ["0.bias"]))[0])
    with pytest.raises(RuntimeError, match=r"ranks disagree.*rank 0: -; rank 1: 0\.bias"):
        TR.check_covered_set(every, every)
    assert [c[0] for c in fake.calls] == ["all_gather", "all_gather_object"]


def test_data_parallel_step_raises_on_the_first_step_where_one_rank_froze_a_parameter(stif, monkeypatch):
    """Through DataParallel.step itself on the CPU: the comparison comes before the first pack, so nothing of the
    GPU path is reached."""
    TR = stif.train
    net, opt = tiny(TR)
    every = [k for k, _ in net.named_parameters()]
    fake = FakeDist(TR, monkeypatch, "gloo", 1, 2, {0: torch.tensor([TR._names_hash(every)])})
    orig = fake.all_gather_object
    monkeypatch.setattr(TR.dist, "all_gather_object",
                        lambda outs, obj, group=None: (orig(outs, obj), outs.__setitem__(0, []))[0])
    net[0].bias.requires_grad_(False)                        # this rank freezes one parameter
    dp = TR.DataParallel(net, opt)
    x, y = torch.ones(4, 3), torch.zeros(4, 2)
    with pytest.raises(RuntimeError, match=r"rank 0: -; rank 1: 0\.bias"):
        dp.step(lambda out, gt: ((out - gt) ** 2).sum(), (x,), y)
    assert dp.arena is None


def test_the_training_script_documents_the_launch(stif):
    doc = open(os.path.join(REPO, "tools", "train.py")).read()
    assert "torch.distributed.run" in doc and "--backend" in doc and "Not built: DDP" not in doc
