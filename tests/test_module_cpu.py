"""Host-side (no GPU) coverage of the model API as an nn.Module and of the f16x3 weight-range guard
at packing time (the packers run on the CPU)."""
import numpy as np
import pytest
import torch


@pytest.fixture(scope="module")
def cpu_model(stif, sd):
    m = stif.LunaTokis(64, 6, 8, 5, 40, device="cpu")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return m


def test_parameters_are_the_reference_state_dict(cpu_model, sd):
    """442 keys in the reference's registration order, 11,312,698 parameters,
    values as loaded; packed kernel copies are non-persistent (not in state_dict)."""
    msd = cpu_model.state_dict()
    assert list(msd.keys()) == list(sd.keys())
    assert sum(p.numel() for p in cpu_model.parameters()) == 11312698
    for k in ("conv_first.weight", "pcd_align.L1_dcnpack_2.conv_offset_mask.bias", "encode_imnet.net.4.weight"):
        assert np.array_equal(msd[k].numpy(), sd[k])
    assert all(not p.requires_grad for p in cpu_model.parameters())
    assert len(list(cpu_model.buffers())) > 300          # packed layers ride along with .to()/replicate


def test_load_state_dict_contract(stif, sd):
    m = stif.LunaTokis(64, 6, 8, 5, 40, device="cpu")
    m.load_state_dict({"module." + k: torch.from_numpy(v) for k, v in sd.items()})   # base_model.py:93-98
    bad = dict(sd)
    del bad["fusion.bias"]
    with pytest.raises(RuntimeError, match="Missing key"):
        m.load_state_dict(bad)
    bad = dict(sd)
    bad["fusion.bias"] = np.zeros(3, np.float32)
    with pytest.raises(RuntimeError, match="size mismatch"):
        m.load_state_dict(bad)
    r = m.load_state_dict({"fusion.bias": sd["fusion.bias"]}, strict=False)
    assert len(r.missing_keys) == 441


def test_module_behaviour(stif, cpu_model):
    assert cpu_model.eval() is cpu_model and not cpu_model.training
    with pytest.raises(NotImplementedError):
        cpu_model.train()
    with pytest.raises(NotImplementedError):
        cpu_model.to(torch.float16)
    with pytest.raises(NotImplementedError):
        cpu_model.half()
    dp = torch.nn.DataParallel(cpu_model)             # VideoSR_base_model.py:31-32 (no GPU: plain call)
    assert dp.module is cpu_model
    with pytest.raises(stif._lib.StifError, match="GPU only"):
        cpu_model(torch.zeros(1, 2, 3, 8, 8), [0.5])


def test_f16x3_weight_range_fallback_at_pack(stif):
    L, ops = stif._lib, stif.ops
    rng = np.random.default_rng(0)
    w = rng.standard_normal((64, 64, 3, 3)).astype(np.float32) * 0.05
    b = np.zeros(64, np.float32)
    assert ops.pack_conv(w, b, L.PACK_WINO | L.PACK_F16X3, "cpu").mode == L.PACK_WINO | L.PACK_F16X3
    big = w.copy()
    big[3, 5, 0, 0] = 70.0                            # U[0][0] = g[0][0] >= 64: not representable split
    assert ops.pack_conv(big, b, L.PACK_WINO | L.PACK_F16X3, "cpu").mode == L.PACK_WINO
    with pytest.raises(L.StifError, match="f16x3 range") as e:
        ops.pack_conv(big, b, L.PACK_WINO | L.PACK_F16X3, "cpu", range_fallback=False)
    assert e.value.code == L.E_RANGE
    assert ops.pack_conv(big, b, L.PACK_PLAIN | L.PACK_F16X3, "cpu").mode == L.PACK_PLAIN   # DCN core


def test_model_packs_out_of_range_layers_in_fp32(stif, sd):
    L = stif._lib
    sd2 = dict(sd)
    sd2["recon_trunk.7.conv2.weight"] = sd["recon_trunk.7.conv2.weight"] * 3000.0
    # x 30 / (2 pi) (the f16x3 packing's sine scale, in revolutions): > 64
    sd2["encode_imnet.net.3.linear.weight"] = sd["encode_imnet.net.3.linear.weight"] * 10000.0
    m = stif.LunaTokis(64, 6, 8, 5, 40, device="cpu")
    m.load_state_dict(sd2)
    lay = m._build_layers(m._pk, m._meta)
    assert lay["recon_trunk.7.conv2"].mode == L.PACK_WINO
    assert lay["recon_trunk.7.conv1"].mode == L.PACK_WINO | L.PACK_F16X3
    assert m._dec_flags == 0 and m._meta["dec.mlp"][1] == 0


def _pk_bufs(pk):
    return [pk._buffers[f"b{i}"] for i in range(len(pk._buffers))]


def _same_packing(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def test_repack_after_out_of_range_checkpoint(stif, sd):
    """A good checkpoint loaded after one that forced the decoder MLP to fp32 packs exactly as into a
    fresh module: the operand flag is derived from ``mfma`` at every packing, not from the last one."""
    L = stif._lib
    sd2 = dict(sd)
    sd2["encode_imnet.net.3.linear.weight"] = sd["encode_imnet.net.3.linear.weight"] * 10000.0
    m = stif.LunaTokis(64, 6, 8, 5, 40, device="cpu")
    m.load_state_dict(sd2)
    assert m._dec_flags == 0 and m._meta["dec.mlp"][1] == 0
    m.load_state_dict(sd)
    assert m._dec_flags == L.CONV_F16X3 and m._meta["dec.mlp"][1] == L.CONV_F16X3
    fresh = stif.LunaTokis(64, 6, 8, 5, 40, device="cpu")
    fresh.load_state_dict(sd)
    assert m._meta == fresh._meta
    assert _same_packing(_pk_bufs(m._pk), _pk_bufs(fresh._pk))


def test_fp32_repack_leaves_the_module_alone(stif, sd):
    """_layers_fp32 (the range fallback's layers) packs into _pk32 / _meta32 only: the module's own packing,
    its operand settings, the constant maps and the decoder tables stay; the copy is kept until the next
    checkpoint."""
    L = stif._lib
    m = stif.LunaTokis(64, 6, 8, 5, 40, device="cpu")
    m.load_state_dict(sd)
    const = m._const(("k", 1), (2, 8, 8), lambda: torch.ones(1))
    m._tables["probe"] = table = object()
    before = (m.mfma, m._dec_flags, dict(m._meta), m._pk, _pk_bufs(m._pk), [b.data_ptr() for b in _pk_bufs(m._pk)])
    lay32 = m._layers_fp32()
    assert (m.mfma, m._dec_flags, m._meta) == before[:3] and m._dec_flags == L.CONV_F16X3
    assert m._pk is before[3] and all(a is b for a, b in zip(_pk_bufs(m._pk), before[4]))
    assert [b.data_ptr() for b in _pk_bufs(m._pk)] == before[5]
    assert m._consts[("cpu", 2, 8, 8)][("k", 1)] is const and m._tables["probe"] is table
    assert not any(v.mode & L.PACK_F16X3 for k, v in lay32.items() if k != "dec.mlp")
    m32 = stif.LunaTokis(64, 6, 8, 5, 40, device="cpu", mfma="f32")
    m32.load_state_dict(sd)
    ref = m32._build_layers(m32._pk, m32._meta)
    assert m._meta32 == m32._meta and list(lay32) == list(ref)
    for k, v in ref.items():
        if k == "dec.mlp":
            assert torch.equal(lay32[k], v)
        else:
            assert (lay32[k].cout, lay32[k].cin, lay32[k].ks, lay32[k].mode) == (v.cout, v.cin, v.ks, v.mode), k
            assert torch.equal(lay32[k].w, v.w) and torch.equal(lay32[k].b, v.b), k
    ptrs32 = [b.data_ptr() for b in _pk_bufs(m._pk32)]
    m._layers_fp32()                                          # kept: nothing is packed again
    assert [b.data_ptr() for b in _pk_bufs(m._pk32)] == ptrs32
    old32 = _pk_bufs(m._pk32)
    m.load_state_dict(sd)                                     # a new checkpoint: the next call repacks
    m._layers_fp32()
    assert all(a is not b for a, b in zip(_pk_bufs(m._pk32), old32))
    assert m._pk32.b2.data_ptr() != ptrs32[2]                 # a packed conv weight: new storage (old32 is alive)
    assert _same_packing(_pk_bufs(m._pk32), old32)


def test_pack_model_is_pure(stif, sd):
    """packing.pack_model is a function of its arguments: the same call twice gives equal results, and
    an fp32 packing in between does not change the next f16x3 one."""
    kw = dict(winograd=True, fused_dcn=True, front_RBs=5, back_RBs=40)
    pack = stif.packing.pack_model
    b1, m1 = pack(sd, "cpu", mfma="f16x3", **kw)
    b2, m2 = pack(sd, "cpu", mfma="f16x3", **kw)
    b32, m32 = pack(sd, "cpu", mfma="f32", **kw)
    b3, m3 = pack(sd, "cpu", mfma="f16x3", **kw)
    assert m1 == m2 == m3 and _same_packing(b1, b2) and _same_packing(b1, b3)
    assert m1["dec.mlp"][1] == stif._lib.CONV_F16X3 and m32["dec.mlp"][1] == 0 and m32 != m1


def test_lane_range_split(stif):
    """The contiguous ranges lanes are made of (the cases test_lanes_are_bit_identical runs)."""
    split = stif.model._split
    assert split(5, 4) == [(0, 2), (2, 4), (4, 5)]
    assert split(15, 2) == [(0, 8), (8, 15)]
    assert split(15, 3) == [(0, 5), (5, 10), (10, 15)]
    assert split(3, 1) == [(0, 3)] and split(2, 5) == [(0, 1), (1, 2)]


def test_const_cache_is_device_scoped_and_bounded(stif, cpu_model):
    """_const (the weight-only constant maps): entries are grouped by (device, shape), at most
    const_shapes groups per device are kept (least recently used evicted), a replica sharing the dict
    on another device never receives this device's tensors, and .to() drops the groups of the device
    the module left (advisor r5)."""
    import copy
    m = cpu_model
    m._consts.clear()
    calls = []

    def mk(tag):
        calls.append(tag)
        return torch.full((1,), float(len(calls)))

    a = m._const(("k", 1), (2, 8, 8), lambda: mk("a"))
    assert m._const(("k", 1), (2, 8, 8), lambda: mk("x")) is a and calls == ["a"]
    m._const(("k", 1), (2, 16, 16), lambda: mk("b"))
    m._const(("k", 1), (2, 8, 8), lambda: mk("y"))          # hit: (2, 8, 8) becomes most recent
    m._const(("k", 1), (2, 32, 32), lambda: mk("c"))        # third shape: evicts (2, 16, 16)
    assert calls == ["a", "b", "c"] and list(m._consts) == [("cpu", 2, 8, 8), ("cpu", 2, 32, 32)]
    assert m._zeros(2, 8, 8, 64).shape == (2, 8, 8, 64) and ("zeros", 2, 8, 8, 64) in m._consts[("cpu", 2, 8, 8)]
    # a replica whose device differs (DataParallel shares __dict__ entries shallowly): its own group
    class OnMeta(type(m)):
        device = property(lambda self: torch.device("meta"))

    rep = copy.copy(m)
    rep.__class__ = OnMeta
    assert rep._consts is m._consts
    r = rep._const(("k", 1), (2, 8, 8), lambda: mk("rep"))
    assert r is not a and calls[-1] == "rep" and ("meta", 2, 8, 8) in m._consts
    m.to("cpu")                                                # leaving "meta"-device entries behind
    assert all(g[0] == "cpu" for g in m._consts)
    with pytest.raises(ValueError):
        stif.LunaTokis(64, 6, 8, 5, 40, device="cpu", const_shapes=0)
