"""Which gradients a conv node of stif_amd.train produces: one that is not asked for is not produced, and asking for
fewer never changes the bits of the others.  The nodes share their ``needs`` tails and their data-gradient helper, so
the contract is pinned for all of them at once: Conv3x3, ResidualBlock_noBN, ConvDown, ConvFirst, Conv3x3Cat,
Conv1x1Cat and ConvLSTMCell, in both ``mfma`` modes where the module has the choice.  (DCN_sep's fused backward takes
the need tuple into the kernel and is covered by tests/test_gpu_dcn_bwd.py.)

The comparison is of the code against itself on purpose: it checks independence, not values -- the values are held
to float64 torch by the modules' own tests.  Inputs [2, 64, 5, 7] ([2, 3, 5, 7] frames for ConvFirst): the smallest
shape of the conv-backward tests, odd sizes (the stride-2 output is 3 x 4), partial tiles and every padding tap.
Procedure: one run with every input and parameter requiring grad; then, for each input and each parameter in turn,
that one alone frozen, from the same seed and grad_out: its ``.grad`` is None, every other gradient is torch.equal to
the full run's, and ``range_status()`` is 0."""
import pytest
import torch

pytestmark = pytest.mark.gpu

N, H, W = 2, 5, 7
# name -> (constructor taking the train module and mfma, the shapes of its inputs, whether it has the mfma choice)
CASES = {
    "Conv3x3": (lambda T, m: T.Conv3x3(64, "lrelu", m), [(N, 64, H, W)], True),
    "ResidualBlock_noBN": (lambda T, m: T.ResidualBlock_noBN(64, m), [(N, 64, H, W)], True),
    "ConvDown": (lambda T, m: T.ConvDown(64, "lrelu"), [(N, 64, H, W)], False),
    "ConvFirst": (lambda T, m: T.ConvFirst(), [(N, 3, H, W)], False),
    "Conv3x3Cat": (lambda T, m: T.Conv3x3Cat("lrelu", m), [(N, 64, H, W)] * 2, True),
    "Conv1x1Cat": (lambda T, m: T.Conv1x1Cat(m), [(N, 64, H, W)] * 2, True),
    "ConvLSTMCell": (lambda T, m: T.ConvLSTMCell(m), [(N, 64, H, W)] * 3, True),
}
PARAMS = [(name, mfma) for name, case in CASES.items() for mfma in (("f32", "f16x3") if case[2] else ("f32",))]


def run(T, name, mfma, frozen):
    """One forward and backward of a freshly seeded module; ``frozen``: ("input", i), ("param", key) or None.
    Returns ({"input i" / parameter name: its .grad or None}, range_status)."""
    make, shapes, _ = CASES[name]
    torch.manual_seed(1234)
    mod = make(T, mfma).cuda()
    if name == "ResidualBlock_noBN":     # its biases start at zero: give them values, from the same seed
        with torch.no_grad():
            for p in mod.parameters():
                p.add_(0.05 * torch.randn_like(p))
    gen = torch.Generator().manual_seed(99)
    inputs = [torch.randn(s, generator=gen).cuda() for s in shapes]
    wants_grad = name != "ConvFirst"     # the gradient with respect to the frames is not built
    for i, t in enumerate(inputs):
        if wants_grad and frozen != ("input", i):
            t.requires_grad_(True)
    for key, p in mod.named_parameters():
        if frozen == ("param", key):
            p.requires_grad_(False)
    if name == "ConvLSTMCell":
        outs = mod(inputs[0], (inputs[1], inputs[2]))
    else:
        outs = (mod(*inputs),)
    gouts = [torch.randn(o.shape, generator=gen).cuda() for o in outs]
    torch.autograd.backward(outs, gouts)
    grads = {f"input {i}": t.grad for i, t in enumerate(inputs) if wants_grad}
    grads.update({key: p.grad for key, p in mod.named_parameters()})
    status = mod.range_status() if hasattr(mod, "range_status") else T.range_status()
    return grads, status


@pytest.mark.parametrize("name,mfma", PARAMS, ids=[f"{n}-{m}" for n, m in PARAMS])
def test_unasked_gradients_are_not_produced_and_the_others_keep_their_bits(stif, name, mfma):
    T = stif.train
    full, status = run(T, name, mfma, None)
    assert status == 0
    assert all(g is not None for g in full.values()), [k for k, g in full.items() if g is None]
    for key in full:
        frozen = ("input", int(key.split()[1])) if key.startswith("input ") else ("param", key)
        got, status = run(T, name, mfma, frozen)
        assert status == 0, key
        assert got[key] is None, f"{key} was frozen and still received a gradient"
        for other, g in full.items():
            if other != key:
                assert got[other] is not None and torch.equal(got[other], g), (key, other)
