"""A pure-torch, differentiable reference of DCN_sep and PCD_Align (not a test): F.conv2d / F.interpolate and a
modulated deformable convolution written with gathers, in whatever dtype its inputs have (float64 for the reference,
float32 for the reference's own rounding floor).  tests/test_pcd_train_host.py pins it to the numpy oracle
(oracle.dcn_v2_forward / dcn_v2_backward / pcd_align); the GPU tests compare the HIP modules with it.

Sampling coordinates are rounded to float32 as the reference's CUDA kernels, the oracle and the HIP kernels compute them
(integer grid position + offset in float32); the rounding is a straight-through step, so autograd differentiates the
bilinear weights as dcn_v2_backward does.

Input recipe (``tame_offsets``): bilinear sampling has a discontinuous offset gradient at integer coordinates, so the
tests keep every sample away from them by construction -- the offset biases of every conv_offset_mask are 0.5 and its
offset rows are rescaled so that |offset - 0.5| <= 0.3 everywhere in the float64 reference; the mask rows stay random.
``assert_offsets_tame`` is the check every DCN test makes on the float64 reference before it compares anything."""
import torch
import torch.nn.functional as F

DG, K = 8, 9


def lrelu(x):
    return F.leaky_relu(x, 0.1)


def up2(x):
    return F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False)


def dcn(inp, offset, mask, weight, bias):
    """Modulated deformable conv, 3x3 / stride 1 / pad 1 / dilation 1, DG groups (dcn_v2_im2col_cuda.cu:125-195):
    offset [B, 2 DG K, H, W] with (group g, tap k) at g 2K + 2k (+1 for w), mask [B, DG K, H, W] after the sigmoid."""
    B, C, H, W = inp.shape
    cpg, P, dt = C // DG, H * W, inp.dtype
    off = offset.reshape(B, DG, K, 2, H, W)
    msk = mask.reshape(B, DG, K, P)
    img = inp.reshape(B, DG, cpg, P)
    ys = torch.arange(H, dtype=dt).view(1, 1, H, 1)
    xs = torch.arange(W, dtype=dt).view(1, 1, 1, W)

    def f32_coord(base, o):
        c = base + o
        c32 = (base.float() + o.detach().float()).to(dt)      # the float32 sum the kernels compute
        return c + (c32 - c).detach()

    cols = []
    for k in range(K):
        i, j = divmod(k, 3)
        h = f32_coord(ys - 1 + i, off[:, :, k, 0]).reshape(B, DG, P)
        w = f32_coord(xs - 1 + j, off[:, :, k, 1]).reshape(B, DG, P)
        inside = ((h > -1) & (w > -1) & (h < H) & (w < W)).to(dt)
        h0, w0 = torch.floor(h).detach(), torch.floor(w).detach()
        lh, lw = h - h0, w - w0
        val = 0
        for hc, wc, wt in ((h0, w0, (1 - lh) * (1 - lw)), (h0, w0 + 1, (1 - lh) * lw),
                           (h0 + 1, w0, lh * (1 - lw)), (h0 + 1, w0 + 1, lh * lw)):
            ok = ((hc >= 0) & (hc <= H - 1) & (wc >= 0) & (wc <= W - 1)).to(dt)
            idx = (hc.clamp(0, H - 1) * W + wc.clamp(0, W - 1)).long()
            v = torch.gather(img, 3, idx.view(B, DG, 1, P).expand(B, DG, cpg, P))
            val = val + v * (wt * ok).view(B, DG, 1, P)
        cols.append(val * (msk[:, :, k] * inside).view(B, DG, 1, P))
    cols = torch.stack(cols, 3).reshape(B, C, K, P)
    out = torch.einsum("ock,bckp->bop", weight.reshape(weight.shape[0], C, K), cols) + bias.view(1, -1, 1)
    return out.reshape(B, -1, H, W)


def offset_mask(fea, w_om, b_om):
    """(offset, mask) of DCN_sep.forward (dcn_v2.py:130-138): cat(o1, o2) is the first two thirds of the channels."""
    om = F.conv2d(fea, w_om, b_om, padding=1)
    return om[:, :2 * DG * K], torch.sigmoid(om[:, 2 * DG * K:])


def dcn_sep(inp, fea, P, name):
    offset, mask = offset_mask(fea, P[name + ".conv_offset_mask.weight"], P[name + ".conv_offset_mask.bias"])
    return dcn(inp, offset, mask, P[name + ".weight"], P[name + ".bias"])


def pcd_align(P, fea1, fea2, feas=None):
    """PCD_Align.forward (Sakuya_arch_test.py:71-130) on the parameter dict ``P`` (the module's state-dict keys).
    ``feas``: a dict that receives the ``fea`` input of every DCN_sep, by its name."""
    c = lambda n, *t: F.conv2d(torch.cat(t, 1), P[n + ".weight"], P[n + ".bias"], padding=1)
    y = []
    for s, fa, fb in (("_1", fea1, fea2), ("_2", fea2, fea1)):
        L3_off = lrelu(c("L3_offset_conv2" + s, lrelu(c("L3_offset_conv1" + s, fa[2], fb[2]))))
        L2_off = lrelu(c("L2_offset_conv1" + s, fa[1], fb[1]))
        L2_off = lrelu(c("L2_offset_conv3" + s, lrelu(c("L2_offset_conv2" + s, L2_off, up2(L3_off) * 2))))
        L1_off = lrelu(c("L1_offset_conv1" + s, fa[0], fb[0]))
        L1_off = lrelu(c("L1_offset_conv3" + s, lrelu(c("L1_offset_conv2" + s, L1_off, up2(L2_off) * 2))))
        if feas is not None:
            feas.update({"L3_dcnpack" + s: L3_off, "L2_dcnpack" + s: L2_off, "L1_dcnpack" + s: L1_off})
        L3_fea = lrelu(dcn_sep(fa[2], L3_off, P, "L3_dcnpack" + s))
        L2_fea = lrelu(c("L2_fea_conv" + s, dcn_sep(fa[1], L2_off, P, "L2_dcnpack" + s), up2(L3_fea)))
        y.append(c("L1_fea_conv" + s, dcn_sep(fa[0], L1_off, P, "L1_dcnpack" + s), up2(L2_fea)))
    return torch.cat(y, 1)


def pcd_param_shapes():
    """{state-dict key: shape} of PCD_Align in the reference's registration order."""
    conv = lambda name, cin: {name + ".weight": (64, cin, 3, 3), name + ".bias": (64,)}
    shapes = {}
    for s in ("_1", "_2"):
        for lv in ("L3", "L2", "L1"):
            shapes.update(conv(f"{lv}_offset_conv1{s}", 128))
            shapes.update(conv(f"{lv}_offset_conv2{s}", 64 if lv == "L3" else 128))
            if lv != "L3":
                shapes.update(conv(f"{lv}_offset_conv3{s}", 64))
            shapes.update(conv(f"{lv}_dcnpack{s}", 64))
            shapes.update({f"{lv}_dcnpack{s}.conv_offset_mask.weight": (216, 64, 3, 3),
                           f"{lv}_dcnpack{s}.conv_offset_mask.bias": (216,)})
            if lv != "L3":
                shapes.update(conv(f"{lv}_fea_conv{s}", 128))
    return shapes


def random_pcd_params(seed, scale=1.0):
    """Float64 parameters, mask rows included: uniform weights of variance 1 / fan_in (every layer keeps the size of
    its input, so the features, masks and gradients of the deepest level are as large as the first's) and biases in
    +-0.1."""
    g = torch.Generator().manual_seed(seed)
    P = {}
    for k, shp in pcd_param_shapes().items():
        bound = 0.1 if len(shp) == 1 else (3.0 / (shp[1] * 9)) ** 0.5
        P[k] = (torch.rand(shp, generator=g, dtype=torch.float64) * 2 - 1) * scale * bound
    return P


def tame_dcn(w_om, b_om, fea, margin=0.3):
    """The recipe for one conv_offset_mask, in place: offset biases 0.5, offset rows scaled to |offset - 0.5| <= margin
    on ``fea`` (float64)."""
    n_off = 2 * DG * K
    with torch.no_grad():
        raw = F.conv2d(fea.double(), w_om[:n_off].double(), None, padding=1)
        w_om[:n_off] *= 0.999 * margin / float(raw.abs().max())
        b_om[:n_off] = 0.5


def tame_offsets(P, fea1, fea2):
    """The recipe for every DCN_sep of PCD_Align, in place on the float64 parameter dict ``P``.  The ``fea`` input of a
    DCN_sep depends on no conv_offset_mask (offsets feed only the deformable convs), so one pass gives them all."""
    feas = {}
    with torch.no_grad():
        pcd_align(P, fea1, fea2, feas)
    for name, fea in feas.items():
        tame_dcn(P[name + ".conv_offset_mask.weight"], P[name + ".conv_offset_mask.bias"], fea)
    return feas


def assert_offsets_tame(offset):
    """Every sampling coordinate of the float64 reference is at least 0.1 from an integer: a failure is a test-input
    bug, not a tolerance case."""
    frac = offset.detach().double() - torch.floor(offset.detach().double())
    assert float(frac.min()) >= 0.1 and float(frac.max()) <= 0.9, (float(frac.min()), float(frac.max()))


def assert_pcd_offsets_tame(P, fea1, fea2):
    feas = {}
    with torch.no_grad():
        pcd_align(P, fea1, fea2, feas)
        for name, fea in feas.items():
            offset, _ = offset_mask(fea, P[name + ".conv_offset_mask.weight"], P[name + ".conv_offset_mask.bias"])
            assert_offsets_tame(offset)


def pyramid_inputs(seed, B, H, W, dtype=torch.float64):
    """Two random lists [L1, L2, L3] of [B, 64, H >> l, W >> l] maps."""
    g = torch.Generator().manual_seed(seed)
    mk = lambda: [torch.randn(B, 64, H >> l, W >> l, generator=g, dtype=torch.float64).to(dtype) for l in range(3)]
    return mk(), mk()
