"""Weight packing: the reference's state dict -> the buffers the gfx950 kernels read.

``pack_model`` is a function of the host weights and the packing settings alone: it reads and writes no
module (LunaTokis installs its result as non-persistent buffers, model.py).
"""
import numpy as np
import torch

from . import _lib as L
from . import ops
from . import weights as W


def pack_model(host, device, *, mfma, winograd, fused_dcn, front_RBs, back_RBs):
    """Pack every layer of the state dict ``host`` (key -> fp32 ndarray) for the kernels, on ``device``.
    Returns (bufs, meta): ``bufs`` the flat list of packed tensors (weight, bias per layer) and ``meta`` the
    layer name -> (index into bufs, cout, cin, ks, mode); ``meta["dec.mlp"] = (index, decoder operand flags)``.
    f16x3 packings whose weights leave the split range fall back to fp32 per layer."""
    h, dev = host, device
    meta = {}
    bufs = []

    def put(name, pc):
        meta[name] = (len(bufs), pc.cout, pc.cin, pc.ks, pc.mode)
        bufs.append(pc.w)
        bufs.append(pc.b if pc.b is not None else torch.zeros(1, device=dev))

    def conv(name, mode=L.PACK_PLAIN):
        put(name, ops.pack_conv(h[name + ".weight"], h[name + ".bias"], mode, dev))

    # 3x3 / stride-1 / 64-cout convs run by Winograd F(2x2,3x3) (stif_conv3x3_wino; the
    # cat(., up(.)) ones on a materialised x2-upsampled second input), as do the offset/mask
    # (64 -> 216) and ConvLSTMCell (128 -> 256, gate epilogue) convs; the strided convs keep the
    # direct kernel, the 1x1 cat convs (fusion, conv_1x1) run k_conv1x1 (f16x3) or the direct
    # kernel (f32).
    f16 = L.PACK_F16X3 if mfma == "f16x3" else 0
    wino = (L.PACK_WINO | f16) if winograd else L.PACK_PLAIN

    put("conv_first", ops.PackedConv(torch.from_numpy(h["conv_first.weight"]).to(dev),
                                     torch.from_numpy(h["conv_first.bias"]).to(dev), 64, 3, 3, L.PACK_PLAIN))
    for i in range(front_RBs):
        conv(f"feature_extraction.{i}.conv1", wino)
        conv(f"feature_extraction.{i}.conv2", wino)
    for n in ("fea_L2_conv1", "fea_L3_conv1"):      # 3x3 stride-2 64 -> 64
        conv(n, L.PACK_PLAIN | f16)
    for n in ("fea_L2_conv2", "fea_L3_conv2"):
        conv(n, wino)

    def pcd(prefix):
        for d in (1, 2):
            for ln, cin, _ in W._PCD_LAYERS:
                n = f"{prefix}{ln}_{d}"
                if cin is None:
                    om = n + ".conv_offset_mask"
                    if f16 and fused_dcn:
                        # the fused DCN_sep kernel (k_dcn_sep); out of the split range -> the two-kernel path
                        try:
                            pom = ops.pack_conv(h[om + ".weight"], h[om + ".bias"], L.PACK_DCNSEP | L.PACK_F16X3,
                                                dev, range_fallback=False)
                            pcore = ops.pack_conv(h[n + ".weight"], h[n + ".bias"], L.PACK_DCNPAIR | L.PACK_F16X3,
                                                  dev, range_fallback=False)
                            put(n, pcore)
                            put(om, pom)
                            continue
                        except L.StifError as e:
                            if e.code != L.E_RANGE:
                                raise
                    conv(n, L.PACK_PLAIN | f16)     # the DCN core (k_dcn)
                    conv(om, (L.PACK_WINO_OFFMASK | f16) if winograd else L.PACK_OFFMASK)
                else:
                    conv(n, wino)

    pcd("pcd_align.")
    conv("fusion", L.PACK_PLAIN | f16)
    conv("ConvBLSTM.forward_net.cell_list.0.conv", (L.PACK_WINO_LSTM | f16) if winograd else L.PACK_LSTM)
    for p in ("ConvBLSTM.forward_net.pcd_h.", "ConvBLSTM.forward_net.pcd_c."):
        for n in ("fea_L2_conv1", "fea_L3_conv1"):
            conv(p + n, L.PACK_PLAIN | f16)
        conv(p + "fusion", L.PACK_PLAIN | f16)
        for n in ("fea_L2_conv2", "fea_L3_conv2"):
            conv(p + n, wino)
        pcd(p + "pcd_align.")
    conv("ConvBLSTM.conv_1x1", L.PACK_PLAIN | f16)
    for i in range(back_RBs):
        conv(f"recon_trunk.{i}.conv1", wino)
        conv(f"recon_trunk.{i}.conv2", wino)
    # decoder: the SIREN MLPs, then the LR projections (their sine-layer scale follows the MLP's
    # operand mode: omega_0 / (2 pi) -- revolutions -- with f16x3, stif.h STIF_DEC_REVOLUTIONS)
    mlp, flags = _pack_mlp(h, L.CONV_F16X3 if f16 else 0)
    for lr_image in (True, False):
        put("dec.proj" if lr_image else "dec.proj_hrimg",
            _pack_proj(h, dev, bool(f16), lr_image, bool(flags & L.CONV_F16X3)))
    meta["dec.mlp"] = (len(bufs), flags)
    bufs.append(mlp.to(dev))
    bufs.append(torch.zeros(1, device=dev))
    return bufs, meta


def _pack_mlp(h, flags):
    """All SIREN layers (stif_pack_dec_mlp_ex) as a host tensor, and the operand flags they were packed
    with: an out-of-range weight for f16x3 -> fp32 packing (flags 0)."""
    lib = L.lib()

    def siren_ptrs(prefix, n_sine):
        """pointers to (weight, bias) of the n_sine sine layers and the last linear layer (the arrays live in h)"""
        layers = [f"{prefix}net.{i}.linear" for i in range(n_sine)] + [f"{prefix}net.{n_sine}"]
        return (L._P * (2 * len(layers)))(*[h[f"{n}.{p}"].ctypes.data for n in layers for p in ("weight", "bias")])

    fp, lp, ep = siren_ptrs("feat_imnet.", 3), siren_ptrs("flow_imnet.", 3), siren_ptrs("encode_imnet.", 4)
    mlp = np.empty(lib.stif_dec_mlp_floats(), np.float32)
    try:
        L.check(lib.stif_pack_dec_mlp_ex(fp, lp, ep, mlp.ctypes.data, flags), "stif_pack_dec_mlp_ex")
    except L.StifError as e:
        if e.code != L.E_RANGE or not flags:
            raise
        flags = 0
        L.check(lib.stif_pack_dec_mlp_ex(fp, lp, ep, mlp.ctypes.data, 0), "stif_pack_dec_mlp_ex")
    return torch.from_numpy(mlp), flags


def _pack_proj(h, dev, f16x3, lr_image, revolutions):
    """LR projection of the decoder's first layers (stif_pack_dec_proj_ex); lr_image=False leaves
    the LR frames out of P2..P4 for decoding_test, which samples the x4-upsampled frames;
    revolutions: sine-layer scale omega_0 / (2 pi), matching an f16x3-packed MLP."""
    lib = L.lib()

    def pack(mode):
        wd = np.empty(lib.stif_conv_weight_floats(256, 200, 1, mode), np.float32)
        bd = np.empty(lib.stif_conv_bias_floats(256, L.PACK_PLAIN), np.float32)
        L.check(lib.stif_pack_dec_proj_ex(h["feat_imnet.net.0.linear.weight"].ctypes.data,
                                          h["feat_imnet.net.0.linear.bias"].ctypes.data,
                                          h["flow_imnet.net.0.linear.weight"].ctypes.data,
                                          h["encode_imnet.net.0.linear.weight"].ctypes.data,
                                          int(lr_image) | (mode & L.PACK_F16X3) | (L.DEC_REVOLUTIONS if revolutions else 0),
                                          wd.ctypes.data, bd.ctypes.data),
                "stif_pack_dec_proj_ex")
        return ops.PackedConv(torch.from_numpy(wd).to(dev), torch.from_numpy(bd).to(dev), 256, 200, 1, mode)

    if f16x3:   # k_conv1x1; a weight outside the split range -> fp32 packing
        try:
            return pack(L.PACK_PLAIN | L.PACK_F16X3)
        except L.StifError as e:
            if e.code != L.E_RANGE:
                raise
    return pack(L.PACK_PLAIN)
