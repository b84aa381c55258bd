"""Thin torch-facing wrappers over the C ABI.

Torch tensors are only device buffers here: every op passes ``data_ptr()``s,
sizes and the current HIP stream to libstif_hip.so.  Feature maps are NHWC
``[items, H, W, C]`` fp32 tensors (any item stride; rows/pixels contiguous).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib as L
from .coords import TABLE_ORDER, check_window, dec_tables, dec_train_tables

# Optional launch tracer (bench.py sets it to time the dominant kernel with HIP events on
# the launch stream): an object with begin(kind: tuple, flops: float) and end().
TRACE = None

# Dynamic tile scheduling of the persistent Winograd conv (stif_conv_args.sched): one block of counters
# per (device, stream), zeroed once and kept for the process (the library tracks each block's running
# totals) -- launches on one stream run in issue order, launches on different streams never share one.
# Default off: at C0 the dynamic schedule measured 0.1-0.3 ms per step slower than the static one alone,
# and equal to it with the PCD DCN branch on a second stream (profiles/r05_dynamic_tiles_ab.log).
DYNAMIC_TILES = False
_SCHED = {}


def _sched_buf():
    if not DYNAMIC_TILES or torch.cuda.is_current_stream_capturing():
        return None
    s = torch.cuda.current_stream()
    key = (s.device.index, s.cuda_stream)
    b = _SCHED.get(key)
    if b is None:
        b = _SCHED[key] = torch.zeros(16, dtype=torch.int32, device=s.device)   # stream-ordered before use
    return b


def _vp(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _launch(what: str, trace, fn, *args):
    """Call the library entry ``fn`` and check its status (errors name ``what``).  ``trace``: None, or the
    arguments of TRACE.begin -- (kind, flops[, nbytes]) -- which callers compute only when TRACE is set."""
    tr = TRACE if trace is not None else None
    if tr is not None:
        tr.begin(*trace)
    L.check(fn(*args), what)
    if tr is not None:
        tr.end()


def _pixels_contiguous(t: torch.Tensor) -> bool:
    """The pixels of each item of NHWC ``t`` are contiguous (strides of size-1 dims never address anything)."""
    _, h, w, c = t.shape
    return (c <= 1 or t.stride(3) == 1) and (w <= 1 or t.stride(2) == c) and (h <= 1 or t.stride(1) == w * c)


def _item_stride(ts: Sequence[Optional[torch.Tensor]], what: str) -> int:
    strides = {t.stride(0) for t in ts if t is not None}
    if len(strides) > 1:
        raise ValueError(f"{what}: groups must share the item stride, got {strides}")
    for t in ts:
        if t is None:
            continue
        if t.dtype != torch.float32 or not t.is_cuda:
            raise ValueError(f"{what}: expected float32 CUDA tensors")
        if not _pixels_contiguous(t):
            raise ValueError(f"{what}: pixels of an item must be contiguous NHWC")
    return strides.pop() if strides else 0


@dataclass
class PackedConv:
    """A conv layer repacked for stif_conv2d_nhwc (see stif_pack_conv_weight)."""
    w: torch.Tensor
    b: torch.Tensor
    cout: int
    cin: int
    ks: int
    mode: int


def pack_conv(weight: np.ndarray, bias: np.ndarray, mode: int = L.PACK_PLAIN, device="cuda",
              range_fallback: bool = True) -> PackedConv:
    """Pack one conv layer.  A STIF_PACK_F16X3 packing whose weights leave the split-fp16 range
    (stif_pack_conv_weight -> STIF_E_RANGE) is re-packed in fp32 (same kernel family, fp32 MFMA)
    when ``range_fallback``; otherwise the StifError propagates."""
    weight = np.ascontiguousarray(weight, np.float32)
    bias = np.ascontiguousarray(bias, np.float32)
    cout, cin, ks, _ = weight.shape
    lib = L.lib()
    wd = np.empty(lib.stif_conv_weight_floats(cout, cin, ks, mode), np.float32)
    bd = np.empty(lib.stif_conv_bias_floats(cout, mode), np.float32)
    try:
        L.check(lib.stif_pack_conv_weight(weight.ctypes.data, bias.ctypes.data, cout, cin, ks, mode,
                                          wd.ctypes.data, bd.ctypes.data), "stif_pack_conv_weight")
    except L.StifError as e:
        if e.code != L.E_RANGE or not range_fallback or not mode & L.PACK_F16X3:
            raise
        return pack_conv(weight, bias, mode & ~L.PACK_F16X3, device, False)
    return PackedConv(torch.from_numpy(wd).to(device), torch.from_numpy(bd).to(device), cout, cin, ks, mode)


def _split_by_mode(groups, key):
    """Launch groups by operand mode: layers that fell back to fp32 packing run in their own launch."""
    f16 = [g for g in groups if g[key].mode & L.PACK_F16X3]
    return [f16, [g for g in groups if not g[key].mode & L.PACK_F16X3]] if 0 < len(f16) < len(groups) else None


def _set_items(a, counts) -> int:
    """Fill the launch's item counts from the groups' own (stif.h item_base): the uniform form (nitems, an all-zero
    table) when they agree, else the prefix table.  Returns the launch's total items."""
    a.ngroups = len(counts)
    if len(set(counts)) == 1:
        a.nitems = counts[0]
    else:
        a.nitems = 0
        for i, c in enumerate(counts):
            a.item_base[i + 1] = a.item_base[i] + c
    return sum(counts)


def conv2d(groups, *, epi=L.EPI_NONE, in1_mode=0, in1_scale=1.0, stride=None, status=None):
    """groups: list of dicts {layer: PackedConv, in0, [in1], out, [res], [out2]} with tensors
    [nitems, H, W, C].  All groups share map shapes and item strides; each may carry its own number of items
    (one launch of up to 16 weight sets).  status: optional int32 device
    word that f16x3 kernels set on a non-finite output (operand out of the split range)."""
    if not 1 <= len(groups) <= L.MAXG:
        raise ValueError(f"conv2d: 1..{L.MAXG} groups")
    parts = _split_by_mode(groups, "layer")
    if parts:
        for part in parts:
            conv2d(part, epi=epi, in1_mode=in1_mode, in1_scale=in1_scale, stride=stride, status=status)
        return
    g0 = groups[0]
    lay: PackedConv = g0["layer"]
    in0 = g0["in0"]
    _, H, W, C0 = in0.shape
    C1 = g0["in1"].shape[3] if in1_mode else 0
    ks = lay.ks
    if stride is None:
        stride = 1
    pad = ks // 2
    Ho = (H + 2 * pad - ks) // stride + 1
    Wo = (W + 2 * pad - ks) // stride + 1
    a = L.ConvArgs()
    for i, g in enumerate(groups):
        if g["layer"].cin != C0 + C1 or g["layer"].ks != ks:
            raise ValueError("conv2d: layer shape mismatch")
        a.in0[i] = _vp(g["in0"])
        a.in1[i] = _vp(g.get("in1"))
        a.w[i] = _vp(g["layer"].w)
        a.bias[i] = _vp(g["layer"].b)
        a.out[i] = _vp(g["out"])
        a.res[i] = _vp(g.get("res"))
        a.out2[i] = _vp(g.get("out2"))
        nitems = g["in0"].shape[0]
        if tuple(g["in0"].shape[1:]) != (H, W, C0):
            raise ValueError(f"conv2d: in0 shape {tuple(g['in0'].shape)} != {(nitems, H, W, C0)}")
        if tuple(g["out"].shape[:3]) != (nitems, Ho, Wo):
            raise ValueError(f"conv2d: output shape {tuple(g['out'].shape)} != {(nitems, Ho, Wo)}")
        for k in ("in1", "res", "out2"):
            if g.get(k) is not None and g[k].shape[0] != nitems:
                raise ValueError(f"conv2d: {k} holds {g[k].shape[0]} items, in0 {nitems}")
    a.in0_item = _item_stride([g["in0"] for g in groups], "in0")
    a.in1_item = _item_stride([g.get("in1") for g in groups], "in1") if in1_mode else 0
    a.out_item = _item_stride([g["out"] for g in groups], "out")
    a.res_item = _item_stride([g.get("res") for g in groups], "res")
    a.out2_item = _item_stride([g.get("out2") for g in groups], "out2")
    total = _set_items(a, [g["in0"].shape[0] for g in groups])
    a.H, a.W, a.C0, a.C1 = H, W, C0, C1
    a.in1_mode, a.in1_scale = in1_mode, in1_scale
    a.Ho, a.Wo, a.cout, a.ks, a.stride, a.epi = Ho, Wo, lay.cout, ks, stride, epi
    wmodes = (L.PACK_WINO, L.PACK_WINO_OFFMASK, L.PACK_WINO_LSTM)
    wino = (lay.mode & ~L.PACK_F16X3) in wmodes
    if any(((g["layer"].mode & ~L.PACK_F16X3) in wmodes) != wino or (g["layer"].mode ^ lay.mode) & L.PACK_F16X3
           for g in groups):
        raise ValueError("conv2d: groups mix Winograd / direct or f32 / f16x3 packings")
    a.flags = L.CONV_F16X3 if lay.mode & L.PACK_F16X3 else 0
    a.status = _vp(status)
    sched = _sched_buf() if wino else None
    a.sched = _vp(sched)
    if sched is not None:
        a.flags |= L.CONV_DYNAMIC
    trace = None
    if TRACE is not None:
        # algorithmic (direct-convolution) FLOPs, whichever algorithm runs
        # algorithmic HBM bytes: every input read once, every output written once
        px_in, px_out = H * W * total, Ho * Wo * total   # over the sets' own item counts
        c_in = C0 + (C1 if in1_mode == 1 else C1 / 4.0 if in1_mode == 2 else 0)
        c_out = 128 if epi == L.EPI_LSTM else lay.cout
        c_res = 64 if epi in (L.EPI_RES, L.EPI_LSTM) else 0
        trace = (("wino" if wino else "conv", ks, stride, epi, in1_mode, lay.cout),
                 2.0 * lay.cout * (C0 + C1) * ks * ks * Ho * Wo * total,
                 4.0 * (c_in * px_in + (c_out + c_res) * px_out))
    if wino:
        _launch("stif_conv3x3_wino", trace, L.lib().stif_conv3x3_wino, C.byref(a), _stream())
    else:
        _launch("stif_conv2d_nhwc", trace, L.lib().stif_conv2d_nhwc, C.byref(a), _stream())


def _pack_dev(what: str, weight, bias, mode: int, cout: int, cin: int, ks: int):
    """The front end of the four device packers: ``weight`` / ``bias`` (or None) checked as float32 CUDA tensors and
    made contiguous, and the PackedConv of a [cout, cin, ks, ks] layer in ``mode`` with its buffers sized by the
    library.  Returns (lib, weight, bias, layer); the caller launches its entry into ``layer.w`` / ``layer.b``."""
    if not (weight.is_cuda and weight.dtype == torch.float32):
        raise ValueError(f"{what}: expected a float32 CUDA weight")
    if bias is not None and not (bias.is_cuda and bias.dtype == torch.float32):
        raise ValueError(f"{what}: expected a float32 CUDA bias")
    weight = weight.detach().contiguous()
    bias = None if bias is None else bias.detach().contiguous()
    lib = L.lib()
    wd = torch.empty(lib.stif_conv_weight_floats(cout, cin, ks, mode), dtype=torch.float32, device=weight.device)
    bd = torch.empty(lib.stif_conv_bias_floats(cout, mode), dtype=torch.float32, device=weight.device)
    return lib, weight, bias, PackedConv(wd, bd, cout, cin, ks, mode)


def pack_conv_dev(weight: torch.Tensor, bias: Optional[torch.Tensor], mode: int = L.PACK_WINO, dgrad: bool = False,
                  status: Optional[torch.Tensor] = None) -> PackedConv:
    """The Winograd packing of a 64 -> 64 3x3 layer on the device (stif_pack_conv_weight_dev): ``weight`` [64,64,3,3]
    and ``bias`` [64] are device tensors and nothing passes through the host.  ``dgrad``: the data gradient's weight
    (transposed and rotated, zero bias; ``bias`` may be None).  With ``PACK_F16X3`` a weight outside the split-fp16
    range sets ``STATUS_PACK_RANGE`` in the int32 device word ``status`` (required then) instead of raising."""
    if weight.dim() != 4 or weight.shape[2] != weight.shape[3]:
        raise ValueError(f"pack_conv_dev: weight shape {tuple(weight.shape)} is not [cout, cin, k, k]")
    cout, cin, ks, _ = weight.shape
    lib, w, b, lay = _pack_dev("pack_conv_dev", weight, bias, mode, cin if dgrad else cout, cout if dgrad else cin, ks)
    _launch("stif_pack_conv_weight_dev", None, lib.stif_pack_conv_weight_dev, _vp(w), _vp(b), cout, cin, ks, mode,
            L.PACK_DGRAD if dgrad else 0, _vp(lay.w), _vp(lay.b), _vp(status), _stream())
    return lay


# The weight gradients' workspace (the workgroups' partial sums): one buffer per (device, stream), grown on demand;
# launches on one stream run in issue order, launches on different streams never share one
_WGRAD_WS = {}


def _wgrad_workspace(device, nbytes: int):
    """The (device, stream) partial-sum buffer grown to ``nbytes``: every weight-gradient reduction shares it (each
    finishes its reduce before the next launch on the stream starts)."""
    s = torch.cuda.current_stream(device)
    key = (s.device.index, s.cuda_stream)
    ws = _WGRAD_WS.get(key)
    if ws is None or ws.numel() * 4 < nbytes:
        ws = _WGRAD_WS[key] = torch.empty(max(nbytes // 4, 4), dtype=torch.float32, device=device)
    return ws, s.cuda_stream


def _wgrad_call(entry: str, fn, nbytes: int, a, gy: torch.Tensor, gw_shape, trace):
    """What the struct-taking weight-gradient wrappers share once their maps are checked and ``a`` (ConvWgradArgs or
    ConvWgradCatArgs) holds the x maps, the item strides and the sizes: the workspace of ``nbytes``, gw [gw_shape] and
    gb, the rest of ``a`` and the launch of the library entry ``fn``.  Returns (gw, gb)."""
    ws, stream = _wgrad_workspace(gy.device, nbytes)
    gw = torch.empty(gw_shape, dtype=torch.float32, device=gy.device)
    gb = torch.empty(gw_shape[0], dtype=torch.float32, device=gy.device)
    a.gy, a.gw, a.gb = _vp(gy), _vp(gw), _vp(gb)
    a.workspace, a.workspace_bytes = _vp(ws), ws.numel() * 4
    _launch(entry, trace, fn, C.byref(a), stream)
    return gw, gb


def _wgrad64_args(what_x: str, what_gy: str, x, gy):
    """ConvWgradArgs of a 64 -> 64 weight gradient: the maps' item strides (checked) and the sizes of ``x``."""
    a = L.ConvWgradArgs()
    a.x, a.x_item, a.gy_item = _vp(x), _item_stride([x], what_x), _item_stride([gy], what_gy)
    a.n, a.H, a.W, a.cin, a.cout = x.shape[0], x.shape[1], x.shape[2], 64, 64
    return a


def _wgrad_cat_args(what_x: str, what_gy: str, xs, gy, cout: int):
    """ConvWgradCatArgs of a weight gradient on one or two 64-channel x maps: item strides (checked) and sizes."""
    a = L.ConvWgradCatArgs()
    for i, x in enumerate(xs):
        a.x[i], a.x_item[i] = _vp(x), _item_stride([x], what_x)
    a.gy_item = _item_stride([gy], what_gy)
    a.n, a.H, a.W, a.nx, a.gy_channels, a.cout = gy.shape[0], gy.shape[1], gy.shape[2], len(xs), gy.shape[3], cout
    return a


def conv3x3_wgrad(x: torch.Tensor, gy: torch.Tensor):
    """Weight and bias gradient of the 3x3 / stride-1 / 64 -> 64 'same' conv: NHWC ``x`` (the forward's input) and
    ``gy`` (the gradient of its output), [n, H, W, 64] fp32 with any item stride, pixels contiguous -- as ops.conv2d
    reads its inputs.  Returns (gw [64, 64, 3, 3] in the state dict's OIHW order, gb [64]); repeated calls give
    identical bits (no atomics)."""
    if x.dim() != 4 or x.shape != gy.shape or x.shape[3] != 64:
        raise ValueError(f"conv3x3_wgrad: x {tuple(x.shape)} and gy {tuple(gy.shape)} must both be [n, H, W, 64]")
    n, H, W, _ = x.shape
    trace = None if TRACE is None else (("wgrad",), 2.0 * 64 * 64 * 9 * n * H * W, 4.0 * 2 * 64 * n * H * W)
    lib = L.lib()
    a = _wgrad64_args("conv3x3_wgrad x", "conv3x3_wgrad gy", x, gy)
    return _wgrad_call("stif_conv3x3_wgrad", lib.stif_conv3x3_wgrad,
                       lib.stif_conv3x3_wgrad_workspace_size(n, H, W, 64, 64), a, gy, (64, 64, 3, 3), trace)


def conv3x3s2_wgrad(x: torch.Tensor, gy: torch.Tensor):
    """Weight and bias gradient of the 3x3 / stride-2 / pad-1 / 64 -> 64 conv: NHWC ``x`` [n, H, W, 64] (the forward's
    input) and ``gy`` [n, (H + 1) // 2, (W + 1) // 2, 64], conventions and determinism of conv3x3_wgrad.  Returns
    (gw [64, 64, 3, 3] OIHW, gb [64])."""
    if x.dim() != 4 or gy.dim() != 4 or x.shape[3] != 64:
        raise ValueError(f"conv3x3s2_wgrad: x {tuple(x.shape)} and gy {tuple(gy.shape)} must be [n, H, W, 64] maps")
    n, H, W, _ = x.shape
    if tuple(gy.shape) != (n, (H + 1) // 2, (W + 1) // 2, 64):
        raise ValueError(f"conv3x3s2_wgrad: gy {tuple(gy.shape)} is not the stride-2 output of x {tuple(x.shape)}")
    px = n * gy.shape[1] * gy.shape[2]
    trace = None if TRACE is None else (("wgrad_s2",), 2.0 * 64 * 64 * 9 * px, 4.0 * 64 * (n * H * W + px))
    lib = L.lib()
    a = _wgrad64_args("conv3x3s2_wgrad x", "conv3x3s2_wgrad gy", x, gy)
    return _wgrad_call("stif_conv3x3s2_wgrad", lib.stif_conv3x3s2_wgrad,
                       lib.stif_conv3x3s2_wgrad_workspace_size(n, H, W, 64, 64), a, gy, (64, 64, 3, 3), trace)


def conv3x3s2_dgrad(gy: torch.Tensor, weight: torch.Tensor, H: int, W: int) -> torch.Tensor:
    """Data gradient of the 3x3 / stride-2 / pad-1 / 64 -> 64 conv: NHWC ``gy`` [n, (H + 1) // 2, (W + 1) // 2, 64]
    (any item stride) and the state dict's ``weight`` [64, 64, 3, 3] on the device; returns gx [n, H, W, 64]."""
    if gy.dim() != 4 or tuple(gy.shape[1:]) != ((H + 1) // 2, (W + 1) // 2, 64):
        raise ValueError(f"conv3x3s2_dgrad: gy {tuple(gy.shape)} is not the stride-2 output of a {H} x {W} map")
    gy_item = _item_stride([gy], "conv3x3s2_dgrad gy")
    if not (weight.is_cuda and weight.dtype == torch.float32) or tuple(weight.shape) != (64, 64, 3, 3):
        raise ValueError("conv3x3s2_dgrad: expected a float32 CUDA weight [64, 64, 3, 3]")
    weight = weight.detach().contiguous()
    n = gy.shape[0]
    gx = torch.empty(n, H, W, 64, dtype=torch.float32, device=gy.device)
    trace = None
    if TRACE is not None:
        px = n * gy.shape[1] * gy.shape[2]
        trace = (("dgrad_s2",), 2.0 * 64 * 64 * 9 * px, 4.0 * 64 * (n * H * W + px))
    _launch("stif_conv3x3s2_dgrad", trace, L.lib().stif_conv3x3s2_dgrad, _vp(gy), _vp(weight), _vp(gx), gy_item,
            H * W * 64, n, H, W, None, 0, torch.cuda.current_stream(gy.device).cuda_stream)
    return gx


def conv_first_wgrad(x_nchw: torch.Tensor, gy: torch.Tensor):
    """Weight and bias gradient of conv_first (3 -> 64, 3x3 'same'): the contiguous NCHW frames ``x_nchw`` [n, 3, h, w]
    as ops.conv_first reads them and NHWC ``gy`` [n, h, w, 64] (any item stride).  Returns (gw [64, 3, 3, 3], gb [64]);
    repeated calls give identical bits."""
    if x_nchw.dim() != 4 or x_nchw.shape[1] != 3 or gy.dim() != 4:
        raise ValueError(f"conv_first_wgrad: x {tuple(x_nchw.shape)} must be [n, 3, h, w] and gy [n, h, w, 64]")
    n, _, h, w = x_nchw.shape
    if tuple(gy.shape) != (n, h, w, 64):
        raise ValueError(f"conv_first_wgrad: gy {tuple(gy.shape)} != {(n, h, w, 64)}")
    gy_item = _item_stride([gy], "conv_first_wgrad gy")
    if not (x_nchw.is_cuda and x_nchw.dtype == torch.float32 and x_nchw.is_contiguous()):
        raise ValueError("conv_first_wgrad: expected contiguous float32 CUDA frames")
    lib = L.lib()
    ws, stream = _wgrad_workspace(gy.device, lib.stif_conv_first_wgrad_workspace_size(n, h, w))
    gw = torch.empty(64, 3, 3, 3, dtype=torch.float32, device=gy.device)
    gb = torch.empty(64, dtype=torch.float32, device=gy.device)
    trace = None if TRACE is None else (("cf_wgrad",), 2.0 * 64 * 28 * n * h * w, 4.0 * (64 + 3) * n * h * w)
    # the one entry without an argument struct (NCHW frames, no x stride): it shares the workspace only
    _launch("stif_conv_first_wgrad", trace, lib.stif_conv_first_wgrad, _vp(x_nchw), _vp(gy), _vp(gw), _vp(gb), gy_item,
            n, h, w, _vp(ws), ws.numel() * 4, stream)
    return gw, gb


def pack_conv_plain_dev(weight: torch.Tensor, bias: Optional[torch.Tensor]) -> PackedConv:
    """The fp32 direct-conv (PACK_PLAIN) packing of a 64 -> 64 3x3 layer on the device (stif_pack_conv_plain_dev):
    the bytes ops.pack_conv writes, with nothing passing through the host -- the layer ops.conv2d(stride=2) reads."""
    if weight.dim() != 4 or weight.shape[2] != weight.shape[3]:
        raise ValueError(f"pack_conv_plain_dev: weight shape {tuple(weight.shape)} is not [cout, cin, k, k]")
    cout, cin, ks, _ = weight.shape
    lib, w, b, lay = _pack_dev("pack_conv_plain_dev", weight, bias, L.PACK_PLAIN, cout, cin, ks)
    _launch("stif_pack_conv_plain_dev", None, lib.stif_pack_conv_plain_dev, _vp(w), _vp(b), cout, cin, ks,
            _vp(lay.w), _vp(lay.b), _stream())
    return lay


def upsample2x(x: torch.Tensor, out: torch.Tensor, scale: float = 1.0):
    """out = scale * bilinear x2 upsample (align_corners=False) of NHWC x [n, h, w, c] (items may be
    strided; pixels contiguous) into out [n, 2h, 2w, c]."""
    n, h, w, c = x.shape
    if tuple(out.shape) != (n, 2 * h, 2 * w, c):
        raise ValueError(f"upsample2x: out shape {tuple(out.shape)} != {(n, 2 * h, 2 * w, c)}")
    if not (_pixels_contiguous(x) and _pixels_contiguous(out)):
        raise ValueError("upsample2x: pixels must be contiguous")
    _launch("stif_upsample2x_nhwc", (("up2",), 0.0), L.lib().stif_upsample2x_nhwc, _vp(x), _vp(out), n, h, w, c,
            float(scale), x.stride(0) if n > 1 else h * w * c, out.stride(0) if n > 1 else 4 * h * w * c, _stream())


def upsample2x_bwd(gy: torch.Tensor, scale: float = 1.0) -> torch.Tensor:
    """The adjoint of upsample2x: NHWC ``gy`` [n, 2h, 2w, c] (items may be strided; pixels contiguous, c % 4 == 0)
    -> a new gx [n, h, w, c], the transpose of scale * bilinear x2 (align_corners=False).  A gather: no atomics."""
    if gy.dim() != 4 or gy.shape[1] % 2 or gy.shape[2] % 2 or gy.shape[3] % 4 or 0 in gy.shape:
        raise ValueError(f"upsample2x_bwd: gy {tuple(gy.shape)} must be [n, 2h, 2w, c] with c % 4 == 0")
    gy_item = _item_stride([gy], "upsample2x_bwd gy")
    n, H, W, c = gy.shape
    gx = torch.empty(n, H // 2, W // 2, c, dtype=torch.float32, device=gy.device)
    trace = (("up2_bwd",), 0.0, 4.0 * 1.25 * c * n * H * W) if TRACE is not None else None
    _launch("stif_upsample2x_bwd_nhwc", trace, L.lib().stif_upsample2x_bwd_nhwc, _vp(gy), _vp(gx), n, H // 2, W // 2, c,
            float(scale), gy_item if n > 1 else H * W * c, (H // 2) * (W // 2) * c,
            torch.cuda.current_stream(gy.device).cuda_stream)
    return gx


def conv3x3_wgrad_cat(xs, gy: torch.Tensor, cout: int):
    """Weight and bias gradient of a 3x3 'same' conv in 64 x 64 channel blocks (stif_conv3x3_wgrad_cat).  ``xs``: the
    one or two NHWC 64-channel maps whose concatenation was the forward's input (never built); ``gy``: [n, H, W, 64] with
    ``cout`` = 64, the 256-channel map of the 64 -> 216 offset / mask conv with ``cout`` = 216 (channels 216.. are
    never read), or with two x maps the ConvLSTM cell's 256 pre-activation gradients with ``cout`` = 256.  Returns
    (gw [cout, 64 len(xs), 3, 3] OIHW, gb [cout]).  Every 64 x 64 block of gw has the bits conv3x3_wgrad returns for the
    same two maps; repeated calls give identical bits."""
    xs = list(xs)
    if len(xs) not in (1, 2) or gy.dim() != 4 or any(x.dim() != 4 or x.shape[3] != 64 or x.shape[:3] != gy.shape[:3]
                                                      for x in xs):
        raise ValueError(f"conv3x3_wgrad_cat: one or two x maps [n, H, W, 64] and a gy over the same pixels, got "
                         f"{[tuple(x.shape) for x in xs]} and {tuple(gy.shape)}")
    n, H, W, gc = gy.shape
    nx = len(xs)
    if (nx, gc, cout) not in ((2, 64, 64), (1, 256, 216), (1, 64, 64), (2, 256, 256)):
        raise ValueError(f"conv3x3_wgrad_cat: unsupported channel counts (nx, gy channels, cout) = {(nx, gc, cout)}")
    trace = None
    if TRACE is not None:
        blocks = nx * ((cout + 63) // 64)
        trace = (("wgrad_cat", nx, cout), 2.0 * cout * 64 * nx * 9 * n * H * W, 4.0 * (64 * blocks + cout) * n * H * W)
    lib = L.lib()
    a = _wgrad_cat_args("conv3x3_wgrad_cat x", "conv3x3_wgrad_cat gy", xs, gy, cout)
    return _wgrad_call("stif_conv3x3_wgrad_cat", lib.stif_conv3x3_wgrad_cat,
                       lib.stif_conv3x3_wgrad_cat_workspace_size(n, H, W, nx, gc, cout), a, gy, (cout, 64 * nx, 3, 3),
                       trace)


# pack_conv_blocks_dev's forms: (weight [cout, cin], dgrad, half) -> (the PackedConv's cout and cin, the (co0, ci0)
# of its 64 x 64 blocks in buffer order)
_ROWS4 = tuple(64 * s for s in range(4))
_BLOCK_FORMS = {
    ((64, 128), False, None): (64, 128, ((0, 0), (0, 64))),
    ((216, 64), False, None): (256, 64, tuple((r, 0) for r in _ROWS4)),
    ((216, 64), True, None): (64, 256, tuple((r, 0) for r in _ROWS4)),
    ((64, 128), True, 0): (64, 64, ((0, 0),)),
    ((64, 128), True, 1): (64, 64, ((0, 64),)),
    ((256, 128), False, None): (256, 128, tuple((r, c) for r in _ROWS4 for c in (0, 64))),
    ((256, 128), True, 0): (64, 256, tuple((r, 0) for r in _ROWS4)),
    ((256, 128), True, 1): (64, 256, tuple((r, 64) for r in _ROWS4)),
}


def pack_conv_blocks_dev(weight: torch.Tensor, bias: Optional[torch.Tensor], mode: int = L.PACK_WINO,
                         dgrad: bool = False, half: Optional[int] = None,
                         status: Optional[torch.Tensor] = None) -> PackedConv:
    """The Winograd packing on the device of PCD_Align's wider 3x3 layers, as 64 x 64 block packs
    (stif_pack_conv_block_dev) laid end to end in one buffer:

    * ``weight`` [64, 128]: the 128 -> 64 layer (the bytes of ops.pack_conv), its two column blocks;
    * ``weight`` [216, 64]: the 64 -> 216 layer with its rows zero-padded to 256 (the bytes of ops.pack_conv; the
      PackedConv says cout = 256, which is what stif_conv3x3_wino writes), its four row blocks;
    * ``weight`` [216, 64], ``dgrad``: the data gradient's 256 -> 64 layer, the four DGRAD row blocks;
    * ``weight`` [64, 128], ``dgrad``, ``half`` = 0 or 1: the data gradient's 64 -> 64 layer of that input half;
    * ``weight`` [256, 128]: the ConvLSTM cell's 128 -> 256 layer in the reference's row order (the bytes of
      ops.pack_conv with PACK_WINO), its eight blocks in row order;
    * ``weight`` [256, 128], ``dgrad``, ``half`` = 0 or 1: the data gradient's 256 -> 64 layer of that input half, four
      DGRAD row blocks.

    ``bias`` may be None with ``dgrad`` (the bias is zero then); ``status`` as ops.pack_conv_dev."""
    shape = tuple(weight.shape)
    form = _BLOCK_FORMS.get((shape[:2], bool(dgrad), half)) if shape[2:] == (3, 3) else None
    if form is None:
        raise ValueError(f"pack_conv_blocks_dev: no block form for weight {shape}, dgrad={dgrad}, half={half}")
    cout, cin, blocks = form
    lib, w, b, lay = _pack_dev("pack_conv_blocks_dev", weight, bias, mode, cout, cin, 3)
    per = lay.w.numel() // len(blocks)
    for i, (co0, ci0) in enumerate(blocks):
        # the blocks of one cout slice share its 64 biases; a row block has its own
        bi = lay.b[co0:co0 + 64] if cout == 256 else lay.b
        _launch("stif_pack_conv_block_dev", None, lib.stif_pack_conv_block_dev, _vp(w), _vp(b), shape[0], shape[1],
                co0, ci0, mode, L.PACK_DGRAD if dgrad else 0, _vp(lay.w[i * per:]), _vp(bi), _vp(status), _stream())
    return lay


def conv1x1_wgrad(xs, gy: torch.Tensor):
    """Weight and bias gradient of the 1x1 conv on one or two 64-channel inputs (stif_conv1x1_wgrad): ``xs`` the NHWC
    maps whose concatenation was the forward's input (never built), ``gy`` [n, H, W, 64]; any item strides, pixels
    contiguous.  Returns (gw [64, 64 len(xs), 1, 1] OIHW, gb [64]); repeated calls give identical bits (no atomics)."""
    xs = list(xs)
    if len(xs) not in (1, 2) or gy.dim() != 4 or gy.shape[3] != 64 or any(x.dim() != 4 or x.shape != gy.shape
                                                                             for x in xs):
        raise ValueError(f"conv1x1_wgrad: one or two x maps and a gy, all [n, H, W, 64], got "
                         f"{[tuple(x.shape) for x in xs]} and {tuple(gy.shape)}")
    n, H, W, _ = gy.shape
    nx = len(xs)
    trace = None if TRACE is None else (("wgrad_1x1", nx), 2.0 * 64 * 64 * nx * n * H * W,
                                        4.0 * 64 * (1 + nx) * n * H * W)
    lib = L.lib()
    a = _wgrad_cat_args("conv1x1_wgrad x", "conv1x1_wgrad gy", xs, gy, 64)
    return _wgrad_call("stif_conv1x1_wgrad", lib.stif_conv1x1_wgrad, lib.stif_conv1x1_wgrad_workspace_size(n, H, W, nx),
                       a, gy, (64, 64 * nx, 1, 1), trace)


def pack_conv1x1_dev(weight: torch.Tensor, bias: Optional[torch.Tensor], mode: int = L.PACK_PLAIN, dgrad: bool = False,
                     half: Optional[int] = None, status: Optional[torch.Tensor] = None) -> PackedConv:
    """The packing on the device of a 1x1 (64 | 64) -> 64 layer (stif_pack_conv1x1_dev): ``weight`` [64, 128, 1, 1],
    ``mode`` PACK_PLAIN or PACK_PLAIN | PACK_F16X3 -- the bytes of ops.pack_conv, the layer ops.conv2d(in1_mode=1)
    reads.  ``dgrad`` with ``half`` = 0 or 1: the fp32 pack of the transposed 64 -> 64 layer of that input half (zero
    bias; ``bias`` may be None).  ``status`` as ops.pack_conv_dev."""
    if tuple(weight.shape) != (64, 128, 1, 1) or (half is not None) != dgrad or half not in (None, 0, 1):
        raise ValueError(f"pack_conv1x1_dev: no form for weight {tuple(weight.shape)}, dgrad={dgrad}, half={half}")
    lib, w, b, lay = _pack_dev("pack_conv1x1_dev", weight, bias, mode, 64, 64 if dgrad else 128, 1)
    _launch("stif_pack_conv1x1_dev", None, lib.stif_pack_conv1x1_dev, _vp(w), _vp(b), 64, 128,
            64 * half if dgrad else 0, mode, L.PACK_DGRAD if dgrad else 0, _vp(lay.w), _vp(lay.b), _vp(status),
            _stream())
    return lay


def _lstm_maps(what, pre, maps):
    """Check the gate kernels' maps (``pre`` [n, H, W, 256], the others [n, H, W, 64] or None); their item strides."""
    if pre.dim() != 4 or pre.shape[3] != 256 or 0 in pre.shape:
        raise ValueError(f"{what}: pre {tuple(pre.shape)} must be [n, H, W, 256]")
    want = tuple(pre.shape[:3]) + (64,)
    for name, t in maps:
        if t is not None and tuple(t.shape) != want:
            raise ValueError(f"{what}: {name} {tuple(t.shape)} must be {want}")
    return [_item_stride([t], f"{what} {name}") for name, t in [("pre", pre)] + list(maps)]


def lstm_gates(pre: torch.Tensor, c_cur: torch.Tensor, h_next: Optional[torch.Tensor] = None,
               c_next: Optional[torch.Tensor] = None):
    """The ConvLSTM cell's gates (stif_lstm_gates_nhwc): NHWC ``pre`` [n, H, W, 256] in the reference's row order
    (gates i, f, o, g of 64 hidden channels each) and ``c_cur`` [n, H, W, 64] -> (h_next, c_next), new tensors unless
    given.  Items may be strided; pixels contiguous."""
    n, H, W = pre.shape[:3] if pre.dim() == 4 else (0, 0, 0)
    if h_next is None:
        h_next = torch.empty(n, H, W, 64, dtype=torch.float32, device=pre.device)
    if c_next is None:
        c_next = torch.empty(n, H, W, 64, dtype=torch.float32, device=pre.device)
    items = _lstm_maps("lstm_gates", pre, [("c_cur", c_cur), ("h_next", h_next), ("c_next", c_next)])
    trace = (("lstm_gates",), 0.0, 4.0 * (256 + 3 * 64) * n * H * W) if TRACE is not None else None
    _launch("stif_lstm_gates_nhwc", trace, L.lib().stif_lstm_gates_nhwc, _vp(pre), _vp(c_cur), _vp(h_next), _vp(c_next),
            n, H, W, *items, torch.cuda.current_stream(pre.device).cuda_stream)
    return h_next, c_next


def lstm_gates_bwd(pre: torch.Tensor, c_cur: torch.Tensor, g_h: Optional[torch.Tensor],
                   g_c_next: Optional[torch.Tensor], need_c: bool = True, g_pre: Optional[torch.Tensor] = None,
                   g_c_cur: Optional[torch.Tensor] = None):
    """The backward of lstm_gates (stif_lstm_gates_bwd_nhwc), the gates recomputed from the forward's inputs ``pre``
    and ``c_cur``: ``g_h`` / ``g_c_next`` the gradients of its outputs, either None for zeros (not both).  Returns
    (g_pre [n, H, W, 256], g_c_cur [n, H, W, 64] or None when ``need_c`` is false)."""
    if g_h is None and g_c_next is None:
        raise ValueError("lstm_gates_bwd: g_h and g_c_next are both None")
    n, H, W = pre.shape[:3] if pre.dim() == 4 else (0, 0, 0)
    if g_pre is None:
        g_pre = torch.empty(n, H, W, 256, dtype=torch.float32, device=pre.device)
    if g_c_cur is None and need_c:
        g_c_cur = torch.empty(n, H, W, 64, dtype=torch.float32, device=pre.device)
    if tuple(g_pre.shape) != tuple(pre.shape):
        raise ValueError(f"lstm_gates_bwd: g_pre {tuple(g_pre.shape)} must be {tuple(pre.shape)}")
    items = _lstm_maps("lstm_gates_bwd", pre, [("c_cur", c_cur), ("g_h", g_h), ("g_c_next", g_c_next)])
    items += [_item_stride([g_pre], "lstm_gates_bwd g_pre")]
    items += _lstm_maps("lstm_gates_bwd", pre, [("g_c_cur", g_c_cur)])[1:]
    moved = 2 * 256 + 64 * (1 + (g_h is not None) + (g_c_next is not None) + (g_c_cur is not None))
    trace = (("lstm_gates_bwd",), 0.0, 4.0 * moved * n * H * W) if TRACE is not None else None
    _launch("stif_lstm_gates_bwd_nhwc", trace, L.lib().stif_lstm_gates_bwd_nhwc, _vp(pre), _vp(c_cur), _vp(g_h),
            _vp(g_c_next), _vp(g_pre), _vp(g_c_cur), n, H, W, *items, torch.cuda.current_stream(pre.device).cuda_stream)
    return g_pre, g_c_cur


# ----------------------------------------------------------------------------- the SIREN decoder for training
SIREN_WIDTHS = {3: (64, 64, 256), 4: (64, 64, 256, 256)}


def _round8(n: int) -> int:
    return (n + 7) // 8 * 8


def _siren_args(what, x, weights, biases):
    """The checks every SIREN call shares, before any launch; returns (args with x / w / b filled, n, kp, zw, cout)."""
    weights, biases = list(weights), list(biases)
    nsine = len(weights) - 1
    if nsine not in SIREN_WIDTHS or len(biases) != len(weights):
        raise ValueError(f"{what}: 4 or 5 weight / bias pairs (3 or 4 sine layers and the linear one), got "
                         f"{len(weights)} and {len(biases)}")
    for t in [x] + weights + biases:
        if not t.is_cuda:
            raise RuntimeError(f"{what}: the HIP kernels need CUDA tensors, got one on {t.device} "
                               "(move the module and its input to the GPU)")
        if t.dtype != torch.float32:
            raise ValueError(f"{what}: expected float32 tensors, got {t.dtype}")
    cin, cout = int(weights[0].shape[1]), int(weights[-1].shape[0])
    dims = [cin] + list(SIREN_WIDTHS[nsine]) + [cout]
    for l, (w, b) in enumerate(zip(weights, biases)):
        if tuple(w.shape) != (dims[l + 1], dims[l]) or tuple(b.shape) != (dims[l + 1],) or not w.is_contiguous():
            raise ValueError(f"{what}: layer {l} must be a contiguous [{dims[l + 1]}, {dims[l]}] weight with its bias "
                             f"(widths {SIREN_WIDTHS[nsine]}), got {tuple(w.shape)} and {tuple(b.shape)}")
    kp = _round8(cin)
    if x.dim() != 2 or x.shape[1] != kp or x.shape[0] < 1 or (x.shape[1] > 1 and x.stride(1) != 1):
        raise ValueError(f"{what}: x must be [n >= 1, {kp}] ({cin} inputs and zero pad columns) with contiguous rows, "
                         f"got {tuple(x.shape)}")
    a = L.SirenArgs()
    a.x, a.x_stride = _vp(x), x.stride(0)
    a.n, a.cin, a.nsine, a.cout = x.shape[0], cin, nsine, cout
    for l, wd in enumerate(SIREN_WIDTHS[nsine]):
        a.width[l] = wd
    for l, (w, b) in enumerate(zip(weights, biases)):
        a.w[l], a.b[l] = _vp(w), _vp(b)
    return a, x.shape[0], kp, sum(SIREN_WIDTHS[nsine]), cout


def siren_fwd(x: torch.Tensor, weights, biases, y: Optional[torch.Tensor] = None, z: Optional[torch.Tensor] = None):
    """A SIREN MLP on the rows of ``x`` for training (stif_siren_fwd): ``x`` [n, round8(cin)] fp32 with zero pad
    columns (rows may be strided by a multiple of 8), ``weights`` / ``biases`` the parameter tensors of the 3 or 4
    sine layers and the final linear layer.  Returns (y [n, cout], z [n, 384 or 640]): the output and the saved
    pre-activations of the sine layers."""
    a, n, _, zw, cout = _siren_args("siren_fwd", x, weights, biases)
    if y is None:
        y = torch.empty(n, cout, dtype=torch.float32, device=x.device)
    if z is None:
        z = torch.empty(n, zw, dtype=torch.float32, device=x.device)
    if tuple(y.shape) != (n, cout) or tuple(z.shape) != (n, zw) or not y.is_contiguous() or not z.is_contiguous():
        raise ValueError(f"siren_fwd: y must be a contiguous [{n}, {cout}] and z [{n}, {zw}]")
    a.y, a.z = _vp(y), _vp(z)
    trace = None
    if TRACE is not None:
        macs = sum(int(w.numel()) for w in weights)
        trace = (("siren_fwd", a.cin, cout), 2.0 * macs * n, 4.0 * n * (x.shape[1] + 2 * zw + cout))
    _launch("stif_siren_fwd", trace, L.lib().stif_siren_fwd, C.byref(a), torch.cuda.current_stream(x.device).cuda_stream)
    return y, z


def siren_bwd(x: torch.Tensor, z: torch.Tensor, weights, biases, g_y: torch.Tensor, need_x: bool = True,
              g_x: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None, g_params=None):
    """The backward of siren_fwd (stif_siren_bwd) from ``g_y`` [n, cout], ``x`` and the saved ``z``: returns
    (g_x [n, round8(cin)] with zero pad columns, or None without ``need_x``; the weight gradients; the bias
    gradients).  The weight and bias gradients are deterministic (no atomics, whatever ``workspace`` held).
    ``g_params``: (weight gradients, bias gradients) to write into, contiguous and shaped as the parameters."""
    a, n, kp, zw, cout = _siren_args("siren_bwd", x, weights, biases)
    for name, t, shape in (("z", z, (n, zw)), ("g_y", g_y, (n, cout))):
        if not t.is_cuda or t.dtype != torch.float32 or tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f"siren_bwd: {name} must be a contiguous float32 CUDA [{shape[0]}, {shape[1]}]")
    lib = L.lib()
    a.z, a.g_y = _vp(z), _vp(g_y)
    if need_x:
        if g_x is None:
            g_x = torch.empty(n, kp, dtype=torch.float32, device=x.device)
        if g_x.dim() != 2 or tuple(g_x.shape) != (n, kp) or g_x.stride(1) != 1:
            raise ValueError(f"siren_bwd: g_x must be [{n}, {kp}] with contiguous rows")
        a.g_x, a.gx_stride = _vp(g_x), g_x.stride(0)
    else:
        g_x = None
    if g_params is None:
        g_ws, g_bs = [torch.empty_like(w) for w in weights], [torch.empty_like(b) for b in biases]
    else:
        g_ws, g_bs = list(g_params[0]), list(g_params[1])
        for g, p in zip(g_ws + g_bs, list(weights) + list(biases)):
            if not g.is_cuda or g.dtype != torch.float32 or g.shape != p.shape or not g.is_contiguous():
                raise ValueError("siren_bwd: g_params must be contiguous float32 CUDA tensors shaped as the parameters")
    for l, (gw, gb) in enumerate(zip(g_ws, g_bs)):
        a.g_w[l], a.g_b[l] = _vp(gw), _vp(gb)
    nbytes = lib.stif_siren_bwd_workspace_size(n, a.nsine)
    if workspace is None:
        workspace = torch.empty(nbytes // 4, dtype=torch.float32, device=x.device)
    a.workspace, a.workspace_bytes = _vp(workspace), workspace.numel() * workspace.element_size()
    trace = None
    if TRACE is not None:
        macs = sum(int(w.numel()) for w in weights)
        trace = (("siren_bwd", a.cin, cout), (4.0 if need_x else 4.0 - 2.0 * weights[0].numel() / macs) * macs * n,
                 4.0 * n * (x.shape[1] * (2 if need_x else 1) + 4 * zw + cout))
    _launch("stif_siren_bwd", trace, lib.stif_siren_bwd, C.byref(a), torch.cuda.current_stream(x.device).cuda_stream)
    return g_x, g_ws, g_bs


_DEC_TRAIN_TABLES = {}   # (h, w, HH, WW, device index) -> the uploaded tables of coords.dec_train_tables


class DecTrainGeom:
    """The geometry of one training decode (stif_dec_train_geom) and the tensors it points to: the NHWC latent
    ``feat`` [B, H, W, 192], the planar frames [B, 6, H, W], a time per item ``t`` [B] and the per-axis tables of
    the HH x WW query grid (uploaded once per size and device).  Refuses CPU tensors, wrong channel counts and
    HH or WW < 2 before anything is launched."""

    def __init__(self, feat: torch.Tensor, frames: torch.Tensor, t: torch.Tensor, HH: int, WW: int):
        HH, WW = int(HH), int(WW)
        for name, v in (("feat", feat), ("frames", frames), ("t", t)):
            if not v.is_cuda:
                raise RuntimeError(f"DecTrainGeom: the HIP kernels need CUDA tensors, got {name} on {v.device} "
                                   "(move the module and its input to the GPU)")
            if v.dtype != torch.float32 or not v.is_contiguous():
                raise ValueError(f"DecTrainGeom: {name} must be a contiguous float32 tensor")
        if feat.dim() != 4 or feat.shape[3] != 192 or 0 in feat.shape:
            raise ValueError(f"DecTrainGeom: feat must be the NHWC latent [B, H, W, 192], got {tuple(feat.shape)}")
        B, H, W, _ = feat.shape
        if tuple(frames.shape) != (B, 6, H, W):
            raise ValueError(f"DecTrainGeom: frames must be [{B}, 6, {H}, {W}], got {tuple(frames.shape)}")
        if tuple(t.shape) != (B,):
            raise ValueError(f"DecTrainGeom: t must be [{B}], got {tuple(t.shape)}")
        if HH < 2 or WW < 2:
            raise ValueError(f"DecTrainGeom: HH and WW must be at least 2 (the warp grid divides by n - 1), got "
                             f"{HH} x {WW}")
        key = (H, W, HH, WW, feat.device.index)
        tabs = _DEC_TRAIN_TABLES.get(key)
        if tabs is None:
            host = dec_train_tables(H, W, HH, WW)
            tabs = _DEC_TRAIN_TABLES[key] = {n: torch.from_numpy(np.ascontiguousarray(host[n])).to(feat.device)
                                             for n in L.DEC_TRAIN_TABLES}
        self.feat, self.frames, self.t, self.tables = feat, frames, t, tabs
        self.B, self.H, self.W, self.HH, self.WW, self.N = B, H, W, HH, WW, B * HH * WW
        g = self.c = L.DecTrainGeom()
        g.B, g.H, g.W, g.HH, g.WW = B, H, W, HH, WW
        g.feat, g.frames, g.t = _vp(feat), _vp(frames), _vp(t)
        for n in L.DEC_TRAIN_TABLES:
            setattr(g, n, _vp(tabs[n]))

    def _mat(self, what, t, width, make=torch.empty):
        if t is None:
            return make(self.N, width, dtype=torch.float32, device=self.feat.device)
        if not t.is_cuda or t.dtype != torch.float32 or tuple(t.shape) != (self.N, width) or not t.is_contiguous():
            raise ValueError(f"{what} must be a contiguous float32 CUDA [{self.N}, {width}], got {tuple(t.shape)}")
        return t

    def _lat(self, what, t):
        if t is None:
            return torch.empty_like(self.feat)
        if not t.is_cuda or t.dtype != torch.float32 or t.shape != self.feat.shape or not t.is_contiguous():
            raise ValueError(f"{what} must be a contiguous float32 CUDA {tuple(self.feat.shape)}, got {tuple(t.shape)}")
        return t

    def _run(self, name, trace, *ptrs):
        _launch(name, trace, getattr(L.lib(), name), C.byref(self.c), *ptrs,
                torch.cuda.current_stream(self.feat.device).cuda_stream)


def dec_x1_fwd(g: DecTrainGeom, x1: Optional[torch.Tensor] = None) -> torch.Tensor:
    """feat_imnet's input matrix X1 [N, 208] (stif_dec_x1_fwd): nearest latent and frames, rel_coord, t, zero pad."""
    x1 = g._mat("dec_x1_fwd: x1", x1, 208)
    trace = (("dec_x1_fwd",), 0.0, 4.0 * g.N * (208 + 192)) if TRACE is not None else None
    g._run("stif_dec_x1_fwd", trace, _vp(x1))
    return x1


def dec_x1_bwd(g: DecTrainGeom, g_x1: torch.Tensor, g_feat: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The adjoint of dec_x1_fwd with respect to the latent (stif_dec_x1_bwd), gather form: g_feat [B, H, W, 192]."""
    g_x1 = g._mat("dec_x1_bwd: g_x1", g_x1, 208)
    g_feat = g._lat("dec_x1_bwd: g_feat", g_feat)
    trace = (("dec_x1_bwd",), 0.0, 4.0 * (g.N * 192 + g_feat.numel())) if TRACE is not None else None
    g._run("stif_dec_x1_bwd", trace, _vp(g_x1), _vp(g_feat))
    return g_feat


def dec_x2_fwd(g: DecTrainGeom, hrfeat: torch.Tensor, x2: Optional[torch.Tensor] = None) -> torch.Tensor:
    """flow_imnet's input matrix X2 [N, 264] (stif_dec_x2_fwd): HRfeat, the bilinear latent and frames at the fixed
    query grid, t, zero pad."""
    hrfeat = g._mat("dec_x2_fwd: hrfeat", hrfeat, 64)
    x2 = g._mat("dec_x2_fwd: x2", x2, 264)
    trace = (("dec_x2_fwd",), 0.0, 4.0 * g.N * (264 + 64 + 192)) if TRACE is not None else None
    g._run("stif_dec_x2_fwd", trace, _vp(hrfeat), _vp(x2))
    return x2


def dec_x2_bwd(g: DecTrainGeom, g_x2: torch.Tensor, g_hrfeat: Optional[torch.Tensor] = None,
               g_feat: Optional[torch.Tensor] = None):
    """The adjoint of dec_x2_fwd (stif_dec_x2_bwd), gather form: (g_hrfeat [N, 64], g_feat [B, H, W, 192])."""
    g_x2 = g._mat("dec_x2_bwd: g_x2", g_x2, 264)
    g_hrfeat = g._mat("dec_x2_bwd: g_hrfeat", g_hrfeat, 64)
    g_feat = g._lat("dec_x2_bwd: g_feat", g_feat)
    trace = (("dec_x2_bwd",), 0.0, 4.0 * (g.N * (192 + 128) + g_feat.numel())) if TRACE is not None else None
    g._run("stif_dec_x2_bwd", trace, _vp(g_x2), _vp(g_hrfeat), _vp(g_feat))
    return g_hrfeat, g_feat


def dec_x3_fwd(g: DecTrainGeom, hrfeat: torch.Tensor, flow: torch.Tensor,
               x3: Optional[torch.Tensor] = None) -> torch.Tensor:
    """encode_imnet's input matrix X3 [N, 528] (stif_dec_x3_fwd): HRfeat, latent and frames at the two warped grids
    of ``flow`` [N, 4] (x1, y1, x2, y2 in HR pixels), t, zero pad."""
    hrfeat = g._mat("dec_x3_fwd: hrfeat", hrfeat, 64)
    flow = g._mat("dec_x3_fwd: flow", flow, 4)
    x3 = g._mat("dec_x3_fwd: x3", x3, 528)
    trace = (("dec_x3_fwd",), 0.0, 4.0 * g.N * (528 + 4 * 524)) if TRACE is not None else None
    g._run("stif_dec_x3_fwd", trace, _vp(hrfeat), _vp(flow), _vp(x3))
    return x3


def segsum(dst: torch.Tensor, src: torch.Tensor, row_stride: int, K: int, col0: int, w: torch.Tensor,
           sorted_words: torch.Tensor, seg: torch.Tensor) -> torch.Tensor:
    """The ordered segment sum stif_segsum (stif.h states the value): ``dst`` [D, C] float32 (C = 8, 64 or 192, every
    row overwritten), ``src`` the float32 buffer of sub-rows, ``w`` [E] float32, ``sorted_words`` [E] int64 -- the
    packed words (key << 32) | entry in ascending order -- and ``seg`` [D + 1] int64, seg[d] the index of the first
    word whose key is >= d.  No atomics: identical bits on every call."""
    if dst.dim() != 2 or dst.dtype != torch.float32 or not dst.is_cuda or not dst.is_contiguous():
        raise ValueError(f"segsum: dst must be a contiguous float32 CUDA [D, C], got {tuple(dst.shape)}")
    D, Cc = dst.shape
    E = w.numel()
    for name, t, dt, numel in (("src", src, torch.float32, None), ("w", w, torch.float32, E),
                               ("sorted_words", sorted_words, torch.int64, E), ("seg", seg, torch.int64, D + 1)):
        if t.dtype != dt or t.device != dst.device or not t.is_contiguous() or (numel is not None and t.numel() != numel):
            raise ValueError(f"segsum: {name} must be a contiguous {dt} tensor on {dst.device}"
                             + (f" of {numel} elements" if numel is not None else ""))
    rows = ((E + 3) // 4 + K - 1) // max(K, 1)
    if K >= 1 and src.numel() < (rows - 1) * row_stride + K * Cc + col0:
        raise ValueError(f"segsum: src holds {src.numel()} floats, fewer than {rows} rows of {row_stride}")
    trace = (("segsum", Cc), 2.0 * E * Cc, 4.0 * (D * Cc + E * (Cc / 4 + 3))) if TRACE is not None else None
    _launch("stif_segsum", trace, L.lib().stif_segsum, _vp(dst), _vp(src), row_stride, K, col0, _vp(w),
            _vp(sorted_words), _vp(seg), D, E, Cc, torch.cuda.current_stream(dst.device).cuda_stream)
    return dst


class GradTable:
    """The device table of one ``grad_pack`` layout (stif.h stif_grad_seg): segment i holds ``sizes[i]`` floats at
    ``offsets[i]``, each offset the previous end rounded up to 4 floats; ``floats`` is the end of the last segment,
    rounded.  Sizes, offsets and the chunk prefix are fixed; the source pointers are refreshed by ``update`` and
    uploaded (from pinned memory, on the current stream, nothing read back) only when one of them changed."""

    def __init__(self, sizes, device):
        self.sizes = tuple(int(s) for s in sizes)
        if not self.sizes or len(self.sizes) > L.GRAD_MAX_SEGS or min(self.sizes) < 0:
            raise ValueError(f"grad_pack: 1 .. {L.GRAD_MAX_SEGS} tensors, got {len(self.sizes)}")
        host = np.zeros((len(self.sizes), 4), np.int64)
        off = chunk = 0
        for i, n in enumerate(self.sizes):
            host[i, 1:] = (off, n, chunk)
            off += (n + 3) & ~3
            chunk += -(-n // L.GRAD_CHUNK)
        self.offsets, self.floats = host[:, 1].tolist(), off
        self.device = torch.device(device)
        self.host = torch.from_numpy(host)
        self.ptrs = self.dev = self._uploaded = None
        if self.device.type == "cuda":
            self.host = self.host.pin_memory()
            self.dev = torch.empty((len(self.sizes), 4), dtype=torch.int64, device=self.device)

    def update(self, tensors):
        ptrs = [t.data_ptr() for t in tensors]
        if ptrs == self.ptrs:
            return
        if self._uploaded is not None:
            self._uploaded.synchronize()      # the pinned rows may still be on their way from the last change
        self.host[:, 0] = torch.tensor(ptrs, dtype=torch.int64)
        self.dev.copy_(self.host, non_blocking=True)
        self._uploaded = torch.cuda.Event()
        self._uploaded.record(torch.cuda.current_stream(self.device))
        self.ptrs = ptrs


def grad_pack(tensors: Sequence[torch.Tensor], arena: torch.Tensor, table: Optional[GradTable] = None) -> GradTable:
    """stif_grad_pack: the contiguous float32 CUDA ``tensors`` (views at any 4-byte offset included) gathered into the
    1-d float32 ``arena`` in one launch, tensor i at ``table.offsets[i]``; the gap after each tensor up to a multiple
    of 4 floats and the arena's tail are written as +0.0.  The device table is built once per layout (the tensors'
    sizes) and returned: hand it back as ``table`` on the next call and only changed source pointers are uploaded.
    Runs on the current stream (use a table on one stream only) and reads nothing back."""
    tensors = list(tensors)
    if arena.dim() != 1 or arena.dtype != torch.float32 or not arena.is_cuda or not arena.is_contiguous():
        raise ValueError(f"grad_pack: arena must be a contiguous 1-d float32 CUDA tensor, got {arena.dtype} "
                         f"{tuple(arena.shape)} on {arena.device}")
    dev = arena.get_device()
    for i, t in enumerate(tensors):
        if t.dtype is not torch.float32 or not t.is_cuda or t.get_device() != dev or not t.is_contiguous():
            raise ValueError(f"grad_pack: tensor {i} must be a contiguous float32 tensor on {arena.device}, got "
                             f"{t.dtype} {tuple(t.shape)} (strides {t.stride()}) on {t.device}")
    sizes = tuple(t.numel() for t in tensors)
    if table is None or table.sizes != sizes or table.device != arena.device:
        table = GradTable(sizes, arena.device)
    if table.floats > arena.numel():
        raise ValueError(f"grad_pack: the layout needs {table.floats} floats, the arena holds {arena.numel()}")
    with torch.cuda.device(arena.device):
        table.update(tensors)
        moved = 4.0 * (sum(sizes) + arena.numel())
        trace = (("grad_pack", len(sizes)), 0.0, moved) if TRACE is not None else None
        _launch("stif_grad_pack", trace, L.lib().stif_grad_pack, _vp(table.dev), len(sizes), _vp(arena), arena.numel(),
                torch.cuda.current_stream(arena.device).cuda_stream)
    return table


def rank_sum(slab: torch.Tensor, dst: torch.Tensor) -> torch.Tensor:
    """stif_rank_sum: ``dst`` [n] = ((slab[0] + slab[1]) + ...) + slab[R - 1], plain fp32 adds in row order -- the
    cross-rank gradient sum with a defined order.  ``slab`` float32 CUDA [R, row] with
    contiguous rows of at least n floats, R <= 64, n a multiple of 4; ``dst`` must not overlap it.  Identical bits on
    every call; runs on the current stream and reads nothing back."""
    if slab.dim() != 2 or slab.dtype != torch.float32 or not slab.is_cuda or (slab.shape[1] > 1 and slab.stride(1) != 1):
        raise ValueError(f"rank_sum: slab must be a float32 CUDA [R, row] with contiguous rows, got {slab.dtype} "
                         f"{tuple(slab.shape)} on {slab.device}")
    if dst.dim() != 1 or dst.dtype != torch.float32 or dst.device != slab.device or not dst.is_contiguous():
        raise ValueError(f"rank_sum: dst must be a contiguous 1-d float32 tensor on {slab.device}")
    R, n = slab.shape[0], dst.numel()
    if n > slab.shape[1]:
        raise ValueError(f"rank_sum: dst holds {n} floats, a slab row {slab.shape[1]}")
    row = slab.stride(0) if R > 1 else max(slab.shape[1], n)
    trace = (("rank_sum", R), float((R - 1) * n), 4.0 * (R + 1) * n) if TRACE is not None else None
    _launch("stif_rank_sum", trace, L.lib().stif_rank_sum, _vp(slab), row, R, _vp(dst), n,
            torch.cuda.current_stream(slab.device).cuda_stream)
    return dst


def _sorted_segments(words: torch.Tensor, D: int):
    """The packed words of a scatter in ascending order and the D + 1 segment starts: integer torch calls on the
    device whose results are unique (the words are distinct), so nothing here depends on an order of arrival."""
    srt = torch.sort(words).values
    bounds = torch.arange(D + 1, dtype=torch.int64, device=words.device) << 32
    return srt, torch.searchsorted(srt, bounds)


def dec_x3_bwd(g: DecTrainGeom, hrfeat: torch.Tensor, flow: torch.Tensor, g_x3: torch.Tensor,
               g_flow: Optional[torch.Tensor] = None, deterministic: bool = False):
    """The adjoint of dec_x3_fwd (stif_dec_x3_bwd): (g_flow [N, 4], g_hrfeat [N, 64], g_feat [B, H, W, 192]).  g_flow
    is written with plain stores and is exactly zero where a grid is clamped; g_hrfeat and g_feat are zeroed here and
    scattered into with fp32 atomics -- the only order-dependent sums of the decoder backward.  ``deterministic``:
    the same g_flow bytes from stif_dec_x3_bwd_contrib, which stores every corner's weight and packed sort word in
    place of the scatters; the words are sorted and stif_segsum adds g_hrfeat and g_feat per destination in a fixed
    order (identical bits on every call)."""
    hrfeat = g._mat("dec_x3_bwd: hrfeat", hrfeat, 64)
    flow = g._mat("dec_x3_bwd: flow", flow, 4)
    g_x3 = g._mat("dec_x3_bwd: g_x3", g_x3, 528)
    g_flow = g._mat("dec_x3_bwd: g_flow", g_flow, 4)
    if deterministic:
        dev, E = g.feat.device, 8 * g.N
        w_hr, w_lr = torch.empty(2, E, dtype=torch.float32, device=dev)
        words_hr, words_lr = torch.empty(2, E, dtype=torch.int64, device=dev)
        trace = (("dec_x3_bwd_contrib",), 0.0, 4.0 * g.N * (528 + 4 * 262 + 8 * 6)) if TRACE is not None else None
        g._run("stif_dec_x3_bwd_contrib", trace, _vp(hrfeat), _vp(flow), _vp(g_x3), _vp(g_flow), _vp(w_hr),
               _vp(words_hr), _vp(w_lr), _vp(words_lr))
        g_hrfeat = g._mat("dec_x3_bwd: g_hrfeat", None, 64)
        g_feat = torch.empty_like(g.feat)
        segsum(g_hrfeat, g_x3, 528, 2, 0, w_hr, *_sorted_segments(words_hr, g.N))
        segsum(g_feat.view(-1, 192), g_x3, 528, 2, 128, w_lr, *_sorted_segments(words_lr, g.B * g.H * g.W))
        return g_flow, g_hrfeat, g_feat
    g_hrfeat = g._mat("dec_x3_bwd: g_hrfeat", None, 64, torch.zeros)
    g_feat = torch.zeros_like(g.feat)
    trace = (("dec_x3_bwd",), 0.0, 4.0 * g.N * (528 + 3 * 4 * 262)) if TRACE is not None else None
    g._run("stif_dec_x3_bwd", trace, _vp(hrfeat), _vp(flow), _vp(g_x3), _vp(g_flow), _vp(g_hrfeat), _vp(g_feat))
    return g_flow, g_hrfeat, g_feat


def conv_first(x_nchw: torch.Tensor, w: torch.Tensor, b: torch.Tensor, out: torch.Tensor):
    n, c, h, wd = x_nchw.shape
    assert c == 3 and x_nchw.is_contiguous() and out.is_contiguous()
    L.check(L.lib().stif_conv_first(_vp(x_nchw), _vp(w), _vp(b), _vp(out), n, h, wd, _stream()), "stif_conv_first")


def dcn(groups, *, epi=L.EPI_NONE, status=None):
    """Fused DCN_sep core. groups: list of {layer: PackedConv (64->64 3x3), inp, offmask, out}."""
    parts = _split_by_mode(groups, "layer")
    if parts:
        for part in parts:
            dcn(part, epi=epi, status=status)
        return
    if not 1 <= len(groups) <= L.MAXG:
        raise ValueError(f"dcn: 1..{L.MAXG} groups")
    g0 = groups[0]
    _, H, W, Cc = g0["inp"].shape
    assert Cc == 64
    a = L.DcnArgs()
    for i, g in enumerate(groups):
        if not g["inp"].shape[0] == g["offmask"].shape[0] == g["out"].shape[0]:
            raise ValueError("dcn: inp / offmask / out of a group must hold the same number of items")
        a.inp[i] = _vp(g["inp"])
        a.offmask[i] = _vp(g["offmask"])
        a.w[i] = _vp(g["layer"].w)
        a.bias[i] = _vp(g["layer"].b)
        a.out[i] = _vp(g["out"])
    a.in_item = _item_stride([g["inp"] for g in groups], "dcn in")
    a.om_item = _item_stride([g["offmask"] for g in groups], "dcn offmask")
    a.out_item = _item_stride([g["out"] for g in groups], "dcn out")
    total = _set_items(a, [g["inp"].shape[0] for g in groups])
    a.H, a.W, a.epi = H, W, epi
    f16 = g0["layer"].mode & L.PACK_F16X3
    a.flags = L.CONV_F16X3 if f16 else 0
    a.status = _vp(status)
    trace = None
    if TRACE is not None:
        trace = (("dcn", epi), 2.0 * 64 * 576 * H * W * total, 4.0 * (64 + 216 + 64) * H * W * total)
    _launch("stif_dcn_nhwc", trace, L.lib().stif_dcn_nhwc, C.byref(a), _stream())


def dcn_offmask(om: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The offset / mask conv's NHWC map ``om`` [n, H, W, 256] (reference row order: offsets 0..143, mask logits
    144..215, pad channels never read) as the offmask ops.dcn reads, [n, H, W, 216] = [group][tap][dy, dx,
    sigmoid(logit)] (stif_dcn_offmask_nhwc): offsets bit for bit, one pass.  Items may be strided, pixels contiguous."""
    if om.dim() != 4 or om.shape[3] != 256 or 0 in om.shape:
        raise ValueError(f"dcn_offmask: om {tuple(om.shape)} must be [n, H, W, 256]")
    n, H, W, _ = om.shape
    if out is None:
        out = torch.empty(n, H, W, 216, dtype=torch.float32, device=om.device)
    elif tuple(out.shape) != (n, H, W, 216):
        raise ValueError(f"dcn_offmask: out shape {tuple(out.shape)} != {(n, H, W, 216)}")
    om_item = _item_stride([om], "dcn_offmask om")
    out_item = _item_stride([out], "dcn_offmask out")
    trace = (("dcn_offmask",), 0.0, 4.0 * 2 * 216 * n * H * W) if TRACE is not None else None
    _launch("stif_dcn_offmask_nhwc", trace, L.lib().stif_dcn_offmask_nhwc, _vp(om), _vp(out),
            om_item if n > 1 else H * W * 256, out_item if n > 1 else H * W * 216, n, H, W,
            torch.cuda.current_stream(om.device).cuda_stream)
    return out


# The ordered g_in path works on as many items of a call at a time as keep its transient buffers under this many bytes
# (and E = items * H * W * 288 below 2^31); one item is the least.  Per pixel: the contribution slab 576 floats, 288
# corner weights (float32), 288 packed words (int64), torch.sort's sorted words and indices (2 x 288 int64) and as much
# again allowed for the radix sort's own double buffer, and the 8 + 8 int64 of the segment bounds and starts.
DET_TRANSIENT_BYTES = 1 << 30
_DET_BYTES_PER_PIXEL = 576 * 4 + 288 * 4 + 288 * 8 * (1 + 2 + 2) + 2 * 8 * 8


def _dcn_bwd_ordered(inp, offmask, weight, gout, out, epi, need_om):
    """(g_in, g_om or None) of dcn_bwd without atomics: stif_dcn_bwd_contrib, a sort of its packed words, the segment
    starts and stif_segsum, over chunks of items (items are independent, so the chunking cannot change a bit)."""
    n, H, W, _ = inp.shape
    dev, px = inp.device, H * W
    per_chunk = max(1, min(DET_TRANSIENT_BYTES // (_DET_BYTES_PER_PIXEL * px), (2 ** 31 - 1) // (288 * px), n))
    g_in = torch.empty(n, H, W, 64, dtype=torch.float32, device=dev)
    g_om = torch.empty(n, H, W, 256, dtype=torch.float32, device=dev) if need_om else None
    cm = torch.empty(per_chunk * px, 576, dtype=torch.float32, device=dev)
    wgt = torch.empty(per_chunk * px * 288, dtype=torch.float32, device=dev)
    words = torch.empty(per_chunk * px * 288, dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    for i0 in range(0, n, per_chunk):
        m = min(per_chunk, n - i0)
        a = L.DcnBwdContribArgs()
        def item(t, what):
            stride = _item_stride([t], "dcn_bwd " + what)
            return _vp(t[i0:]), (stride if m > 1 else px * t.shape[3])

        a.inp, a.in_item = item(inp, "inp")
        a.offmask, a.om_item = item(offmask, "offmask")
        a.gout, a.gout_item = item(gout, "gout")
        a.w = _vp(weight)
        if epi == L.EPI_LRELU:
            a.out, a.out_item = item(out, "out")
        if need_om:
            a.g_om, a.gom_item = _vp(g_om[i0:]), px * 256
        E, D = m * px * 288, m * px * 8
        a.cm, a.wgt, a.words = _vp(cm), _vp(wgt), _vp(words)
        a.n, a.H, a.W, a.epi = m, H, W, epi
        trace = None
        if TRACE is not None:
            trace = (("dcn_bwd_contrib", epi, need_om), 2.0 * 64 * 576 * m * px,
                     4.0 * (64 * 2 + 216 + 256 * need_om + 576 + 288 * 3) * m * px)
        _launch("stif_dcn_bwd_contrib", trace, L.lib().stif_dcn_bwd_contrib, C.byref(a), stream)
        srt, seg = _sorted_segments(words[:E], D)
        segsum(g_in[i0:i0 + m].view(D, 8), cm, 576, 72, 0, wgt[:E], srt, seg)
    return g_in, g_om


def dcn_bwd(inp: torch.Tensor, offmask: torch.Tensor, weight: torch.Tensor, gout: torch.Tensor, *,
            out: Optional[torch.Tensor] = None, epi=L.EPI_NONE, need=(True, True, True), deterministic: bool = False):
    """Backward of ops.dcn (fp32, one group) on NHWC maps (stif_dcn_bwd_nhwc): ``inp`` / ``gout`` [n, H, W, 64],
    ``offmask`` [n, H, W, 216] as the forward read it, ``weight`` the state dict's [64, 64, 3, 3] on the device,
    ``out`` the forward's output (needed with ``epi`` = EPI_LRELU only: the activation's derivative).  ``need`` =
    (g_in, g_om, g_w): what to compute.  Returns (g_in [n, H, W, 64], g_om [n, H, W, 256], g_w [64, 64, 3, 3],
    g_b [64]) with None for what was not asked for (g_b comes with g_w).  g_om is the gradient of the offset / mask
    conv's 256-channel output: grad_offset in channels 0..143, grad_mask * m (1 - m) in 144..215, zeros in the pad
    channels.  g_om, g_w and g_b have identical bits on repeated calls; g_in is an fp32 atomic sum.  ``deterministic``:
    g_in is the ordered sum instead (stif_dcn_bwd_contrib, a sort, stif_segsum; DET_TRANSIENT_BYTES bounds its
    transient buffers), with identical bits on repeated calls; g_om, g_w and g_b keep their bytes."""
    need_in, need_om, need_w = (bool(v) for v in need)
    if inp.dim() != 4 or inp.shape[3] != 64 or 0 in inp.shape or gout.shape != inp.shape:
        raise ValueError(f"dcn_bwd: inp {tuple(inp.shape)} and gout {tuple(gout.shape)} must both be [n, H, W, 64]")
    n, H, W, _ = inp.shape
    if tuple(offmask.shape) != (n, H, W, 216):
        raise ValueError(f"dcn_bwd: offmask shape {tuple(offmask.shape)} != {(n, H, W, 216)}")
    if tuple(weight.shape) != (64, 64, 3, 3) or not (weight.is_cuda and weight.dtype == torch.float32):
        raise ValueError("dcn_bwd: expected a float32 CUDA weight [64, 64, 3, 3]")
    if epi not in (L.EPI_NONE, L.EPI_LRELU):
        raise ValueError("dcn_bwd: epi must be EPI_NONE or EPI_LRELU")
    if epi == L.EPI_LRELU and (out is None or out.shape != inp.shape):
        raise ValueError("dcn_bwd: EPI_LRELU needs the forward's output [n, H, W, 64]")
    if not (need_in or need_om or need_w):
        raise ValueError("dcn_bwd: nothing to compute")
    weight = weight.detach().contiguous()
    dev = inp.device
    if deterministic and need_in:
        g_in, g_om = _dcn_bwd_ordered(inp, offmask, weight, gout, out, epi, need_om)
        g_w = g_b = None
        if need_w:   # the weight kernel alone: already a fixed-order sum
            _, _, g_w, g_b = dcn_bwd(inp, offmask, weight, gout, out=out, epi=epi, need=(False, False, True))
        return g_in, g_om, g_w, g_b
    a = L.DcnBwdArgs()
    def item(t, what):   # checks dtype, device and pixel contiguity; the stride of a size-1 dim addresses nothing
        stride = _item_stride([t], "dcn_bwd " + what)
        return stride if n > 1 else H * W * t.shape[3]

    a.inp, a.in_item = _vp(inp), item(inp, "inp")
    a.offmask, a.om_item = _vp(offmask), item(offmask, "offmask")
    a.gout, a.gout_item = _vp(gout), item(gout, "gout")
    a.w = _vp(weight)
    if epi == L.EPI_LRELU:
        a.out, a.out_item = _vp(out), item(out, "out")
    g_in = g_om = g_w = g_b = None
    if need_in:
        g_in = torch.empty(n, H, W, 64, dtype=torch.float32, device=dev)
        a.g_in, a.gin_item = _vp(g_in), H * W * 64
    if need_om:
        g_om = torch.empty(n, H, W, 256, dtype=torch.float32, device=dev)
        a.g_om, a.gom_item = _vp(g_om), H * W * 256
    stream = torch.cuda.current_stream(dev).cuda_stream
    if need_w:
        g_w = torch.empty(64, 64, 3, 3, dtype=torch.float32, device=dev)
        g_b = torch.empty(64, dtype=torch.float32, device=dev)
        ws, stream = _wgrad_workspace(dev, L.lib().stif_dcn_bwd_workspace_size(n, H, W))
        a.g_w, a.g_b, a.workspace, a.workspace_bytes = _vp(g_w), _vp(g_b), _vp(ws), ws.numel() * 4
    a.n, a.H, a.W, a.epi = n, H, W, epi
    trace = None
    if TRACE is not None:   # the column-gradient GEMM (data kernel) and the weight-gradient GEMM
        flops = 2.0 * 64 * 576 * n * H * W * ((need_in or need_om) + need_w)
        trace = (("dcn_bwd", epi, need_in, need_om, need_w), flops, 4.0 * (64 * 3 + 216 + 256) * n * H * W)
    _launch("stif_dcn_bwd_nhwc", trace, L.lib().stif_dcn_bwd_nhwc, C.byref(a), stream)
    return g_in, g_om, g_w, g_b


def dcn_sep_fusable(om_layer: PackedConv, layer: PackedConv) -> bool:
    """Both layers of a DCN_sep packed for the fused kernel (stif_dcn_sep_nhwc)."""
    return om_layer.mode == (L.PACK_DCNSEP | L.PACK_F16X3) and layer.mode == (L.PACK_DCNPAIR | L.PACK_F16X3)


def dcn_sep(groups, *, epi=L.EPI_NONE, status=None):
    """Fused DCN_sep (dcn_v2.py:127-140): offset/mask conv + sigmoid + deformable conv in one launch.
    groups: list of {om_layer: PackedConv (STIF_PACK_DCNSEP | F16X3), layer: PackedConv (64->64 3x3,
    STIF_PACK_DCNPAIR | F16X3), fea, inp, out} with NHWC [nitems, H, W, 64] tensors."""
    if not 1 <= len(groups) <= L.MAXG:
        raise ValueError(f"dcn_sep: 1..{L.MAXG} groups")
    g0 = groups[0]
    _, H, W, Cc = g0["inp"].shape
    a = L.DcnSepArgs()
    for i, g in enumerate(groups):
        if not dcn_sep_fusable(g["om_layer"], g["layer"]):
            raise ValueError("dcn_sep: layers not packed for the fused kernel")
        nitems = g["inp"].shape[0]   # each group may carry its own number of items
        for k in ("fea", "inp", "out"):
            if tuple(g[k].shape) != (nitems, H, W, 64):
                raise ValueError(f"dcn_sep: {k} shape {tuple(g[k].shape)} != {(nitems, H, W, 64)}")
        a.fea[i] = _vp(g["fea"])
        a.inp[i] = _vp(g["inp"])
        a.w_om[i] = _vp(g["om_layer"].w)
        a.b_om[i] = _vp(g["om_layer"].b)
        a.w[i] = _vp(g["layer"].w)
        a.bias[i] = _vp(g["layer"].b)
        a.out[i] = _vp(g["out"])
    a.fea_item = _item_stride([g["fea"] for g in groups], "dcn_sep fea")
    a.in_item = _item_stride([g["inp"] for g in groups], "dcn_sep in")
    a.out_item = _item_stride([g["out"] for g in groups], "dcn_sep out")
    total = _set_items(a, [g["inp"].shape[0] for g in groups])
    a.H, a.W, a.epi = H, W, epi
    a.flags = L.CONV_F16X3
    a.status = _vp(status)
    trace = None
    if TRACE is not None:
        px = H * W * total
        # algorithmic: the offset/mask conv (216 x 576 MACs) + the deformable conv (64 x 576) per pixel;
        # HBM bytes: the offset feature, the DCN input and the output read / written once (768 B / px)
        trace = (("dcnsep", epi), 2.0 * (216 + 64) * 576 * px, 4.0 * 3 * 64 * px)
    _launch("stif_dcn_sep_nhwc", trace, L.lib().stif_dcn_sep_nhwc, C.byref(a), _stream())


def _dcn_v2_args(name, tensors, kernel_h, kernel_w, *geom):
    """The checks both drop-in entry points share (tensors = input, weight, ...): the tensors made contiguous
    and the 14 shape arguments of the C ABI.  geom: stride, pad, dilation (h, w each) and deformable_group."""
    for t in tensors:
        if not (t.is_cuda and t.dtype == torch.float32):
            raise RuntimeError(f"{name}: tensors must be float32 on the GPU")
    tensors = tuple(t.contiguous() for t in tensors)
    b, c, h, w = tensors[0].shape
    co, ci, kh, kw = tensors[1].shape
    if (kh, kw) != (kernel_h, kernel_w):
        raise RuntimeError(f"Input shape and kernel shape wont match: ({kernel_h} x {kernel_w} vs {kh} x {kw}).")
    if ci != c:
        raise RuntimeError(f"Input shape and kernel channels wont match: ({c} vs {ci}).")
    return tensors, (b, c, h, w, co, kernel_h, kernel_w, *geom)


def _dcn_v2_workspace(size_fn, dims, device):
    nbytes = size_fn(*dims)
    return torch.empty(max(nbytes // 4, 1), device=device, dtype=torch.float32), nbytes


def dcn_v2_forward(input, weight, bias, offset, mask, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w,
                   dilation_h, dilation_w, deformable_group):
    """Drop-in for ``_ext.dcn_v2_forward`` (DCNv2/src/dcn_v2.h:9-23): NCHW in, new NCHW tensor out."""
    ts, dims = _dcn_v2_args("dcn_v2_forward", (input, weight, bias, offset, mask), kernel_h, kernel_w, stride_h,
                            stride_w, pad_h, pad_w, dilation_h, dilation_w, deformable_group)
    b, _, h, w, co = dims[:5]
    ho = (h + 2 * pad_h - (dilation_h * (kernel_h - 1) + 1)) // stride_h + 1
    wo = (w + 2 * pad_w - (dilation_w * (kernel_w - 1) + 1)) // stride_w + 1
    out = torch.empty(b, co, ho, wo, device=input.device, dtype=torch.float32)
    ws, nbytes = _dcn_v2_workspace(L.lib().stif_dcn_v2_workspace_size, dims, out.device)
    trace = (("dcn_v2_fwd",), 2.0 * co * dims[1] * kernel_h * kernel_w * b * ho * wo) if TRACE is not None else None
    _launch("dcn_v2_forward", trace, L.lib().stif_dcn_v2_forward, *[_vp(t) for t in ts], _vp(out), *dims, _vp(ws),
            nbytes, _stream())
    return out


def dcn_v2_backward(input, weight, bias, offset, mask, grad_output, kernel_h, kernel_w, stride_h, stride_w, pad_h,
                    pad_w, dilation_h, dilation_w, deformable_group):
    """Drop-in for ``_ext.dcn_v2_backward`` (DCNv2/src/dcn_v2.h:39-52): returns new tensors
    (grad_input, grad_offset, grad_mask, grad_weight, grad_bias) in that order, as
    ``_DCNv2.backward`` (DCNv2/dcn_v2.py:31-45) unpacks them."""
    ts, dims = _dcn_v2_args("dcn_v2_backward", (input, weight, bias, offset, mask, grad_output), kernel_h, kernel_w,
                            stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w, deformable_group)
    input, weight, bias, offset, mask, _ = ts
    grads = [torch.empty_like(t) for t in (input, offset, mask, weight, bias)]
    ws, nbytes = _dcn_v2_workspace(L.lib().stif_dcn_v2_backward_workspace_size, dims, input.device)
    trace = None
    if TRACE is not None:   # the column GEMM and the weight-gradient GEMM
        gb, _, gh, gw_ = grad_output.shape
        trace = (("dcn_v2_bwd",), 4.0 * weight.numel() * gb * gh * gw_)
    _launch("dcn_v2_backward", trace, L.lib().stif_dcn_v2_backward, *[_vp(t) for t in ts], *[_vp(g) for g in grads],
            *dims, _vp(ws), nbytes, _stream())
    return tuple(grads)


class DecTablesDev:
    """Device copies of coords.dec_tables(h, w, HH, WW[, shift]) + the C struct pointing at them.
    With a shift (local ensemble) the HR remap tables are set too; ``plain`` is then the same tables without the
    remap (hr_y = hr_x = NULL), as the windowed feat-only pass of a shifted query takes them."""

    def __init__(self, h, w, HH, WW, device="cuda", shift=None):
        tab = dec_tables(h, w, HH, WW, shift)
        keys = TABLE_ORDER + (["hr_y", "hr_x"] if shift is not None else [])
        self._t = {k: torch.from_numpy(np.ascontiguousarray(tab[k])).to(device) for k in keys}
        self.c = L.DecTables(*[self._t[k].data_ptr() for k in keys])
        self.shape = (h, w, HH, WW)
        self.plain = self
        if shift is not None:
            self.plain = object.__new__(DecTablesDev)
            self.plain._t, self.plain.shape, self.plain.plain = self._t, self.shape, self.plain
            self.plain.c = L.DecTables(*[self._t[k].data_ptr() for k in TABLE_ORDER])
            # the remap rectangle of a window is known on the host: the tables are monotone
            self.hr_y, self.hr_x = tab["hr_y"], tab["hr_x"]

    @property
    def shifted(self):
        """These tables carry the remap (hr_y / hr_x) of a shifted query; ``plain`` never does."""
        return "hr_y" in self._t and bool(self.c.hr_y)

    def remap_rect(self, rect):
        """The rectangle (y0, x0, hh, ww) of HR pixels whose HRfeat the flow stage of a shifted query reads for the
        window ``rect``: [hr_y[y0], hr_y[y0 + hh - 1]] x [hr_x[x0], hr_x[x0 + ww - 1]]."""
        return remap_rect(self.hr_y, self.hr_x, rect)


def remap_rect(hr_y, hr_x, rect):
    """``DecTablesDev.remap_rect`` from the (monotone) host tables hr_y / hr_x of coords.dec_tables(shift=)."""
    y0, x0, hh, ww = rect
    ry0, ry1, rx0, rx1 = int(hr_y[y0]), int(hr_y[y0 + hh - 1]), int(hr_x[x0]), int(hr_x[x0 + ww - 1])
    return ry0, rx0, ry1 - ry0 + 1, rx1 - rx0 + 1


ENSEMBLE_SHIFTS = [(vx, vy) for vx in (-1, 1) for vy in (-1, 1)]   # the reference's order (:1006-1007)
# The order the four decodes are blended in place: stif_dec_blend4, as built, rounds decode 1's product and fuses
# the other three (stif.h stif_dec_stage2_blend_win), so this order gives decoding_localensemble's bits
ENSEMBLE_BLEND_ORDER = (1, 0, 2, 3)


def dec_blend(k, tables4, accumulate=True) -> L.DecBlend:
    """The stif_dec_blend of decode ``k`` given the four shifted DecTablesDev in ENSEMBLE_SHIFTS order;
    accumulate=False for the first decode blended into an output (it stores, the others add)."""
    if len(tables4) != 4:
        raise ValueError("dec_blend: the tables of the four shifted queries")
    b = L.DecBlend()
    b.k, b.accumulate = int(k), int(bool(accumulate))
    for j, tb in enumerate(tables4):
        b.rel_y[j], b.rel_x[j] = tb._t["rel_y"].data_ptr(), tb._t["rel_x"].data_ptr()
    return b


class DecImageDev:
    """decoding_test's HRinp: the x`s` bilinear upsample of the frame pair ([n, s*h, s*w, 8] NHWC on
    the device, stif_upsample_image) and its bilinear tables at the HR query grid (HH, WW).  shift: the local
    ensemble's (vx, vy), as DecTablesDev's -- the image is sampled at the same shifted query as the latent."""

    def __init__(self, x_nchw, s, HH, WW, shift=None):
        n, _, _, h, w = x_nchw.shape
        self.img = torch.empty(n, s * h, s * w, 8, device=x_nchw.device, dtype=torch.float32)
        L.check(L.lib().stif_upsample_image(_vp(x_nchw), _vp(self.img), n, h, w, s, _stream()), "stif_upsample_image")
        t = dec_tables(s * h, s * w, HH, WW, shift, (h, w))
        keys = ["b0_y", "b1_y", "w0_y", "w1_y", "b0_x", "b1_x", "w0_x", "w1_x"]
        self._t = {k: torch.from_numpy(np.ascontiguousarray(t[k])).to(x_nchw.device) for k in keys}
        self._keys = keys
        self.c = L.DecImage(self.img.data_ptr(), s * h, s * w, *[self._t[k].data_ptr() for k in keys])

    def items(self, a, b):
        """The same image and tables for items [a, b) only (decoder passes over an item range)."""
        o = object.__new__(DecImageDev)
        o.img, o._t, o._keys = self.img[a:b], self._t, self._keys
        o.c = L.DecImage(o.img.data_ptr(), self.c.ih, self.c.iw, *[o._t[k].data_ptr() for k in o._keys])
        return o


def dec_blend4(preds, weights, out):
    """out = sum_k preds[k] * weights[k] (per HR pixel), the local ensemble's area blend."""
    n, _, HH, WW = out.shape
    pp = (C.c_void_p * 4)(*[_vp(p) for p in preds])
    ww = (C.c_void_p * 4)(*[_vp(w_) for w_ in weights])
    L.check(L.lib().stif_dec_blend4(pp, ww, _vp(out), n, HH, WW, _stream()), "stif_dec_blend4")


def dec_pack_lr(f0, f1, f2, x, out):
    n, h, w, _ = f0.shape
    L.check(L.lib().stif_dec_pack_lr(_vp(f0), _vp(f1), _vp(f2), _vp(x), _vp(out), n, h, w, _stream()),
            "stif_dec_pack_lr")


def dec_window(rect, HH, WW, frect=None) -> L.DecWindow:
    """A stif_dec_window for the query rectangle ``rect = (y0, x0, hh, ww)`` of the virtual HH x WW grid
    (ValueError if it is not inside), HRfeat held over ``frect`` (None: the query rectangle itself)."""
    y0, x0, hh, ww = check_window(rect, HH, WW)
    win = L.DecWindow(y0, x0, hh, ww)
    if frect is not None:
        win.fy0, win.fx0, win.fh, win.fw = check_window(frect, HH, WW)
    return win


def _win_shapes(window, tables, n, hrfeat, flow):
    """(HH, WW) of a windowed stage call after checking the buffers against the window's rectangles."""
    HH, WW = tables.shape[2:]
    check_window((window.y0, window.x0, window.hh, window.ww), HH, WW)
    fh, fw = (window.fh, window.fw) if (window.fh or window.fw) else (window.hh, window.ww)
    if tuple(hrfeat.shape) != (n, fh, fw, 64) or not hrfeat.is_contiguous():
        raise ValueError(f"windowed decoder stage: hrfeat must be a contiguous {(n, fh, fw, 64)}, got {tuple(hrfeat.shape)}")
    if flow is not None and (tuple(flow.shape) != (n, window.hh, window.ww, 4) or not flow.is_contiguous()):
        raise ValueError(f"windowed decoder stage: flow must be a contiguous {(n, window.hh, window.ww, 4)}, "
                         f"got {tuple(flow.shape)}")
    return HH, WW


class DecTime:
    """A time field for dec_stage1 / dec_stage2 in place of the [n] time tensor: the query time of pixel (gy, gx) of
    the virtual HH x WW grid of item i is ``t`` at element offset i * item + gy * row + gx * col from its first
    element (stif_dec_time; strides >= 0, 0 broadcasts).  ``n``: the items the field holds (None with item = 0: any
    number).  ``DecTime.of(v)`` takes a [b, hh, ww] fp32 device tensor or view, each dim 1 or the full size -- a dim
    of size 1 and an expanded dim broadcast.  ``f[a:b]`` is the field of items [a, b), as ``t[a:b]`` of a vector."""

    def __init__(self, t: torch.Tensor, item: int, row: int, col: int, n=None, offset: int = 0, grid=None):
        if t.dtype != torch.float32 or not t.is_cuda:
            raise ValueError("DecTime: expected a float32 CUDA tensor")
        if min(item, row, col) < 0:
            raise ValueError("DecTime: strides must be >= 0")
        self.t, self.item, self.row, self.col, self.n, self.offset = t, int(item), int(row), int(col), n, int(offset)
        self.grid = grid   # (hh, ww) the field spans, each 1 or the grid's size; checked against the tables' grid
        self.c = L.DecTimeField(t.data_ptr() + 4 * self.offset, self.item, self.row, self.col)

    @classmethod
    def of(cls, v: torch.Tensor):
        if v.dim() != 3:
            raise ValueError(f"DecTime.of: a [b, hh, ww] tensor, got {tuple(v.shape)}")
        st = [0 if v.shape[d] == 1 else v.stride(d) for d in range(3)]
        return cls(v, *st, n=None if st[0] == 0 else v.shape[0], grid=tuple(v.shape[1:]))

    @property
    def shape(self):
        return (self.n,)

    def __getitem__(self, s):
        if not isinstance(s, slice) or s.step not in (None, 1):
            raise TypeError("DecTime: only item slices [a:b]")
        if self.n is None:
            return self
        a, b, _ = s.indices(self.n)
        return DecTime(self.t, self.item, self.row, self.col, max(0, b - a), self.offset + a * self.item, self.grid)


def _time_field_call(t, n, image, tables, what):
    if image is not None or tables.shifted:
        raise ValueError(f"{what}: a time field has no high-resolution-image and no local-ensemble form")
    if t.n is not None and t.n != n:
        raise ValueError(f"{what}: the time field holds {t.n} items, the call has {n}")
    HH, WW = tables.shape[2:]
    if t.grid is not None and (t.grid[0] not in (1, HH) or t.grid[1] not in (1, WW)):
        raise ValueError(f"{what}: a time field over {t.grid} does not broadcast to the {HH} x {WW} grid")


def _stage_entry(stage, t, window, blend=None):
    """(entry name for errors, library function, time argument, trailing arguments) of decoder stage ``stage`` for
    the time ``t`` (an [n] tensor or a DecTime), a window and a blend (either may be None)."""
    win = C.byref(window) if window is not None else None
    if isinstance(t, DecTime):
        what, targ, tail = f"stif_dec_stage{stage}_tf", C.byref(t.c), (win,)
    elif blend is not None:
        what, targ, tail = "stif_dec_stage2_blend_win", _vp(t), (C.byref(blend), win)
    elif window is not None:
        what, targ, tail = f"stif_dec_stage{stage}_win", _vp(t), (win,)
    else:
        return f"stif_dec_stage{stage}", getattr(L.lib(), f"stif_dec_stage{stage}_ex"), _vp(t), ()
    return what, getattr(L.lib(), what), targ, tail


def dec_stage1(proj, mlp, tables: DecTablesDev, t, hrfeat, flow, image: "DecImageDev" = None, flags=0, status=None,
               window: L.DecWindow = None):
    """window (dec_window): the stage over that rectangle of the tables' grid -- flow [n, hh, ww, 4] (None: HRfeat
    only), hrfeat over the window's F rectangle.  t: the [n] time tensor, or a DecTime (a time per pixel of the
    tables' grid; no image, no shifted tables)."""
    n, h, w, _ = proj.shape
    if isinstance(t, DecTime):
        _time_field_call(t, n, image, tables, "dec_stage1")
    HH, WW = _win_shapes(window, tables, n, hrfeat, flow) if window is not None else hrfeat.shape[1:3]
    trace = None
    if window is None and TRACE is not None:
        # per HR px: feat_imnet layers 1-3 (36,864 MAC) + flow_imnet HRfeat/1-3 (25,600 MAC)
        trace = (("dec1",), 2.0 * 62464 * n * HH * WW)
    what, fn, targ, tail = _stage_entry(1, t, window)
    _launch(what, trace, fn, _vp(proj), _vp(mlp), C.byref(tables.c), C.byref(image.c) if image else None, targ,
            _vp(hrfeat), _vp(flow), n, h, w, HH, WW, flags, _vp(status), _stream(), *tail)


def dec_flow_win(proj, mlp, tables: DecTablesDev, t, hrfeat, flow, flags=0, status=None, window: L.DecWindow = None):
    """The windowed flow-only stage of a shifted query (``tables`` with the remap): flow [n, hh, ww, 4] over the
    window, its HRfeat operand read at (hr_y, hr_x) from ``hrfeat`` over the window's F rectangle, which has to hold
    the window's remap rectangle (``tables.remap_rect``); bit 2 of ``status`` reports an F that does not."""
    n, h, w, _ = proj.shape
    if window is None:
        raise ValueError("dec_flow_win: a window (dec_window) is required")
    HH, WW = _win_shapes(window, tables, n, hrfeat, flow)
    if flow is None:
        raise ValueError("dec_flow_win: flow is the output")
    _launch("stif_dec_flow_win", None, L.lib().stif_dec_flow_win, _vp(proj), _vp(mlp), C.byref(tables.c), None, _vp(t),
            _vp(hrfeat), _vp(flow), n, h, w, HH, WW, flags, _vp(status), _stream(), C.byref(window))


def dec_bounds(flow, tables: DecTablesDev, box, window: L.DecWindow):
    """box (4 int32 on the device) = ymin, ymax, xmin, xmax of every HRfeat row / column stage 2 reads for the
    window, given stage 1's flow [n, hh, ww, 4] over it."""
    HH, WW = tables.shape[2:]
    check_window((window.y0, window.x0, window.hh, window.ww), HH, WW)
    n = flow.shape[0]
    if tuple(flow.shape) != (n, window.hh, window.ww, 4) or not flow.is_contiguous():
        raise ValueError(f"dec_bounds: flow must be a contiguous {(n, window.hh, window.ww, 4)}, got {tuple(flow.shape)}")
    if box.dtype != torch.int32 or box.numel() != 4 or not box.is_contiguous():
        raise ValueError("dec_bounds: box must be 4 contiguous int32")
    L.check(L.lib().stif_dec_bounds(_vp(flow), C.byref(tables.c), _vp(box), n, HH, WW, _stream(), C.byref(window)),
            "stif_dec_bounds")


def dec_stage2(proj, mlp, hrfeat, flow, tables: DecTablesDev, t, out, image: "DecImageDev" = None, flags=0,
               status=None, window: L.DecWindow = None, blend: L.DecBlend = None):
    """window (dec_window): the stage over that rectangle -- hrfeat over its F rectangle, flow [n, hh, ww, 4], and
    out any [n, 3, hh, ww] view with unit column stride (e.g. a tile of a larger [n, 3, HH, WW] tensor).
    blend (dec_blend; needs a window, no image): the local ensemble's epilogue -- w_k rgb is stored, or added to
    what ``out`` holds (blend.accumulate)."""
    n, h, w, _ = proj.shape
    trace = win = None
    if blend is not None and (window is None or image is not None):
        raise ValueError("dec_stage2: the blending epilogue is the windowed stage's, without a high-resolution image")
    if isinstance(t, DecTime):
        _time_field_call(t, n, image, tables, "dec_stage2")
        if blend is not None:
            raise ValueError("dec_stage2: a time field has no blending (local-ensemble) form")
    if window is not None:
        HH, WW = _win_shapes(window, tables, n, hrfeat, flow)
        if tuple(out.shape) != (n, 3, window.hh, window.ww) or (window.ww > 1 and out.stride(3) != 1):
            raise ValueError(f"dec_stage2: out must be {(n, 3, window.hh, window.ww)} with unit column stride")
        win = L.DecWindow.from_buffer_copy(window)
        win.out_item, win.out_plane, win.out_pitch = out.stride(0), out.stride(1), out.stride(2)
    else:
        HH, WW = hrfeat.shape[1:3]
        if TRACE is not None:   # per HR px: encode_imnet HRfeat part + layers 1-4 (94,976 MAC)
            trace = (("dec2",), 2.0 * 94976 * n * HH * WW)
    what, fn, targ, tail = _stage_entry(2, t, win, blend)
    _launch(what, trace, fn, _vp(proj), _vp(mlp), _vp(hrfeat), _vp(flow), C.byref(tables.c),
            C.byref(image.c) if image else None, targ, _vp(out), n, h, w, HH, WW, flags, _vp(status), _stream(), *tail)


class DecPoints:
    """A point list for dec_stage1_pts / dec_corners_pts / dec_stage2_pts (stif_dec_points): point p of item i is
    row ``y`` / column ``x`` (int32) of the tables' grid at element offset i * y_item + p (i * x_item + p) and time
    ``t`` (float32) at i * t_item + p * t_point from the tensors' first elements; strides >= 0, 0 broadcasts.
    ``n``: the items the list holds (None when no item stride is set: any number).  ``sub(a, b, p0, p1)`` is the list
    of points [p0, p1) of items [a, b)."""

    def __init__(self, y, x, t, y_item, x_item, t_item, t_point, npts, n=None, offsets=(0, 0, 0)):
        for v, dt, name in ((y, torch.int32, "y"), (x, torch.int32, "x"), (t, torch.float32, "t")):
            if v.dtype != dt or not v.is_cuda:
                raise ValueError(f"DecPoints: {name} must be a {dt} CUDA tensor")
        if min(y_item, x_item, t_item, t_point) < 0:
            raise ValueError("DecPoints: strides must be >= 0")
        if npts < 1:
            raise ValueError("DecPoints: at least one point per item")
        self.y, self.x, self.t, self.n, self.npts = y, x, t, n, int(npts)
        self.strides = (int(y_item), int(x_item), int(t_item), int(t_point))
        self.offsets = tuple(int(o) for o in offsets)
        oy, ox, ot = self.offsets
        self.c = L.DecPointList(y.data_ptr() + 4 * oy, x.data_ptr() + 4 * ox, t.data_ptr() + 4 * ot, *self.strides,
                                self.npts)

    def sub(self, a, b, p0, p1):
        yi, xi, ti, tp = self.strides
        oy, ox, ot = self.offsets
        return DecPoints(self.y, self.x, self.t, yi, xi, ti, tp, p1 - p0, None if self.n is None else b - a,
                         (oy + a * yi + p0, ox + a * xi + p0, ot + a * ti + p0 * tp))


def _points_call(pts, n, tables, what):
    if tables.shifted:
        raise ValueError(f"{what}: a point list has no local-ensemble form")
    if pts.n is not None and pts.n != n:
        raise ValueError(f"{what}: the point list holds {pts.n} items, the call has {n}")


def _dense(t, shape, dtype, what):
    if tuple(t.shape) != tuple(shape) or t.dtype != dtype or not t.is_cuda or not t.is_contiguous():
        raise ValueError(f"{what} must be a contiguous {dtype} CUDA tensor of shape {tuple(shape)}, got "
                         f"{t.dtype} {tuple(t.shape)}")


def dec_stage1_pts(proj, mlp, tables: DecTablesDev, pts: DecPoints, hrfeat, flow, flags=0, status=None):
    """Stage 1 over a point list: hrfeat [n, npts, 64] and flow [n, npts, 4] (None: HRfeat only) of every point at
    its own time.  A row / column outside the tables' grid is clamped into it and sets bit 3 of ``status``."""
    n, h, w, _ = proj.shape
    _points_call(pts, n, tables, "dec_stage1_pts")
    _dense(hrfeat, (n, pts.npts, 64), torch.float32, "dec_stage1_pts: hrfeat")
    if flow is not None:
        _dense(flow, (n, pts.npts, 4), torch.float32, "dec_stage1_pts: flow")
    HH, WW = tables.shape[2:]
    _launch("stif_dec_stage1_pts", None, L.lib().stif_dec_stage1_pts, _vp(proj), _vp(mlp), C.byref(tables.c),
            C.byref(pts.c), _vp(hrfeat), _vp(flow), n, h, w, HH, WW, flags, _vp(status), _stream())


def dec_corners_pts(flow, tables: DecTablesDev, pts: DecPoints, cy, cx, ct, status=None) -> DecPoints:
    """The eight HRfeat corner pixels stage 2 gathers for every point, from stage 1's flow [n, npts, 4], into cy, cx
    (int32) and ct (float32, the point's time), each [n, 8 * npts]; returns them as the point list of the feat-only
    pass (dec_stage1_pts with flow=None), whose hrfeat [n, 8 * npts, 64] is dec_stage2_pts' hrfeat8."""
    n = flow.shape[0]
    _points_call(pts, n, tables, "dec_corners_pts")
    _dense(flow, (n, pts.npts, 4), torch.float32, "dec_corners_pts: flow")
    m = 8 * pts.npts
    for v, dt, name in ((cy, torch.int32, "cy"), (cx, torch.int32, "cx"), (ct, torch.float32, "ct")):
        _dense(v, (n, m), dt, f"dec_corners_pts: {name}")
    HH, WW = tables.shape[2:]
    _launch("stif_dec_corners_pts", None, L.lib().stif_dec_corners_pts, _vp(flow), C.byref(tables.c), C.byref(pts.c),
            _vp(cy), _vp(cx), _vp(ct), n, HH, WW, _vp(status), _stream())
    return DecPoints(cy, cx, ct, m, m, m, 1, m, n)


def dec_stage2_pts(proj, mlp, hrfeat8, flow, tables: DecTablesDev, pts: DecPoints, out, flags=0, status=None):
    """Stage 2 over a point list: hrfeat8 [n, 8 * npts, 64] (the corner rows in dec_corners_pts' order), flow
    [n, npts, 4], out [n, 3, npts]."""
    n, h, w, _ = proj.shape
    _points_call(pts, n, tables, "dec_stage2_pts")
    _dense(hrfeat8, (n, 8 * pts.npts, 64), torch.float32, "dec_stage2_pts: hrfeat8")
    _dense(flow, (n, pts.npts, 4), torch.float32, "dec_stage2_pts: flow")
    _dense(out, (n, 3, pts.npts), torch.float32, "dec_stage2_pts: out")
    HH, WW = tables.shape[2:]
    _launch("stif_dec_stage2_pts", None, L.lib().stif_dec_stage2_pts, _vp(proj), _vp(mlp), _vp(hrfeat8), _vp(flow),
            C.byref(tables.c), C.byref(pts.c), _vp(out), n, h, w, HH, WW, flags, _vp(status), _stream())


def _shifted_points_call(pts, n, tables, what):
    if not tables.shifted:
        raise ValueError(f"{what}: the tables of a shifted query (local ensemble) are required")
    if pts.n is not None and pts.n != n:
        raise ValueError(f"{what}: the point list holds {pts.n} items, the call has {n}")


def dec_remap_pts(tables: DecTablesDev, pts: DecPoints, n, ry, rx, status=None) -> DecPoints:
    """The HR pixel whose HRfeat row the flow stage of the shifted query ``tables`` reads for every point of the ``n``
    items: ry = hr_y[y], rx = hr_x[x] (int32 [n, npts]) at the point's row / column, clamped into the grid (bit 3 of
    ``status``).  Returns them with the points' times as the point list of the feat-only pass (dec_stage1_pts with
    ``tables.plain`` and flow=None), whose hrfeat [n, npts, 64] is dec_flow_pts' operand."""
    _shifted_points_call(pts, n, tables, "dec_remap_pts")
    for v, name in ((ry, "ry"), (rx, "rx")):
        _dense(v, (n, pts.npts), torch.int32, f"dec_remap_pts: {name}")
    HH, WW = tables.shape[2:]
    _launch("stif_dec_remap_pts", None, L.lib().stif_dec_remap_pts, C.byref(tables.c), C.byref(pts.c), _vp(ry), _vp(rx),
            n, HH, WW, _vp(status), _stream())
    m = pts.npts
    return DecPoints(ry, rx, pts.t, m, m, pts.strides[2], pts.strides[3], m, n, (0, 0, pts.offsets[2]))


def dec_flow_pts(proj, mlp, tables: DecTablesDev, pts: DecPoints, hrfeat, flow, flags=0, status=None):
    """The flow-only stage of a shifted query (``tables`` with the remap) over a point list: flow [n, npts, 4], the
    HRfeat operand of point p of item i row [i, p] of ``hrfeat`` [n, npts, 64] (dec_remap_pts)."""
    n, h, w, _ = proj.shape
    _shifted_points_call(pts, n, tables, "dec_flow_pts")
    _dense(hrfeat, (n, pts.npts, 64), torch.float32, "dec_flow_pts: hrfeat")
    if flow is None:
        raise ValueError("dec_flow_pts: flow is the output")
    _dense(flow, (n, pts.npts, 4), torch.float32, "dec_flow_pts: flow")
    HH, WW = tables.shape[2:]
    _launch("stif_dec_flow_pts", None, L.lib().stif_dec_flow_pts, _vp(proj), _vp(mlp), C.byref(tables.c),
            C.byref(pts.c), _vp(hrfeat), _vp(flow), n, h, w, HH, WW, flags, _vp(status), _stream())


def dec_stage2_blend_pts(proj, mlp, hrfeat8, flow, tables: DecTablesDev, pts: DecPoints, out, blend: L.DecBlend,
                         flags=0, status=None):
    """dec_stage2_pts with the local ensemble's epilogue (dec_blend): w_k rgb is stored into out [n, 3, npts], or
    added to what it holds (blend.accumulate), the weight taken at the point's row / column.  ``tables``: those of
    the shifted query or their ``plain`` (the remap is not read)."""
    n, h, w, _ = proj.shape
    if pts.n is not None and pts.n != n:
        raise ValueError(f"dec_stage2_blend_pts: the point list holds {pts.n} items, the call has {n}")
    if not isinstance(blend, L.DecBlend):
        raise ValueError("dec_stage2_blend_pts: blend must be a dec_blend")
    _dense(hrfeat8, (n, 8 * pts.npts, 64), torch.float32, "dec_stage2_blend_pts: hrfeat8")
    _dense(flow, (n, pts.npts, 4), torch.float32, "dec_stage2_blend_pts: flow")
    _dense(out, (n, 3, pts.npts), torch.float32, "dec_stage2_blend_pts: out")
    HH, WW = tables.shape[2:]
    _launch("stif_dec_stage2_blend_pts", None, L.lib().stif_dec_stage2_blend_pts, _vp(proj), _vp(mlp), _vp(hrfeat8),
            _vp(flow), C.byref(tables.c), C.byref(pts.c), _vp(out), n, h, w, HH, WW, flags, _vp(status), _stream(),
            C.byref(blend))


# ----------------------------------------------------------------------------- video I/O (planar YUV <-> RGB)
_YUV_MATRIX = {"bt601": L.YUV_BT601, "bt709": L.YUV_BT709}


def _yuv_planes(frames, fmt):
    """(stif_yuv_format, y, u, v pointers of frame 0, n) for ``frames``: a uint8 device tensor [n, fmt.frame_bytes]
    (or [fmt.frame_bytes]) of dense Y4M frame payloads Y | U | V, or three uint8 plane tensors (y, u, v), each
    [n, rows, row bytes] with contiguous rows -- views of one buffer, so that they share the frame stride."""
    f = L.YuvFormat(fmt.width, fmt.height, fmt.sub_x, fmt.sub_y, fmt.depth, _YUV_MATRIX[fmt.matrix],
                    int(bool(fmt.full_range)))
    cw, ch = fmt.chroma_size
    bps = fmt.bytes_per_sample
    if isinstance(frames, (tuple, list)):
        y, u, v = frames
        n = y.shape[0]
        for t, rows, rb in ((y, fmt.height, fmt.width * bps), (u, ch, cw * bps), (v, ch, cw * bps)):
            if t.dtype != torch.uint8 or not t.is_cuda or tuple(t.shape) != (n, rows, rb) or (rb > 1 and t.stride(2) != 1):
                raise ValueError(f"yuv planes must be uint8 CUDA tensors [n, rows, row bytes]; expected {(n, rows, rb)}, "
                                 f"got {t.dtype} {tuple(t.shape)}")
        if u.stride(1) != v.stride(1) or (n > 1 and not y.stride(0) == u.stride(0) == v.stride(0)):
            raise ValueError("yuv planes must share the chroma pitch and the frame stride (views of one buffer)")
        f.pitch_y, f.pitch_c = y.stride(1), u.stride(1)
        f.frame_stride = y.stride(0) if n > 1 else 0
        return f, y.data_ptr(), u.data_ptr(), v.data_ptr(), n
    t = frames
    if t.dim() == 1:
        t = t[None]
    if t.dtype != torch.uint8 or not t.is_cuda or t.dim() != 2 or t.shape[1] != fmt.frame_bytes or not t.is_contiguous():
        raise ValueError(f"yuv frames must be a contiguous uint8 CUDA tensor [n, {fmt.frame_bytes}], got {t.dtype} "
                         f"{tuple(t.shape)}")
    ysz, csz = fmt.height * fmt.width * bps, ch * cw * bps
    p = t.data_ptr()
    return f, p, p + ysz, p + ysz + csz, t.shape[0]


def _rgb_strides(t, n, H, W, what):
    if t.dtype != torch.float32 or not t.is_cuda or t.dim() != 4 or t.shape[0] != n or t.shape[1] != 3:
        raise ValueError(f"{what} must be a float32 CUDA tensor [{n}, 3, H, W], got {t.dtype} {tuple(t.shape)}")
    if t.shape[3] > 1 and t.stride(3) != 1:
        raise ValueError(f"{what}: the last dimension must be contiguous")
    item = t.stride(0) if n > 1 else 2 * t.stride(1) + (H - 1) * t.stride(2) + W   # one item: never used
    return item, t.stride(1), t.stride(2)


def yuv_to_rgb(frames, fmt, out=None):
    """Planar YUV frames (see ``_yuv_planes``; ``fmt``: a y4m.YuvFormat) -> fp32 RGB in [0, 1] (stif_yuv_to_rgb).
    out: None for a new [n, 3, H, W], or any float32 [n, 3, >= H, >= W] with contiguous rows -- the frames are
    written into its top-left corner through its strides and the rest of it is left as it is, so a zero-filled
    tensor padded to a multiple of 4 is the model's input with no further copy."""
    f, y, u, v, n = _yuv_planes(frames, fmt)
    H, W = fmt.height, fmt.width
    if out is None:
        dev = (frames[0] if isinstance(frames, (tuple, list)) else frames).device
        out = torch.empty(n, 3, H, W, device=dev, dtype=torch.float32)
    elif out.dim() != 4 or out.shape[2] < H or out.shape[3] < W:
        raise ValueError(f"yuv_to_rgb: out must be [n, 3, >= {H}, >= {W}], got {tuple(out.shape)}")
    item, plane, pitch = _rgb_strides(out, n, H, W, "yuv_to_rgb: out")
    _launch("stif_yuv_to_rgb", None, L.lib().stif_yuv_to_rgb, C.byref(f), y, u, v, n, _vp(out), item, plane, pitch,
            _stream())
    return out


def rgb_to_yuv(rgb, fmt, out=None):
    """fp32 RGB frames [n, 3, H, W] (unclamped; any view with contiguous rows, e.g. the top-left crop of a padded
    decoder output) -> planar YUV frames of ``fmt`` (stif_rgb_to_yuv): a uint8 [n, fmt.frame_bytes] tensor of dense
    Y4M frame payloads (``out``, or a new one), or the three plane tensors passed as ``out`` (see ``_yuv_planes``)."""
    if rgb.dim() == 3:
        rgb = rgb[None]
    n = rgb.shape[0]
    H, W = fmt.height, fmt.width
    if tuple(rgb.shape[2:]) != (H, W):
        raise ValueError(f"rgb_to_yuv: rgb is {tuple(rgb.shape)}, the format {H} x {W}")
    item, plane, pitch = _rgb_strides(rgb, n, H, W, "rgb_to_yuv: rgb")
    if out is None:
        out = torch.empty(n, fmt.frame_bytes, device=rgb.device, dtype=torch.uint8)
    f, y, u, v, n_out = _yuv_planes(out, fmt)
    if n_out != n:
        raise ValueError(f"rgb_to_yuv: out holds {n_out} frames, rgb {n}")
    _launch("stif_rgb_to_yuv", None, L.lib().stif_rgb_to_yuv, C.byref(f), _vp(rgb), item, plane, pitch, n, y, u, v,
            _stream())
    return out


# ----------------------------------------------------------------------------- scene cuts
def scene_sad(frames, h=None, w=None):
    """Sum of absolute differences of the 8-bit luma of every adjacent pair of ``frames`` (stif_scene_sad): a
    float32 CUDA tensor [n >= 2, 3, H, W] with contiguous rows (any view ``_rgb_strides`` accepts) -> an int64 device
    tensor [n - 1].  ``h``, ``w`` select the top-left h x w rectangle (default: all of H x W), so a padded model
    input is scored without its padding.  Exact integers; nothing is read back here."""
    if frames.dim() != 4 or frames.shape[0] < 2:
        raise ValueError(f"scene_sad: frames must be [n >= 2, 3, H, W], got {tuple(frames.shape)}")
    n = frames.shape[0]
    h = frames.shape[2] if h is None else int(h)
    w = frames.shape[3] if w is None else int(w)
    if not (1 <= h <= frames.shape[2] and 1 <= w <= frames.shape[3]):
        raise ValueError(f"scene_sad: the rectangle {h} x {w} does not lie in {tuple(frames.shape)}")
    item, plane, pitch = _rgb_strides(frames, n, h, w, "scene_sad: frames")
    sad = torch.empty(n - 1, device=frames.device, dtype=torch.int64)
    ws = torch.empty(max(1, L.lib().stif_scene_workspace_size(n, h, w) // 8), device=frames.device, dtype=torch.int64)
    _launch("stif_scene_sad", None, L.lib().stif_scene_sad, _vp(frames), item, plane, pitch, n, h, w, _vp(sad),
            _vp(ws), ws.numel() * 8, _stream())
    return sad
