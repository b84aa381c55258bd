"""LunaTokis host: the reference model API driving the gfx950 kernels.

Mirrors ``codes/models/modules/Sakuya_arch_test.py:LunaTokis`` -- constructor
``LunaTokis(nf, nframes, groups, front_RBs, back_RBs)`` (:268-311),
``forward(x, times, scale=None, test=False)`` (:1222-1231), ``gen_feat`` (:313-362),
``decoding`` (:364-459), ``load_state_dict(sd, strict=True)`` over the reference's
442 keys -- as an ``nn.Module`` whose parameters are those 442 tensors, but every layer
runs through libstif_hip.so (ops.py) on repacked copies (packing.py); no torch.nn layer
is on the path.

Work is batched across everything the reference runs sequentially but that is
independent: both PCD_Align directions (different weights -> launch groups), both
ConvLSTM directions (BiDeformableConvLSTM runs the same net on x and reversed x,
:256-266), pcd_h and pcd_c, all pairs of a window, and all three latent steps of
the reconstruction trunk.  Per-frame encoder features are computed once per frame
(a sliding window shares each inner frame between two pairs), and so is the
BiConvLSTM's first step, which reads one frame and the zero state only (step0_plan).
"""
from __future__ import annotations

import contextlib
import math
import warnings
import threading
from collections import OrderedDict

import numpy as np
import torch
from torch import nn

from . import _lib as L
from . import ops
from . import weights as W
from .coords import (check_points, check_window, classify_point_query, classify_time_query, ensemble_weights,
                     point_passes, point_strides, tile_windows, window_from_center)
from .packing import pack_model

_CONST_LOCK = threading.Lock()   # _const's dict is shared by DataParallel replicas (replicate() threads)


def _np(v):
    if isinstance(v, np.ndarray):
        return v.astype(np.float32, copy=False)
    return v.detach().cpu().numpy().astype(np.float32, copy=False)


def _drain(gen):
    """Run a stage generator (see LunaTokis._lockstep) to completion; returns its return value."""
    while True:
        try:
            next(gen)
        except StopIteration as e:
            return e.value


def _split(n, k):
    """Items [0, n) as up to ``k`` contiguous ranges of ceil(n / k) items (the last one may be shorter)."""
    per = -(-n // max(1, min(k, n)))
    return [(c0, min(n, c0 + per)) for c0 in range(0, n, per)]


def _bases(counts):
    """Prefix offsets of per-set item counts: set i holds items [b[i], b[i + 1]) of a flat buffer."""
    b = [0]
    for c in counts:
        b.append(b[-1] + c)
    return b


def step0_plan(pairs, window):
    """The launches around the BiConvLSTM's first step for one chunk of ``pairs`` pairs, as item counts per
    weight set (pure: no device, no tensors).  ``window``: the pairs are the adjacent pairs of ``pairs + 1``
    frames of one sequence, whose per-frame features the caller holds.  Then step 0 -- which reads one frame
    and the all-zero state only, with the same weights in both directions -- runs once per frame: pair b's
    forward recurrence continues from frame b's (h0, c0), its reversed one from frame b + 1's.

    Returns a dict: ``frames`` (per-frame items, None without sharing), ``fwd`` / ``rev`` (the frame ranges
    whose h0 / c0 the two recurrences of the chunk's pairs read) and ``launches``, an ordered dict
    name -> item count of every weight set of that launch group, in launch order:
      first_pcd        PCD_Align of the frame pairs, sets (alignment direction)
      first_fusion     its 1x1 fusion conv
      input_pyramid    Easy_PCD pyramids of the LSTM inputs, sets (pcd, input); on the window path sets (pcd) of
                       the frames (the middle latent's ride in step1_pyramid)
      step0_pcd        step 0's alignments, sets (pcd, [direction,] alignment direction); ``zero_l1`` lists the
                       sets whose L1 input is the zero state (no L1 offset branch, no L1 DCN)
      step0_fusion     Easy_PCD.fusion, sets (pcd[, direction])
      step0_cell       the ConvLSTM cell, sets (direction) or one per-frame set
      step1_pyramid    pyramids of step 1's state (h0, c0), sets (pcd[, direction]); on the window path the middle
                       latent's input pyramids ride along as two more sets of ``pairs`` items."""
    B = int(pairs)
    if B < 1:
        raise ValueError("step0_plan: at least one pair")
    if not window:
        return dict(frames=None, fwd=None, rev=None, zero_l1=(1, 3, 5, 7), launches=OrderedDict(
            first_pcd=[B, B], first_fusion=[B], input_pyramid=[B] * 6, step0_pcd=[B] * 8, step0_fusion=[B] * 4,
            step0_cell=[B, B], step1_pyramid=[B] * 4))
    F = B + 1
    return dict(frames=F, fwd=(0, B), rev=(1, F), zero_l1=(1, 3), launches=OrderedDict(
        first_pcd=[B, B], first_fusion=[B], input_pyramid=[F, F], step0_pcd=[F] * 4, step0_fusion=[F, F],
        step0_cell=[F], step1_pyramid=[F, F, B, B]))


_NO_CAPTURE = ("a windowed / tiled decode reads the HRfeat bounding box back on the host: "
               "it cannot be captured in a hipGraph")


def _hr_size(H, Wd, scale):
    """(HH, WW) of decoding's virtual grid: ``scale`` itself, x4 by default."""
    return (H * 4, Wd * 4) if scale is None else (int(scale[0]), int(scale[1]))


class _Container(nn.Module):
    """A plain node of the reference's module tree (holds the reference parameters by their key)."""


class LunaTokis(nn.Module):
    """STIF LunaTokis (Sakuya_arch_test.py:268) on MI355X.

    An ``nn.Module`` whose parameters are exactly the reference's 442 state-dict tensors (same keys,
    shapes and registration order; ``requires_grad=False``: inference engine), so ``state_dict``,
    ``load_state_dict``, ``.to()`` / ``.cuda()`` and ``nn.DataParallel`` (VideoSR_base_model.py:29-32)
    behave as on the reference module.  The kernels read repacked copies of those weights
    (non-persistent buffers under ``_pk``, derived at ``load_state_dict``; they move and replicate with
    the module), never the parameters themselves."""

    def __init__(self, nf=64, nframes=3, groups=8, front_RBs=5, back_RBs=10, device="cuda", winograd=True,
                 mfma="f16x3", range_check="rerun", chunk_px=2 ** 21, lanes=1, dec_chunk_px=2 ** 25,
                 fused_dcn=True, trunk_lanes=2, dec_lanes=None, lstm_lanes=1, pcd_streams=1, const_shapes=2):
        super().__init__()
        if nf != 64 or groups != 8:
            raise ValueError("the gfx950 kernels implement nf=64, groups=8 (the shipped STIF configuration)")
        self.nf, self.groups = nf, groups
        self.in_frames = 1 + nframes // 2        # unused attributes kept for API parity (:272-273)
        self.ot_frames = nframes
        self.front_RBs, self.back_RBs = front_RBs, back_RBs
        self._spec = W.state_dict_spec(nf, front_RBs, back_RBs, groups)
        dev = torch.device(device)
        # the reference module tree: one parameter per state-dict key, registered in key order
        for key, shape in self._spec.items():
            *path, leaf = key.split(".")
            node = self
            for name in path:
                if name not in node._modules:
                    node.add_module(name, _Container())
                node = node._modules[name]
            node.register_parameter(leaf, nn.Parameter(torch.zeros(shape, device=dev), requires_grad=False))
        self._pk = _Container()                   # packed kernel weights (non-persistent buffers)
        self._meta = {}                           # layer name -> (buffer index, cout, cin, ks, mode)
        self._meta32 = None                       # fp32 re-packing of the f16x3 layers (range fallback)
        self.register_buffer("_range_status", torch.zeros(1, dtype=torch.int32, device=dev), persistent=False)
        self._host = None
        self._layers_key = None
        self.layers, self._dec_flags = {}, 0      # the layer set in use and its decoder operand flags (_use)
        self._feat = None
        self.inp = None
        self._tables = {}
        self.training = False
        # 3x3 convs by Winograd F(2x2,3x3) where the shape allows (fp32 throughout); False = direct
        self.winograd = bool(winograd)
        # operand arithmetic: "f32" (fp32 MFMA) or "f16x3" (fp32 products from three fp16 MFMAs on split
        # operands, ~22-bit operands, fp32 accumulation; stif.h)
        if mfma not in ("f32", "f16x3"):
            raise ValueError("mfma must be 'f32' or 'f16x3'")
        self.mfma = mfma
        # f16x3: DCN_sep as one kernel (offset/mask conv + sigmoid + deformable conv, k_dcn_sep); False =
        # the offset/mask conv (k_wino_om) and the deformable conv (k_dcn) as two launches
        self.fused_dcn = bool(fused_dcn)
        # f16x3 activations outside the split range: "rerun" the call in fp32 (warning), "raise", or "off"
        if range_check not in ("rerun", "raise", "off"):
            raise ValueError("range_check must be 'rerun', 'raise' or 'off'")
        self.range_check = range_check
        self.range_reruns = 0
        # pairs per encoder pass: a window is processed in chunks of about chunk_px LR pixels, which
        # bounds the PCD / BiConvLSTM working set (~20 KB per pair-pixel) at large frames
        self.chunk_px = int(chunk_px)
        # HR pixels per decoder pass (decoding): bounds the decoder's scratch (~9 GB at the default)
        self.dec_chunk_px = int(dec_chunk_px)
        self.last_window_F = None            # HRfeat rectangle of the last window decoded (_decode_windowed)
        self.window_peak_scratch_bytes = 0   # and the largest per-pass decoder scratch of that call
        # independent pair ranges run as `lanes` concurrent HIP streams (_run_lanes), so one lane's kernels
        # could fill the others' tail waves and dispatch gaps; results do not depend on it.  Default 1:
        # at C0, 2 lanes measured 5 % slower (82.5 -> 76.7, 84.6 -> 80.4 Mpix/s, same box) -- the
        # persistent, XCD-mapped kernels lose more to sharing the CUs than the gaps cost
        if int(lanes) < 1:
            raise ValueError("lanes must be >= 1")
        self.lanes = int(lanes)
        # the recon trunk's items (3 latents per pair, independent chains of 80 convs) split over
        # `trunk_lanes` streams, block by block round-robin, so one half's tail waves overlap the other's.
        # At C0 (18 items = 2,304 tiles = 4.5 per persistent workgroup) 2 streams measured -0.1 to -0.5 ms
        # per step against 1, 3 streams +0.2 ms; splitting the 7-frame feature_extraction stack the same
        # way measured slower (profiles/r05_trunk_lanes_ab.log)
        if int(trunk_lanes) < 1:
            raise ValueError("trunk_lanes must be >= 1")
        self.trunk_lanes = int(trunk_lanes)
        # the BiConvLSTM's two directions on two streams (lstm_lanes=2): bit-identical, but measured
        # +0.9 ms per C0 step (17.2 vs 16.3 ms, profiles/r05_trunk_lanes_ab.log) -- half-size PCD launches
        # of two chains competing for the CUs; default 1
        if int(lstm_lanes) not in (1, 2):
            raise ValueError("lstm_lanes must be 1 or 2")
        self.lstm_lanes = int(lstm_lanes)
        # PCD alignment: the DCN / feature branch on a second stream (_pcd_align); bit-identical, measured
        # equal to one stream at C0 with either tile schedule (profiles/r05_dynamic_tiles_ab.log); default 1
        if int(pcd_streams) not in (1, 2):
            raise ValueError("pcd_streams must be 1 or 2")
        self.pcd_streams = int(pcd_streams)
        # decoding's pair ranges on their own streams (None: follow `lanes`)
        if dec_lanes is not None and int(dec_lanes) < 1:
            raise ValueError("dec_lanes must be >= 1")
        self.dec_lanes = None if dec_lanes is None else int(dec_lanes)
        self._lane_streams = {}
        self._active = False
        # weight-only constant maps (_const) are kept for this many (items, H, W) shapes per device
        if int(const_shapes) < 1:
            raise ValueError("const_shapes must be >= 1")
        self.const_shapes = int(const_shapes)

    # ------------------------------------------------------------------ nn.Module API
    @property
    def device(self):
        return self.conv_first.weight.device

    def train(self, mode=True):
        if mode:
            raise NotImplementedError("training (DCNv2 backward) is out of scope; inference only")
        return super().train(False)

    def to(self, *args, **kwargs):
        device, dtype, _, _ = torch._C._nn._parse_to(*args, **kwargs)
        if dtype is not None and dtype != torch.float32:
            raise NotImplementedError("LunaTokis (stif_amd) computes in fp32 (operand modes: mfma='f32'|'f16x3')")
        out = super().to(*args, **kwargs)
        with _CONST_LOCK:   # the constant maps of the device the module left are not used again
            consts = self.__dict__.get("_consts")
            if consts:
                for g in [g for g in consts if g[0] != str(self.device)]:
                    del consts[g]
        return out

    def half(self):
        raise NotImplementedError("LunaTokis (stif_amd) computes in fp32")

    bfloat16 = double = half

    def load_state_dict(self, state_dict, strict=True, assign=False):
        """Same key contract as nn.Module.load_state_dict on the reference module; a 'module.' prefix
        (DataParallel/DDP checkpoints) is stripped as base_model.py:93-98 does.  Repacks the kernel
        weights on the parameters' device."""
        sd = OrderedDict()
        for k, v in state_dict.items():
            sd[k[7:] if k.startswith("module.") else k] = v
        missing = [k for k in self._spec if k not in sd]
        unexpected = [k for k in sd if k not in self._spec]
        if strict and (missing or unexpected):
            raise RuntimeError("Error(s) in loading state_dict for LunaTokis:\n"
                               f"\tMissing key(s): {missing}\n\tUnexpected key(s): {unexpected}")
        params = dict(self.named_parameters())
        host = OrderedDict()
        for k, shape in self._spec.items():
            if k in sd:
                a = _np(sd[k])
                if tuple(a.shape) != tuple(shape):
                    raise RuntimeError(f"size mismatch for {k}: copying a param with shape {tuple(a.shape)}, "
                                       f"the shape in current model is {tuple(shape)}")
                host[k] = np.ascontiguousarray(a)
                params[k].data.copy_(torch.from_numpy(host[k]))
            elif self._host is not None:
                host[k] = self._host[k]
            else:
                host[k] = params[k].detach().cpu().numpy().astype(np.float32)
        self._host = host
        self._pk, self._meta = self._packed(self.mfma)
        self._meta32 = None        # the fp32 copy, the decoder tables and the constant maps follow the weights
        self._tables = {}
        self._consts = OrderedDict()
        self._use(self._build_layers(self._pk, self._meta), self._meta)
        self._layers_key = self._pk.b0.data_ptr()
        return type("IncompatibleKeys", (), {"missing_keys": missing, "unexpected_keys": unexpected})()

    # ------------------------------------------------------------------ packed layers
    def _packed(self, mfma):
        """The host weights packed for the kernels (packing.pack_model) on the parameters' device, as
        non-persistent buffers b0..bN of a new container (so they move and replicate with the module), and
        their meta."""
        bufs, meta = pack_model(self._host, self.device, mfma=mfma, winograd=self.winograd, fused_dcn=self.fused_dcn,
                                front_RBs=self.front_RBs, back_RBs=self.back_RBs)
        pk = _Container()
        for i, b in enumerate(bufs):
            pk.register_buffer(f"b{i}", b, persistent=False)
        return pk, meta

    def _use(self, layers, meta):
        """Make ``layers`` (built from ``meta``) the layer set the kernels run with."""
        self.layers, self._dec_flags = layers, meta["dec.mlp"][1]

    def _build_layers(self, pk, meta):
        bufs = pk._buffers
        lay = {}
        for name, m in meta.items():
            w, b = bufs[f"b{m[0]}"], bufs[f"b{m[0] + 1}"]
            lay[name] = w if name == "dec.mlp" else ops.PackedConv(w, b, *m[1:])
        return lay

    def _layers_fp32(self):
        """The f16x3 layers re-packed in fp32 (range fallback), as non-persistent buffers of ``_pk32``."""
        if self._meta32 is None or self._pk32.b0.device != self.device:
            self._pk32, self._meta32 = self._packed("f32")
        return self._build_layers(self._pk32, self._meta32)

    # ------------------------------------------------------------------ call wrapper
    def _call(self, fn, *args, **kwargs):
        """Run a public entry point on the module's device (its current stream), with the packed
        layers of this module (or replica).  With f16x3 operands the kernels report non-finite
        outputs in ``_range_status``; the call is then re-run in fp32 (range_check='rerun') or
        raises (range_check='raise')."""
        if self._host is None:
            raise RuntimeError("LunaTokis: call load_state_dict first")
        dev = self.device
        if dev.type != "cuda":
            raise L.StifError("LunaTokis (stif_amd) runs on the GPU only: move it with .to('cuda')")
        if self._active:                       # nested entry (e.g. decoding_fasttest -> decoding)
            return fn(*args, **kwargs)
        with torch.cuda.device(dev):
            key = self._pk.b0.data_ptr()
            if self._layers_key != key:
                self._use(self._build_layers(self._pk, self._meta), self._meta)
                self._layers_key = key
            check = self.range_check != "off" and (self.mfma == "f16x3")
            # inside a hipGraph capture the status word is still zeroed and written by the captured
            # kernels, but read by the caller after each replay (tools/graph_step.py), not here
            capturing = torch.cuda.is_current_stream_capturing()
            self._active = True
            try:
                if check:
                    self._range_status.zero_()
                out = fn(*args, **kwargs)
                if check and not capturing and int(self._range_status.item()):
                    if self.range_check == "raise":
                        raise L.StifError("f16x3 operand outside the split-fp16 range (|activation| >= 1024): "
                                          "use LunaTokis(mfma='f32') or range_check='rerun'", L.E_RANGE)
                    warnings.warn("LunaTokis: an f16x3 operand left the split-fp16 range; re-running this call "
                                  "with fp32 MFMA operands", RuntimeWarning, stacklevel=3)
                    self.range_reruns += 1
                    keep = self.layers
                    self._use(self._layers_fp32(), self._meta32)
                    try:
                        out = fn(*args, **kwargs)
                    finally:
                        self._use(keep, self._meta)
            finally:
                self._active = False
        return out

    @property
    def _status(self):
        return self._range_status if self.range_check != "off" else None

    # ------------------------------------------------------------------ encoder pieces
    def _conv(self, groups, **kw):
        ops.conv2d(groups, status=self._status, **kw)

    def _dcn(self, groups, **kw):
        ops.dcn(groups, status=self._status, **kw)

    def _dcn_sep(self, items, epi=L.EPI_NONE):
        """DCN_sep.forward (dcn_v2.py:127-140) for a launch group of items (layer name, fea, inp, out):
        the fused kernel where both layers are packed for it, else conv_offset_mask (OFFMASK epilogue)
        into a 216-channel map and the deformable conv."""
        lay = self.layers
        fused = [it for it in items if ops.dcn_sep_fusable(lay[it[0] + ".conv_offset_mask"], lay[it[0]])]
        rest = [it for it in items if not ops.dcn_sep_fusable(lay[it[0] + ".conv_offset_mask"], lay[it[0]])]
        if fused:
            ops.dcn_sep([dict(om_layer=lay[n + ".conv_offset_mask"], layer=lay[n], fea=f, inp=x, out=o)
                         for n, f, x, o in fused], epi=epi, status=self._status)
        if rest:
            om = self._sets([f.shape[0] for _, f, _, _ in rest], *rest[0][1].shape[1:3], 216)
            self._conv([dict(layer=lay[n + ".conv_offset_mask"], in0=f, out=om[i]) for i, (n, f, x, o) in enumerate(rest)],
                       epi=L.EPI_OFFMASK)
            self._dcn([dict(layer=lay[n], inp=x, offmask=om[i], out=o) for i, (n, f, x, o) in enumerate(rest)], epi=epi)

    def _empty(self, *shape):
        return torch.empty(*shape, device=self.device, dtype=torch.float32)

    def _sets(self, counts, *shape):
        """One buffer per weight set of a launch, set i with counts[i] items of ``shape``: slices of one
        allocation, so all share the item stride a launch requires."""
        flat, b = self._empty(sum(counts), *shape), _bases(counts)
        return [flat[b[i]:b[i + 1]] for i in range(len(counts))]

    def _const(self, key, shape, make):
        """Maps that depend only on the packed weights and a shape (the all-zero initial state, its
        pyramids, the zero-state L1 DCN output), computed on first use and kept until the layers are
        re-packed.  Entries are grouped by (device, shape): the key holds the weight buffers' addresses
        (so the fp32 range re-run's layers get their own entries) and the device is part of every
        group, so DataParallel replicas -- which share this dict through replicate()'s shallow
        __dict__ copy -- and a module moved by .to() never receive another device's tensors.  At most
        ``const_shapes`` groups per device are kept (least recently used evicted): one C0 group is
        ~0.1 GB, a 720p / 1080p group ~1.7 / 2 GB, so a serving process that sees many resolutions
        holds at most two of them.  Not cached inside a hipGraph capture (computed in the graph)."""
        if self.device.type == "cuda" and torch.cuda.is_current_stream_capturing():
            return make()
        dev = str(self.device)
        grp = (dev,) + tuple(int(s) for s in shape)
        with _CONST_LOCK:
            consts = self.__dict__.get("_consts")
            if not isinstance(consts, OrderedDict):
                consts = self.__dict__["_consts"] = OrderedDict()
            ent = consts.get(grp)
            if ent is not None and key in ent:
                consts.move_to_end(grp)
                return ent[key]
        v = make()
        if self.device.type == "cuda":   # once: other streams (lanes) read it without an event
            torch.cuda.current_stream(self.device).synchronize()
        with _CONST_LOCK:
            consts.setdefault(grp, {})[key] = v
            consts.move_to_end(grp)
            mine = [g for g in consts if g[0] == dev]
            for g in mine[:max(0, len(mine) - max(1, self.const_shapes))]:
                del consts[g]
        return v

    def _zeros(self, *shape):
        # grouped with the other maps of the same (items, H, W)
        return self._const(("zeros",) + tuple(shape), shape[:3],
                           lambda: torch.zeros(*shape, device=self.device, dtype=torch.float32))

    def _frame_features(self, frames):
        """conv_first + feature_extraction + pyramid (:318-325) for frames [n,3,H,W] (NCHW)."""
        return _drain(self._frame_features_steps(frames))

    def _frame_features_steps(self, frames):
        n, _, H, Wd = frames.shape
        l1 = self._empty(n, H, Wd, 64)
        ops.conv_first(frames, self.layers["conv_first"].w, self.layers["conv_first"].b, l1)
        tmp = self._empty(n, H, Wd, 64)
        yield from self._resblocks(l1, tmp, [f"feature_extraction.{i}" for i in range(self.front_RBs)])
        l2, l3 = self._pyramid([(l1, "")])
        return l1, l2[0], l3[0]

    # ------------------------------------------------------------------ lanes
    def _streams(self, k, pool="lanes"):
        dev = self.device
        ss = self._lane_streams.setdefault((pool, str(dev)), [])
        while len(ss) < k:
            ss.append(torch.cuda.Stream(device=dev))
        return ss[:k]

    def _lockstep(self, gens, pool):
        """Advance the generators ``gens`` in lock step (generator: one yield per round).  Each ``yield``
        of a generator is a point where the others may issue.  One generator runs on the current stream,
        with no stream call at all (the default path, and what a hipGraph capture sees).  Several run on
        one stream each of ``pool``, forked from and joined back into the current stream, and advance
        round-robin (a finished one drops out), so every stream has queued work from the start and the
        kernels of one fill the last waves and the dispatch gaps of the others."""
        if len(gens) == 1:
            yield from gens[0]
            return
        main = torch.cuda.current_stream()
        streams = self._streams(len(gens), pool)
        for s in streams:
            s.wait_stream(main)
        live = list(zip(streams, gens))
        while live:
            nxt = []
            for s, g in live:
                with torch.cuda.stream(s):
                    try:
                        next(g)
                        nxt.append((s, g))
                    except StopIteration:
                        pass
            live = nxt
            if live:
                yield
        for s in streams:
            main.wait_stream(s)

    def _run_lanes(self, n, make, lanes=None, pool="lanes"):
        """Items [0, n) in up to ``self.lanes`` contiguous ranges, each on its own stream (_lockstep);
        ``make(c0, c1)`` is a generator issuing one range's launches.  Every kernel computes each item
        independently of the batch it is launched in, so the results are bit-identical for any lane
        count."""
        _drain(self._lockstep([make(c0, c1) for c0, c1 in _split(n, self.lanes if lanes is None else lanes)], pool))

    def _resblocks(self, x, tmp, names, lanes=1):
        """A stack of ResidualBlock_noBN on x [n, H, W, 64] in place (generator, one yield per block).
        The items are independent chains, so with ``lanes`` > 1 they are split into that many
        contiguous ranges on their own streams, issued block by block round-robin: one range's tail
        waves and dispatch gaps overlap the other's work.  Bit-identical for any split."""
        ranges = _split(x.shape[0], lanes)
        if len(ranges) > 1:
            yield from self._lockstep([self._resblocks(x[c0:c1], tmp[c0:c1], names) for c0, c1 in ranges], "trunk")
            return
        for name in names:
            self._resblock(x, tmp, name)
            yield

    def _resblock(self, x, tmp, name):
        """ResidualBlock_noBN (module_util.py:48-52), x updated in place."""
        self._conv([dict(layer=self.layers[name + ".conv1"], in0=x, out=tmp)], epi=L.EPI_RELU)
        self._conv([dict(layer=self.layers[name + ".conv2"], in0=tmp, out=x, res=x)], epi=L.EPI_RES)

    def _pyramid(self, srcs):
        """fea_L2_conv1/2, fea_L3_conv1/2 with lrelu for a list of (L1 map, weight prefix): one launch per
        layer over the sources as weight sets, each with its own number of items.  Returns the L2 and the
        L3 maps, one per source."""
        _, H, Wd, _ = srcs[0][0].shape
        counts = [s.shape[0] for s, _ in srcs]
        a2 = self._sets(counts, H // 2, Wd // 2, 64)
        b2 = self._sets(counts, H // 2, Wd // 2, 64)
        a3 = self._sets(counts, H // 4, Wd // 4, 64)
        b3 = self._sets(counts, H // 4, Wd // 4, 64)
        lay = self.layers
        self._conv([dict(layer=lay[p + "fea_L2_conv1"], in0=s, out=a2[i]) for i, (s, p) in enumerate(srcs)],
                   epi=L.EPI_LRELU, stride=2)
        self._conv([dict(layer=lay[p + "fea_L2_conv2"], in0=a2[i], out=b2[i]) for i, (s, p) in enumerate(srcs)],
                   epi=L.EPI_LRELU)
        self._conv([dict(layer=lay[p + "fea_L3_conv1"], in0=b2[i], out=a3[i]) for i, (s, p) in enumerate(srcs)],
                   epi=L.EPI_LRELU, stride=2)
        self._conv([dict(layer=lay[p + "fea_L3_conv2"], in0=a3[i], out=b3[i]) for i, (s, p) in enumerate(srcs)],
                   epi=L.EPI_LRELU)
        return b2, b3

    def _pcd_align(self, units, zero_l1=()):
        """PCD_Align.forward (:71-130) for up to 16 independent (module, direction) units, each a weight set
        of every launch with its own number of items (sets of frames and sets of pairs may share a launch;
        the window's per-frame step 0 uses sets of frames, _step0_shared).
        unit = (prefix, d, fa[L1,L2,L3], fb[L1,L2,L3], y_out).  ``zero_l1``: indices of units whose
        fa L1 map is all zeros (the ConvLSTM's initial state, convlstm.py:60-63, sampled by the
        reversed-direction alignment of the first step): their L1 DCN samples only zeros, so its output
        is its bias wherever the offsets land (DCN_sep, dcn_v2.py:127-140: sum of 0 * w + b), and the
        L1 offset branch that only steers it (L1_offset_conv1..3, conv_offset_mask) is not run for
        them -- bit-identical to running it (for finite offsets)."""
        _, H, Wd, _ = units[0][2][0].shape
        ns = [u[2][0].shape[0] for u in units]          # items per unit
        lay = self.layers
        lv = [(H, Wd), (H // 2, Wd // 2), (H // 4, Wd // 4)]

        def buf(level, c=64):
            return self._sets(ns, *lv[level], c)

        def L_(u, name):
            return lay[f"{u[0]}{name}_{u[1]}"]

        conv = self._conv
        E = enumerate
        # pcd_streams = 2: the DCN / feature branch (L3 DCN; L2 DCN + fea conv; L1 DCN + fea conv) on a
        # side stream, each part forked when its offsets are ready, so it overlaps the offset convs of the
        # next level (which depend on the offsets only) -- the under-filled L3 launches and the tails of
        # every launch get work beside them
        main = torch.cuda.current_stream()
        side = self._streams(1, pool="pcd")[0] if self.pcd_streams > 1 else None

        def branch():
            if side is None:
                return contextlib.nullcontext()
            side.wait_stream(main)
            return torch.cuda.stream(side)

        def conv_up(make, coarse, scale, epi):
            """conv on cat(x, scale * up2(coarse)) for every unit, the x2 upsample fused into the
            conv's staging (Winograd: expanded from an LDS-staged coarse patch per tile; direct
            kernel: register-staged) -- the upsampled map never reaches HBM"""
            conv([make(i, u, coarse[i]) for i, u in E(units)], epi=epi, in1_mode=2, in1_scale=scale)
        # ---- L3
        o = buf(2)
        conv([dict(layer=L_(u, "L3_offset_conv1"), in0=u[2][2], in1=u[3][2], out=o[i]) for i, u in E(units)],
             epi=L.EPI_LRELU, in1_mode=1)
        l3off = buf(2)
        conv([dict(layer=L_(u, "L3_offset_conv2"), in0=o[i], out=l3off[i]) for i, u in E(units)], epi=L.EPI_LRELU)
        l3fea = buf(2)
        with branch():
            self._dcn_sep([(f"{u[0]}L3_dcnpack_{u[1]}", l3off[i], u[2][2], l3fea[i]) for i, u in E(units)],
                          L.EPI_LRELU)
        # ---- L2
        o1 = buf(1)
        conv([dict(layer=L_(u, "L2_offset_conv1"), in0=u[2][1], in1=u[3][1], out=o1[i]) for i, u in E(units)],
             epi=L.EPI_LRELU, in1_mode=1)
        o2 = buf(1)
        conv_up(lambda i, u, c: dict(layer=L_(u, "L2_offset_conv2"), in0=o1[i], in1=c, out=o2[i]),
                l3off, 2.0, L.EPI_LRELU)
        l2off = buf(1)
        conv([dict(layer=L_(u, "L2_offset_conv3"), in0=o2[i], out=l2off[i]) for i, u in E(units)], epi=L.EPI_LRELU)
        d2 = buf(1)
        l2fea = buf(1)
        with branch():
            self._dcn_sep([(f"{u[0]}L2_dcnpack_{u[1]}", l2off[i], u[2][1], d2[i]) for i, u in E(units)])
            conv_up(lambda i, u, c: dict(layer=L_(u, "L2_fea_conv"), in0=d2[i], in1=c, out=l2fea[i]),
                    l3fea, 1.0, L.EPI_LRELU)
        # ---- L1 (offset branch and DCN for the units whose fa L1 is not all zeros; k = their index)
        live = [(i, u) for i, u in E(units) if i not in zero_l1]
        d1 = buf(0)
        if live:
            nl = [ns[i] for i, _ in live]
            o1 = self._sets(nl, H, Wd, 64)
            conv([dict(layer=L_(u, "L1_offset_conv1"), in0=u[2][0], in1=u[3][0], out=o1[k])
                  for k, (i, u) in E(live)], epi=L.EPI_LRELU, in1_mode=1)
            o2 = self._sets(nl, H, Wd, 64)
            conv([dict(layer=L_(u, "L1_offset_conv2"), in0=o1[k], in1=l2off[i], out=o2[k]) for k, (i, u) in E(live)],
                 epi=L.EPI_LRELU, in1_mode=2, in1_scale=2.0)
            l1off = self._sets(nl, H, Wd, 64)
            conv([dict(layer=L_(u, "L1_offset_conv3"), in0=o2[k], out=l1off[k]) for k, (i, u) in E(live)],
                 epi=L.EPI_LRELU)
            del o1, o2
            with branch():
                self._dcn_sep([(f"{u[0]}L1_dcnpack_{u[1]}", l1off[k], u[2][0], d1[i]) for k, (i, u) in E(live)])
        # the zero-state units' L1 DCN output is its bias everywhere: a constant map, kept across calls
        d1z = {}
        for i in zero_l1:
            b, n = L_(units[i], "L1_dcnpack").b, ns[i]
            d1z[i] = self._const(("dcn_bias", b.data_ptr()), (n, H, Wd), lambda b=b, n=n: b.view(1, 1, 1, 64).expand(
                n, H, Wd, 64).contiguous())
        with branch():
            conv_up(lambda i, u, c: dict(layer=L_(u, "L1_fea_conv"), in0=d1z.get(i, d1[i]), in1=c, out=u[4]),
                    l2fea, 1.0, L.EPI_NONE)
        if side is not None:
            main.wait_stream(side)   # before any buffer of this call can be freed and reused on main

    def _step0_shared(self, fr):
        """The BiConvLSTM's step 0 of a window chunk, once per frame.  ``fr``: [L1, L2, L3] of the chunk's
        F = pairs + 1 frames.  Step 0 of either recurrence reads one frame, that frame's input pyramids and the
        all-zero state, through the same ConvBLSTM.forward_net weights in both directions: reversed step 0 of
        pair b and forward step 0 of pair b + 1 are the same function of frame b + 1, kernel for kernel, so it
        runs once per frame (step0_plan): F items per weight set where the per-pair form has 2 (F - 1).
        Returns (h0, c0, input pyramids): h0 / c0 [F, H, W, 64] -- read-only from here on, two recurrences
        continue from every inner frame's -- and the frames' L2 / L3 input pyramids per pcd."""
        F_, H, Wd, _ = fr[0].shape
        lay = self.layers
        pf = "ConvBLSTM.forward_net."
        pcds = (pf + "pcd_h.", pf + "pcd_c.")
        plan = step0_plan(F_ - 1, True)
        zero = self._zeros(F_, H, Wd, 64)               # the initial h and c (convlstm.py:60-63), never written
        fp2, fp3 = self._pyramid([(fr[0], pcds[p]) for p in range(2)])
        zkey = ("zero_pyr", lay[pcds[0] + "fea_L2_conv1"].w.data_ptr())
        z2, z3 = self._const(zkey, (F_, H, Wd), lambda: self._pyramid([(zero, pcds[p]) for p in range(2)]))
        Y = self._sets(plan["launches"]["step0_pcd"], H, Wd, 64)     # (pcd, align direction)
        units = []
        for p in range(2):
            f1, f2 = [fr[0], fp2[p], fp3[p]], [zero, z2[p], z3[p]]
            units.append((pcds[p] + "pcd_align.", 1, f1, f2, Y[2 * p]))
            units.append((pcds[p] + "pcd_align.", 2, f2, f1, Y[2 * p + 1]))
        # the reversed alignments sample the all-zero initial state at L1
        self._pcd_align(units, zero_l1=plan["zero_l1"])
        T = self._empty(2, F_, H, Wd, 64)               # Easy_PCD.fusion outputs per pcd
        self._conv([dict(layer=lay[pcds[p] + "fusion"], in0=Y[2 * p], in1=Y[2 * p + 1], out=T[p]) for p in range(2)],
                   in1_mode=1)
        h0, c0 = self._empty(F_, H, Wd, 64), self._empty(F_, H, Wd, 64)
        self._conv([dict(layer=lay[pf + "cell_list.0.conv"], in0=fr[0], in1=T[0], res=T[1], out=h0, out2=c0)],
                   epi=L.EPI_LSTM, in1_mode=1)
        return h0, c0, (fp2, fp3)

    def _bilstm_steps(self, X, feats=None, frames=None):
        """BiDeformableConvLSTM.forward (:256-266) with DeformableConvLSTM.forward (:192-242) for
        both directions batched.  X: the 3 latent inputs [B, H, W, 64] (t-major; views with one common
        item stride).  Returns [3,B,H,W,64] (in ``feats`` when given).
        ``frames``: [L1, L2, L3] of the B + 1 frames whose adjacent pairs the items are (X[0] = their L1[:-1],
        X[2] = L1[1:]): per-frame step 0 (_step0_shared), on the calling stream before the directions fork;
        steps 1 and 2 follow per pair, pair b's forward recurrence from frame b's (h0, c0) and its reversed
        one from frame b + 1's, as views of the per-frame buffers, which nothing writes (steps 1 and 2 put
        their c elsewhere)."""
        B, H, Wd, _ = X[0].shape
        lay = self.layers
        pf = "ConvBLSTM.forward_net."
        pcds = (pf + "pcd_h.", pf + "pcd_c.")
        shared = frames is not None
        cs = self._empty(2, B, H, Wd, 64)               # c of the last step run here (step 0 reads the zero state)
        if shared:
            h0, c0, (fp2, fp3) = self._step0_shared(frames)
            plan = step0_plan(B, True)
            fsl = [slice(*plan["fwd"]), slice(*plan["rev"])]   # the frames of direction d's step 0
            hs12 = self._empty(2, 2, B, H, Wd, 64)      # h of (direction, step 1 / 2)
            hs = {(d, t): h0[fsl[d]] if t == 0 else hs12[d, t - 1] for d in range(2) for t in range(3)}
            # step 1's state pyramids once per frame, from h0 / c0; the middle latent's input pyramids (per
            # pair) are two more weight sets of the same launches
            s2, s3 = self._pyramid([(h0, pcds[0]), (c0, pcds[1]), (X[1], pcds[0]), (X[1], pcds[1])])

            def xpyr(p, level, fr):
                if fr == 1:
                    return (s2 if level == 2 else s3)[2 + p]
                return (fp2 if level == 2 else fp3)[p][fsl[fr // 2]]
        else:
            hs_ = self._empty(2, 3, B, H, Wd, 64)       # h of (direction, step)
            hs = {(d, t): hs_[d, t] for d in range(2) for t in range(3)}
            zero = self._zeros(B, H, Wd, 64)            # the initial h and c (convlstm.py:60-63), never written
            # Easy_PCD pyramids (:148-160) of the inputs, once per (pcd, input): the forward direction reads
            # X[t] and the reversed one X[2 - t] with the same weights, so per-step pyramids of the inputs
            # would compute each of them twice (bit-identical results, half the work); groups (pcd, t)
            xp2, xp3 = self._pyramid([(X[t], pcds[p]) for p in range(2) for t in range(3)])

            def xpyr(p, level, fr):
                return (xp2 if level == 2 else xp3)[p * 3 + fr]

            # the step-0 state pyramids (zeros) once per pcd, depending on the weights only: kept across calls
            zkey = ("zero_pyr", lay[pcds[0] + "fea_L2_conv1"].w.data_ptr())
            z2, z3 = self._const(zkey, (B, H, Wd), lambda: self._pyramid([(zero, pcds[p]) for p in range(2)]))

        def step(t, ds):
            """Step t of the directions ds (0 forward, 1 reversed): state pyramids, PCD alignments,
            Easy_PCD fusion and the ConvLSTM cell, each one launch over (pcd, direction) groups."""
            fr = [t, 2 - t]                               # forward / reversed sequence
            xin = [X[f] for f in fr]
            pd = [(p, d) for p in range(2) for d in ds]
            if t == 0:
                st = {k: zero for k in pd}
                pyr = {(p, d): (z2[p], z3[p]) for p, d in pd}
            elif shared and t == 1:
                st = {(p, d): (h0 if p == 0 else c0)[fsl[d]] for p, d in pd}
                pyr = {(p, d): (s2[p][fsl[d]], s3[p][fsl[d]]) for p, d in pd}
            else:
                st = {(p, d): hs[d, t - 1] if p == 0 else cs[d] for p, d in pd}
                a2, a3 = self._pyramid([(st[p, d], pcds[p]) for p, d in pd])
                pyr = {k: (a2[i], a3[i]) for i, k in enumerate(pd)}
            nd = len(ds)
            Y = self._empty(2, nd, 2, B, H, Wd, 64)      # (pcd, dir, align direction)
            units = []
            for p in range(2):
                for j, d in enumerate(ds):
                    f1 = [xin[d], xpyr(p, 2, fr[d]), xpyr(p, 3, fr[d])]
                    f2 = [st[p, d], *pyr[p, d]]
                    units.append((pcds[p] + "pcd_align.", 1, f1, f2, Y[p, j, 0]))
                    units.append((pcds[p] + "pcd_align.", 2, f2, f1, Y[p, j, 1]))
            # step 0: the reversed alignments (odd units) sample the all-zero initial state at L1
            self._pcd_align(units, zero_l1=range(1, len(units), 2) if t == 0 else ())
            T = self._empty(2, nd, B, H, Wd, 64)         # Easy_PCD.fusion outputs: (pcd, dir)
            self._conv([dict(layer=lay[pcds[p] + "fusion"], in0=Y[p, j, 0], in1=Y[p, j, 1], out=T[p, j])
                        for p in range(2) for j in range(nd)], in1_mode=1)
            # ConvLSTMCell (convlstm.py:42-58): combined = cat(x, h~); c_next = f*c~ + i*g
            self._conv([dict(layer=lay[pf + "cell_list.0.conv"], in0=xin[d], in1=T[0, j], res=T[1, j],
                             out=hs[d, t], out2=cs[d]) for j, d in enumerate(ds)], epi=L.EPI_LSTM, in1_mode=1)

        def steps(ds):
            for t in range(1 if shared else 0, 3):
                step(t, ds)
                yield

        # lstm_lanes = 2: the two directions are independent recurrences, one stream each, step by step
        # (a window's per-frame step 0 ran before this fork, on the calling stream)
        yield from self._lockstep([steps((0, 1))] if self.lstm_lanes < 2 else [steps((0,)), steps((1,))], "lstm")
        if feats is None:
            feats = self._empty(3, B, H, Wd, 64)
        self._conv([dict(layer=lay["ConvBLSTM.conv_1x1"], in0=hs[0, t], in1=hs[1, 2 - t], out=feats[t])
                    for t in range(3)], in1_mode=1)
        return feats

    def _gen_feat_core(self, fea1, fea2, out, frames=None):
        """Everything after the per-frame features: PCD + fusion, BiConvLSTM, recon trunk, into
        out [3, B, H, W, 64] (generator: yields between stages, see _lockstep).
        fea1 / fea2: [L1, L2, L3] of the pairs' first / second frames (item = pair).
        ``frames``: [L1, L2, L3] of the B + 1 frames whose adjacent pairs these are (fea1 = frames[:-1],
        fea2 = frames[1:]; the window path hands them down, nothing is inferred from addresses): the
        BiConvLSTM's step 0 then runs once per frame (_bilstm_steps)."""
        B, H, Wd, _ = fea1[0].shape
        X1 = self._empty(B, H, Wd, 64)                  # the fused middle latent input
        Y = self._empty(2, B, H, Wd, 64)
        self._pcd_align([("pcd_align.", 1, fea1, fea2, Y[0]), ("pcd_align.", 2, fea2, fea1, Y[1])])
        self._conv([dict(layer=self.layers["fusion"], in0=Y[0], in1=Y[1], out=X1)], in1_mode=1)
        del Y
        yield
        # the inputs X = [fea1 L1, fused, fea2 L1] as views (no copies) when their item strides agree (the
        # sliding-window path: consecutive frames); the batched pyramid of the inputs needs one stride
        X = [fea1[0], X1, fea2[0]]
        if not all(x.stride(0) == X1.stride(0) for x in X):   # (a [1, ...] view counts as contiguous in torch)
            X = [X1 if x is X1 else self._empty(B, H, Wd, 64).copy_(x) for x in X]
        # the latents go straight into `out` when it is one contiguous block (one chunk of pairs)
        feats = yield from self._bilstm_steps(X, out if out.is_contiguous() else None, frames)
        del X, X1
        trunk = feats.view(3 * B, H, Wd, 64)
        tmp = self._empty(3 * B, H, Wd, 64)
        yield from self._resblocks(trunk, tmp, [f"recon_trunk.{i}" for i in range(self.back_RBs)], self.trunk_lanes)
        if feats is not out:
            out.copy_(feats)

    def _gen_feat_pairs(self, fea1, fea2, out, frames=None):
        """_gen_feat_core over chunks of about ``chunk_px`` LR pixels of pairs (balanced), so the
        working set stays bounded at large frames; pairs are independent, so chunking does not
        change a bit of the result (generator).  ``frames``: the per-frame features [L1, L2, L3] of the
        B + 1 frames of a window (fea1 / fea2 are its adjacent pairs): a chunk of k pairs shares the
        BiConvLSTM's first step among its own k + 1 frames (frames are shared inside a chunk only)."""
        B, H, Wd, _ = fea1[0].shape
        if frames is not None:
            if frames[0].shape[0] != B + 1:
                raise ValueError(f"{B} pairs need the features of {B + 1} frames, got {frames[0].shape[0]}")
            frames = [t.contiguous() for t in frames]    # one item stride for every set of the shared launches
            fea1, fea2 = [t[:-1] for t in frames], [t[1:] for t in frames]
        per = max(1, self.chunk_px // (H * Wd))
        nch = math.ceil(B / per)
        per = math.ceil(B / nch)
        for c0 in range(0, B, per):
            c1 = min(B, c0 + per)
            yield from self._gen_feat_core([t[c0:c1] for t in fea1], [t[c0:c1] for t in fea2], out[:, c0:c1],
                                           None if frames is None else [t[c0:c1 + 1] for t in frames])

    # ------------------------------------------------------------------ reference API
    def _check_input(self, x):
        x = x.to(self.device, torch.float32).contiguous()
        if x.dim() != 5 or x.shape[1] != 2 or x.shape[2] != 3:
            raise ValueError(f"x must be [B, 2, 3, H, W], got {tuple(x.shape)}")
        if x.shape[3] % 4 or x.shape[4] % 4:
            raise ValueError("H and W must be multiples of 4 (custom_video_test.py:44-48 pads to 4)")
        return x

    def gen_feat(self, x):
        """LunaTokis.gen_feat (:313-362): x [B,2,3,H,W] -> self.feat (NHWC [3,B,H,W,64] on device)."""
        return self._call(self._gen_feat, x)

    def _gen_feat(self, x):
        x = self._check_input(x)
        self.inp = x
        B, N, C, H, Wd = x.shape
        out = self._empty(3, B, H, Wd, 64)

        def lane(c0, c1):
            l1, l2, l3 = yield from self._frame_features_steps(x[c0:c1].reshape((c1 - c0) * N, C, H, Wd))
            fea1 = [l1[0::2], l2[0::2], l3[0::2]]
            fea2 = [l1[1::2], l2[1::2], l3[1::2]]
            yield from self._gen_feat_pairs(fea1, fea2, out[:, c0:c1])
        self._run_lanes(B, lane)
        self._feat = out
        return None

    def frame_features(self, frames):
        """Per-frame encoder (conv_first + feature_extraction + pyramid, :318-325) of frames
        [F,3,H,W] -> NHWC (L1, L2, L3); used for sliding windows and the halo exchange."""
        return self._call(lambda f: self._frame_features(f.to(self.device, torch.float32).contiguous()), frames)

    def gen_feat_window(self, frames, last_frame_feats=None, frame_feats=None):
        """Sliding-window gen_feat: frames [F,3,H,W] -> latents of the F-1 adjacent pairs, with the
        per-frame encoder run once per frame (the reference harness runs it twice per inner frame,
        custom_video_test.py:81-97).  ``frame_feats`` = (L1, L2, L3) of all F frames computed
        beforehand (frame_features + parallel.halo_exchange); ``last_frame_feats`` = those of the
        last frame only (the others are computed here)."""
        return self._call(self._gen_feat_window, frames, last_frame_feats, frame_feats)

    def _gen_feat_window(self, frames, last_frame_feats=None, frame_feats=None):
        frames = frames.to(self.device, torch.float32).contiguous()
        x = torch.stack([frames[:-1], frames[1:]], dim=1).contiguous()
        self.inp = self._check_input(x)
        F_ = frames.shape[0]
        _, _, H, Wd = frames.shape
        out = self._empty(3, F_ - 1, H, Wd, 64)
        if frame_feats is None and last_frame_feats is None:
            # lanes of pairs [c0, c1) each run the encoder on their frames c0..c1 (the frame two lanes
            # share is encoded by both, so no lane waits for another)
            def lane(c0, c1):
                l1, l2, l3 = yield from self._frame_features_steps(frames[c0:c1 + 1])
                yield from self._gen_feat_pairs([l1[:-1], l2[:-1], l3[:-1]], [l1[1:], l2[1:], l3[1:]],
                                                out[:, c0:c1], [l1, l2, l3])
            self._run_lanes(F_ - 1, lane)
            self._feat = out
            return None
        if frame_feats is not None:
            l1, l2, l3 = frame_feats
            if l1.shape[0] != F_:
                raise ValueError(f"frame_feats hold {l1.shape[0]} frames, the window {F_}")
        else:
            a1, a2, a3 = self._frame_features(frames[:-1].contiguous())
            l1, l2, l3 = (torch.cat([a, b.reshape(1, *a.shape[1:]).to(a.device)])
                          for a, b in zip((a1, a2, a3), last_frame_feats))
        self._run_lanes(F_ - 1, lambda c0, c1: self._gen_feat_pairs(
            [l1[c0:c1], l2[c0:c1], l3[c0:c1]], [l1[c0 + 1:c1 + 1], l2[c0 + 1:c1 + 1], l3[c0 + 1:c1 + 1]],
            out[:, c0:c1], [l1[c0:c1 + 1], l2[c0:c1 + 1], l3[c0:c1 + 1]]))
        self._feat = out
        return None

    @property
    def feat(self):
        """Latent video as the reference's [B, 3, 64, H, W] (a permuted view of the NHWC buffer)."""
        f = self.__dict__.get("_feat")
        return None if f is None else f.permute(1, 0, 4, 2, 3)

    @feat.setter
    def feat(self, v):
        if v is not None:
            raise AttributeError("feat is produced by gen_feat")
        self._feat = None

    def _time_vec(self, tq, B):
        if isinstance(tq, torch.Tensor):
            t = tq.detach().to(self.device, torch.float32).reshape(-1)
        else:
            t = torch.tensor([float(tq)], device=self.device, dtype=torch.float32)
        if t.numel() == 1:
            t = t.expand(B)
        if t.numel() != B:
            raise ValueError("each time query must hold 1 or B values")
        return t.contiguous()

    def _time_query(self, tq, B, HH, WW):
        """An entry of ``times`` as the decoder stages take it: the [B] time vector (``_time_vec``), or, for a
        tensor that ``coords.classify_time_query`` finds to be a field over the HH x WW grid, an ``ops.DecTime``.
        A float32 view already on the device is used through its strides (a broadcast dim costs no memory);
        anything else is copied to the device once."""
        if isinstance(tq, np.ndarray):
            tq = torch.from_numpy(tq)
        if not isinstance(tq, torch.Tensor):
            return self._time_vec(tq, B)
        kind, s3 = classify_time_query(tq.shape, B, HH, WW)
        if kind == "vector":
            return self._time_vec(tq, B)
        v = tq.detach().to(self.device, torch.float32)
        try:
            v = v.view(s3)
        except RuntimeError:   # e.g. [B, HH * WW] rows that are no [HH, WW] view
            v = v.reshape(s3)
        return ops.DecTime.of(v)

    @staticmethod
    def _is_field(tq, B, HH, WW):
        return isinstance(tq, (torch.Tensor, np.ndarray)) and classify_time_query(tq.shape, B, HH, WW)[0] == "field"

    def _tab(self, H, Wd, HH, WW, shift=None):
        key = (str(self.device), H, Wd, HH, WW, shift)
        if key not in self._tables:
            self._tables[key] = ops.DecTablesDev(H, Wd, HH, WW, self.device, shift)
        return self._tables[key]

    def _projection(self, lr_image=True, c0=0, c1=None):
        """LR projections P1..P4 of the current latent's items [c0, c1) (stage 0 of every decoder
        variant)."""
        if self._feat is None:
            raise RuntimeError("decoding needs gen_feat first")
        feats, x = self._feat, self.inp
        _, B, H, Wd, _ = feats.shape
        c1 = B if c1 is None else c1
        f, x, B = feats[:, c0:c1], x[c0:c1], c1 - c0
        src = self._empty(B, H, Wd, 200)
        ops.dec_pack_lr(f[0], f[1], f[2], x, src)
        proj = self._empty(B, H, Wd, 256)
        self._conv([dict(layer=self.layers["dec.proj" if lr_image else "dec.proj_hrimg"], in0=src, out=proj)])
        return proj

    def _decode_steps(self, proj, tvs, HH, WW, tab, outs, image=None):
        """Decoder stages 1-2 of every query time (time vectors ``tvs``) into ``outs`` (generator)."""
        B = proj.shape[0]
        mlp = self.layers["dec.mlp"]
        hrf = self._empty(B, HH, WW, 64)
        flow = self._empty(B, HH, WW, 4)
        for t, out in zip(tvs, outs):
            ops.dec_stage1(proj, mlp, tab, t, hrf, flow, image, flags=self._dec_flags, status=self._status)
            ops.dec_stage2(proj, mlp, hrf, flow, tab, t, out, image, flags=self._dec_flags, status=self._status)
            yield

    def _decode(self, proj, times, HH, WW, tab, image=None):
        B = proj.shape[0]
        outs = [self._empty(B, 3, HH, WW) for _ in times]
        _drain(self._decode_steps(proj, [self._time_vec(tq, B) for tq in times], HH, WW, tab, outs, image))
        return outs

    def decoding(self, times=None, scale=None, window=None, tile=None, ensemble=False):
        """LunaTokis.decoding (:364-459): list over times of [B,3,HH,WW] (unclamped).

        An entry of ``times`` holds 1 or B values, or is a time field: a tensor that broadcasts to [B, HH, WW]
        ([HH, WW], [B, HH, WW], [B, 1, HH, WW], [HH, 1] ..., or the reference's [B, HH * WW];
        ``coords.classify_time_query``), every output pixel then decoded at its own time -- HRfeat and flow of pixel
        q with t(q), the RGB of pixel p from the HRfeat rows at its warped grids and t(p).  With window= / tile=
        the field stays that of the virtual grid.  Not with ensemble=True.

        window=(y0, x0, hh, ww): only that rectangle of the virtual HH x WW grid, [B,3,hh,ww], bit-identical to
        the crop of the full decode and at the cost of the rectangle (``_decode_windowed``).  tile=(th, tw): the
        same output as without it, rendered by windows of at most th x tw, so the decoder scratch is bounded by
        the largest tile's HRfeat rectangle instead of HH * WW.  Either reads a few ints back from the device per
        window and time, so such a call cannot be captured in a hipGraph.

        ensemble=True: the reference's local ensemble (decoding_localensemble, :962-1085) for any batch, window or
        tile -- four decodes with the query shifted by half an LR pixel, blended per HR pixel by the diagonally
        opposite |rel_y rel_x| area (``_decode_ensemble``); bit-identical to ``decoding_localensemble`` item by
        item.  Over the whole grid without tiles it reads nothing back and can be captured."""
        return self._call(self._decoding, times, scale, window, tile, ensemble)

    def _decoding(self, times=None, scale=None, window=None, tile=None, ensemble=False):
        if times is None:
            raise ValueError("times must be a list of query times")
        if self._feat is None:
            raise RuntimeError("decoding needs gen_feat first")
        _, B, H, Wd, _ = self._feat.shape
        HH, WW = _hr_size(H, Wd, scale)
        if ensemble and any(self._is_field(tq, B, HH, WW) for tq in times):
            raise ValueError("a time field is not supported with ensemble=True (the reference's local ensemble "
                             "takes its times as the batch)")
        tab = self._tab(H, Wd, HH, WW)
        tvs = [self._time_query(tq, B, HH, WW) for tq in times]
        if ensemble:
            return self._decode_ensemble(tvs, H, Wd, HH, WW, window, tile)
        if window is not None or tile is not None:
            return self._decode_windowed(tvs, HH, WW, tab, window, tile)
        outs = [self._empty(B, 3, HH, WW) for _ in times]
        # items per decode pass: the LR projections (1 KB per LR pixel) and the HRfeat / flow scratch
        # (272 B per HR pixel) of at most dec_chunk_px HR pixels -- a 63-pair 720p sequence on one GPU
        # would otherwise need ~300 GB of scratch; every pixel is decoded independently, so chunking
        # does not change a bit
        self._decode_passes(B, max(1, self.dec_chunk_px // (HH * WW)), True, lambda proj, a, b: self._decode_steps(
            proj, [t[a:b] for t in tvs], HH, WW, tab, [o[a:b] for o in outs]))
        return outs

    def decoding_pairs(self, pairs, times=None, scale=None, ensemble=False):
        """``decoding`` for the items ``pairs`` (indices into the current latent, in that order) only: list over
        times of [len(pairs),3,HH,WW]; a query time holds one value or one per selected pair.  Items are decoded
        independently, so each output equals that item's slice of a ``decoding`` of the whole latent bit for bit.
        The latent is left as it is (the video stream renderer decodes the pairs of a chunk that share a number
        of query times in one call).  ensemble: as ``decoding``'s."""
        with self._pairs_selected(pairs, whole_as_is=True) as (pairs, idx, B):
            if idx is not None and times is not None and len(pairs) != B:
                # a time field over the latent's B items: its items are selected like the latent's (a field with
                # len(pairs) items, or with none, is taken as it is -- as a vector of len(pairs) values is)
                _, _, H, Wd, _ = self._feat.shape
                HH, WW = _hr_size(H, Wd, scale)

                def select(tq):
                    if not isinstance(tq, (torch.Tensor, np.ndarray)):
                        return tq
                    if int(np.prod(tuple(tq.shape))) in (1, len(pairs)):
                        return tq
                    try:
                        kind, s3 = classify_time_query(tq.shape, B, HH, WW)
                    except ValueError:
                        return tq   # decoding classifies it against the selected items
                    if kind != "field" or s3[0] != B:
                        return tq
                    tq = torch.from_numpy(tq) if isinstance(tq, np.ndarray) else tq
                    return tq.detach().reshape(s3).index_select(0, idx.to(tq.device))
                times = [select(tq) for tq in times]
            return self.decoding(times, scale, ensemble=ensemble)

    @contextlib.contextmanager
    def _pairs_selected(self, pairs, whole_as_is=False):
        """The latent narrowed to its items ``pairs`` while the block runs, then as it was: yields (pairs as checked
        ints, their index tensor, the latent's item count).  whole_as_is: ``pairs`` naming every item in order
        leaves the latent alone (the index tensor is None)."""
        feat, inp = self.__dict__.get("_feat"), self.__dict__.get("inp")
        if feat is None:
            raise RuntimeError("decoding needs gen_feat first")
        pairs = [int(i) for i in pairs]
        B = feat.shape[1]
        if not pairs or min(pairs) < 0 or max(pairs) >= B:
            raise ValueError(f"pairs must be indices into the {B} items of the latent, got {pairs}")
        if whole_as_is and pairs == list(range(B)):
            yield pairs, None, B
            return
        idx = torch.tensor(pairs, device=feat.device, dtype=torch.long)
        self._feat, self.inp = feat.index_select(1, idx), inp.index_select(0, idx)
        try:
            yield pairs, idx, B
        finally:
            self._feat, self.inp = feat, inp

    # ------------------------------------------------------------------ point queries
    def decoding_points(self, y, x, times, scale=None, pairs=None, return_flow=False, ensemble=False):
        """The decode at a set of points: [B, 3, n] float32 on the device, unclamped, in the order given -- point p
        of item b is, bit for bit, ``decoding([t], scale)[0][b, :, y, x]`` with that point's scalar time t.  With
        ``return_flow`` also stage 1's flow [B, 4, n] in HR pixels.

        ``y``, ``x``: integer rows / columns of the virtual HH x WW grid, [n] (the same points for every item) or
        [B, n].  ``times``: a float, [B] (a time per item), [n] (a time per point) or [B, n]; a one-dim tensor of B
        values is [B] also when B == n (``coords.classify_point_query``).  int32 / float32 tensors already on the
        device are read in place through their strides; anything else is copied to the device once.

        Every point is an independent sample of the scalar-time decode: the eight HRfeat rows stage 2 gathers for
        it are computed with the point's own time (in a time field a gathered row carries its own pixel's time).
        Nothing is shared between points, so a point costs about nine feat_imnet evaluations instead of one and a
        dense block of pixels is cheaper as ``decoding(window=)``.  Measured on the C0 latent (six items, 512 x 512
        grid, DESIGN.md section 3e'''): 4,096 points per item take 0.32 ms against 1.95 ms of the full decode, and
        the full decode followed by an index wins above about 90,000 points per item, a third of the grid.

        Host indices (lists, numpy, CPU tensors) are checked before any launch (IndexError).  Device indices are not
        read back: the kernels clamp them into the grid and flag it, the flag is read once after the launches
        (IndexError) -- not while the stream is being captured and not with range_check='off', when valid indices
        are the caller's responsibility (they are still clamped).  ``pairs``: as ``decoding_pairs`` -- only those
        items of the latent, B = len(pairs).

        ``ensemble=True``: the points of the local ensemble instead -- point p of item b is, bit for bit,
        ``decoding([t], scale, ensemble=True)[0][b, :, y, x]`` (``decoding_localensemble``'s pixel).  The four
        shifted decodes run one after the other over the points, each blended into the output by its weight at the
        point (``_ensemble_points``); a point then costs 36 feat_imnet evaluations, four flow and four encode stages.
        Every argument form, the index checks and the capture rule are those above; ``return_flow`` is a ValueError
        (there are four flows and none of them is the flow).  Measured on the C0 latent (six items, 512 x 512 grid,
        DESIGN.md section 3e'''): 4,096 points per item take 0.738 ms (0.732 .. 0.756) against 7.752 ms
        (7.677 .. 7.959) of the full ensemble decode followed by an index, 65,536 take 5.822 (5.693 .. 5.975)
        against 7.865 (7.781 .. 7.950), and the full ensemble decode wins above about 90,000 points per item, a
        third of the grid (7.198 against 7.873 ms at 81,920, 8.481 against 7.703 at 98,304)."""
        if ensemble and return_flow:
            raise ValueError("decoding_points: return_flow has no meaning with ensemble=True (the local ensemble has "
                             "four flows per point)")
        if pairs is None:
            return self._call(self._decoding_points, y, x, times, scale, return_flow, ensemble)
        with self._pairs_selected(pairs):
            return self._call(self._decoding_points, y, x, times, scale, return_flow, ensemble)

    def _point_list(self, y, x, times, B, HH, WW):
        """The arguments of ``decoding_points`` as an ``ops.DecPoints`` over B items."""
        def host(v):   # the host array of anything that is not on the device, else None
            if isinstance(v, torch.Tensor):
                return None if v.is_cuda else v.detach().numpy()
            return np.asarray(v)

        if not isinstance(times, (torch.Tensor, np.ndarray)):
            times = np.asarray(times, dtype=np.float32)
        n, ys, xs, ts = classify_point_query(tuple(y.shape) if hasattr(y, "shape") else np.shape(y),
                                             tuple(x.shape) if hasattr(x, "shape") else np.shape(x),
                                             tuple(times.shape), B)
        hy, hx = host(y), host(x)
        check_points(hy if hy is not None else (), hx if hx is not None else (), HH, WW)

        def coord(v, hv, s2):
            if hv is not None:
                v = torch.from_numpy(np.ascontiguousarray(hv, dtype=np.int32))
            elif v.is_floating_point() or v.dtype == torch.bool:
                raise TypeError("decoding_points: y and x must be integers")
            v = v.detach().to(self.device, torch.int32).reshape(s2)
            if n > 1 and v.stride(1) != 1:
                v = v.contiguous()
            return v

        yt, xt = coord(y, hy, ys), coord(x, hx, xs)
        tt = (torch.from_numpy(times) if isinstance(times, np.ndarray) else times.detach())
        tt = tt.to(self.device, torch.float32).reshape(ts)
        (yi, _), (xi, _), (ti, tp) = (point_strides(s, v.stride()) for s, v in ((ys, yt), (xs, xt), (ts, tt)))
        return ops.DecPoints(yt, xt, tt, yi, xi, ti, tp, n, B)

    def _ensemble_points(self, proj, mlp, tabs, blends, sub, o, fl, st):
        """The local ensemble at the points ``sub`` of the items of ``proj`` into ``o`` ([k, 3, m]): per shift, in
        ops.ENSEMBLE_BLEND_ORDER on one stream -- the remapped pixel of every point (``ops.dec_remap_pts``), feat_imnet
        of the shifted query there (the flow stage's HRfeat operand), the flow, its eight corner pixels and their
        HRfeat as in the plain path but with the shifted tables, and stage 2 blending w_k rgb into ``o`` (the first
        stores, the others accumulate).  One shift's scratch is alive at a time."""
        k, m = o.shape[0], sub.npts
        ints = lambda *shape: torch.empty(*shape, device=self.device, dtype=torch.int32)
        for s in ops.ENSEMBLE_BLEND_ORDER:
            tab = tabs[s]
            remapped = ops.dec_remap_pts(tab, sub, k, ints(k, m), ints(k, m), status=st)
            hrf = self._empty(k, m, 64)
            ops.dec_stage1_pts(proj, mlp, tab.plain, remapped, hrf, None, flags=fl, status=st)
            flow = self._empty(k, m, 4)
            ops.dec_flow_pts(proj, mlp, tab, sub, hrf, flow, flags=fl, status=st)
            del hrf, remapped
            corners = ops.dec_corners_pts(flow, tab.plain, sub, ints(k, 8 * m), ints(k, 8 * m), self._empty(k, 8 * m),
                                          status=st)
            hrf8 = self._empty(k, 8 * m, 64)
            ops.dec_stage1_pts(proj, mlp, tab.plain, corners, hrf8, None, flags=fl, status=st)
            ops.dec_stage2_blend_pts(proj, mlp, hrf8, flow, tab, sub, o, blends[s], flags=fl, status=st)
            del hrf8, corners, flow

    def _decoding_points(self, y, x, times, scale=None, return_flow=False, ensemble=False):
        if self._feat is None:
            raise RuntimeError("decoding needs gen_feat first")
        _, B, H, Wd, _ = self._feat.shape
        HH, WW = _hr_size(H, Wd, scale)
        pts = self._point_list(y, x, times, B, HH, WW)
        n = pts.npts
        tab = self._tab(H, Wd, HH, WW)
        mlp, fl, st = self.layers["dec.mlp"], self._dec_flags, self._status
        if st is not None and fl == 0:
            st.zero_()   # fp32 operands: only the points' bit 3 is read below
        out = self._empty(B, 3, n)
        flw = self._empty(B, n, 4) if return_flow else None
        # items and points per pass: 8 corner rows of HRfeat per point, at most dec_chunk_px rows per pass -- the
        # scratch bound of the whole-grid decode; points are decoded independently, so chunking changes no bit
        per, ranges = point_passes(B, n, self.dec_chunk_px)
        whole = len(ranges) == 1
        if ensemble:
            tabs = [self._tab(H, Wd, HH, WW, s) for s in ops.ENSEMBLE_SHIFTS]
            blends = {k: ops.dec_blend(k, tabs, accumulate=i > 0) for i, k in enumerate(ops.ENSEMBLE_BLEND_ORDER)}

        def body(proj, a, b):
            k = b - a
            for p0, p1 in ranges:
                m = p1 - p0
                sub = pts.sub(a, b, p0, p1)
                if ensemble:
                    # the range's buffer lives across its four shifts before it is copied into place
                    o = out[a:b] if whole else self._empty(k, 3, m)
                    self._ensemble_points(proj, mlp, tabs, blends, sub, o, fl, st)
                    if not whole:
                        out[a:b, :, p0:p1].copy_(o)
                    del o
                    yield
                    continue
                hrf = self._empty(k, m, 64)
                flow = flw[a:b] if whole and return_flow else self._empty(k, m, 4)
                ops.dec_stage1_pts(proj, mlp, tab, sub, hrf, flow, flags=fl, status=st)
                del hrf   # the point's own HRfeat row: stage 2 reads the corner rows only
                cy, cx = (torch.empty(k, 8 * m, device=self.device, dtype=torch.int32) for _ in range(2))
                corners = ops.dec_corners_pts(flow, tab, sub, cy, cx, self._empty(k, 8 * m), status=st)
                hrf8 = self._empty(k, 8 * m, 64)
                ops.dec_stage1_pts(proj, mlp, tab, corners, hrf8, None, flags=fl, status=st)
                o = out[a:b] if whole else self._empty(k, 3, m)
                ops.dec_stage2_pts(proj, mlp, hrf8, flow, tab, sub, o, flags=fl, status=st)
                if not whole:
                    out[a:b, :, p0:p1].copy_(o)
                    if return_flow:
                        flw[a:b, p0:p1].copy_(flow)
                del hrf8, corners, cy, cx, flow, o
                yield
        self._decode_passes(B, per, True, body)
        if st is not None and not torch.cuda.is_current_stream_capturing() and int(st.item()) & 8:
            raise IndexError(f"decoding_points: a point lies outside the {HH} x {WW} grid")
        return (out, flw.permute(0, 2, 1).contiguous()) if return_flow else out

    def _decode_passes(self, B, per, lr_image, body):
        """The items [0, B) over the ``dec`` lanes, in passes of ``per``: the LR projection of a pass's items
        [a, b), then ``body(proj, a, b)`` (a generator issuing their decode), then the projection is dropped."""
        def lane(c0, c1):
            for a in range(c0, c1, per):
                b = min(c1, a + per)
                proj = self._projection(lr_image, a, b)
                yield
                yield from body(proj, a, b)
                del proj
        self._run_lanes(B, lane, self.dec_lanes, pool="dec")

    def decoding_test(self, times=None, scale=None, window=None, tile=None):
        """LunaTokis.decoding_test (:461-598), what forward(test=True) returns: the flow and encode
        stages sample HRinp = F.upsample(inp, x4, bilinear) instead of the LR frames; HH = H * scale
        (integer scale, default 4).  The reference's q/3 chunking only bounds its memory.
        window / tile: as ``decoding``."""
        return self._call(self._decoding_test, times, scale, window, tile)

    def _decoding_test(self, times=None, scale=None, window=None, tile=None):
        if times is None:
            raise ValueError("times must be a list of query times")
        if self._feat is None:
            raise RuntimeError("decoding needs gen_feat first")
        _, B, H, Wd, _ = self._feat.shape
        s = 4 if scale is None else int(scale)
        HH, WW = H * s, Wd * s
        if any(self._is_field(tq, B, HH, WW) for tq in times):
            raise ValueError("a time field is not supported in decoding_test (high-resolution image)")
        windowed = window is not None or tile is not None
        proj = None if windowed else self._projection(lr_image=False)   # a windowed decode projects per pass
        image = ops.DecImageDev(self.inp, 4, HH, WW)
        tab = self._tab(H, Wd, HH, WW)
        if windowed:
            return self._decode_windowed([self._time_vec(tq, B) for tq in times], HH, WW, tab, window, tile, image)
        return self._decode(proj, times, HH, WW, tab, image)

    # ------------------------------------------------------------------ windowed decoding
    def _window_F(self, flow, tab, box, win, base):
        """The HRfeat rectangle F of a window: the bounding box of the HRfeat rows / columns stage 2 will gather
        given stage 1's ``flow``, read back from the device, united with ``base``."""
        ops.dec_bounds(flow, tab, box, win)
        ymin, ymax, xmin, xmax = box.tolist()   # the device-to-host read (synchronises this stream)
        fy0, fx0 = min(ymin, base[0]), min(xmin, base[1])
        return fy0, fx0, max(ymax + 1, base[0] + base[2]) - fy0, max(xmax + 1, base[1] + base[3]) - fx0

    def _stage2_given_F(self, proj, mlp, tab, feat_tab, t, hrf, flow, out, rect, frect, per, kw, image=None,
                        blend=None):
        """Stage 2 over the window ``rect`` into ``out`` with HRfeat over ``frect``.  ``hrf``: that HRfeat where
        stage 1 left it over all of F; None where F is larger -- the caller has dropped its buffer, which the caching
        allocator reuses for the F buffer (same stream) -- and HRfeat over F then comes from a feat-only stage 1
        with ``feat_tab``, ``per`` items a pass.  kw: the stages' flags and status."""
        HH, WW = tab.shape[2:]
        wf = ops.dec_window(rect, HH, WW, frect)
        if hrf is not None:
            ops.dec_stage2(proj, mlp, hrf, flow, tab, t, out, image, window=wf, blend=blend, **kw)
            return
        n = proj.shape[0]
        for a in range(0, n, per):
            b = min(n, a + per)
            img = image.items(a, b) if image is not None else None
            hf = self._empty(b - a, frect[2], frect[3], 64)
            ops.dec_stage1(proj[a:b], mlp, feat_tab, t[a:b], hf, None, img, window=ops.dec_window(frect, HH, WW), **kw)
            ops.dec_stage2(proj[a:b], mlp, hf, flow[a:b], tab, t[a:b], out[a:b], img, window=wf, blend=blend, **kw)
            del hf

    def _window_steps(self, proj, tvs, HH, WW, tab, outs, rect, image=None):
        """Decoder stages of every query time for the window ``rect`` into ``outs`` ([n,3,hh,ww] views; generator).
        Per time: stage 1 (HRfeat + flow) over the window W; F = box U W (``_window_F``); if F is larger than W,
        HRfeat over F by a feat-only stage 1 (recomputing W's part: two launches with one layout beat a scatter of
        W's rows into F, and W is the smaller part whenever the flows matter); stage 2 over W.  The F passes take at
        most dec_chunk_px // |F| items each."""
        n = proj.shape[0]
        _, _, hh, ww = rect
        mlp, kw = self.layers["dec.mlp"], dict(flags=self._dec_flags, status=self._status)
        win = ops.dec_window(rect, HH, WW)
        box = torch.empty(4, device=self.device, dtype=torch.int32)
        for t, out in zip(tvs, outs):
            hrf = self._empty(n, hh, ww, 64)
            flow = self._empty(n, hh, ww, 4)
            ops.dec_stage1(proj, mlp, tab, t, hrf, flow, image, window=win, **kw)
            frect = self._window_F(flow, tab, box, win, rect)
            per = max(1, self.dec_chunk_px // (frect[2] * frect[3]))
            self.last_window_F = frect
            self.window_peak_scratch_bytes = max(self.window_peak_scratch_bytes,
                                                 min(n, per) * frect[2] * frect[3] * 272)
            if frect != rect:
                hrf = None
            self._stage2_given_F(proj, mlp, tab, tab, t, hrf, flow, out, rect, frect, per, kw, image)
            yield

    def _decode_tiles(self, tvs, B, region, rects, steps, lr_image, bits, failure):
        """The windows ``rects`` of ``region``, each written in place into the outputs ([B,3,rh,rw] per entry of
        ``tvs``) through its strides by ``steps(proj, tvs of the items, views, rect, a, b)`` for the items [a, b) of a
        pass.  bits: the status bits that say a gather left its HRfeat rectangle, read back after the launches and
        raised as ``failure`` (0: nothing is read back).  Starts ``last_window_F`` / ``window_peak_scratch_bytes``."""
        ry, rx, rh, rw = region
        outs = [self._empty(B, 3, rh, rw) for _ in tvs]
        self.last_window_F, self.window_peak_scratch_bytes = None, 0
        st = self._status if bits else None
        if st is not None and self._dec_flags == 0:
            st.zero_()   # fp32 operands: only the windows' bits are read below
        per = max(1, self.dec_chunk_px // max(r[2] * r[3] for r in rects))

        def tiles(proj, a, b):
            for r in rects:
                views = [o[a:b, :, r[0] - ry:r[0] - ry + r[2], r[1] - rx:r[1] - rx + r[3]] for o in outs]
                yield from steps(proj, [t[a:b] for t in tvs], views, r, a, b)
        self._decode_passes(B, per, lr_image, tiles)
        if st is not None and int(st.item()) & bits:
            raise L.StifError(failure)
        return outs

    def _decode_windowed(self, tvs, HH, WW, tab, window, tile, image=None):
        """``decoding`` / ``decoding_test`` (image given) over ``window`` (None: the whole grid), rendered by
        tiles of at most ``tile`` (None: one).  Every tile is a window written in place into the output through
        its strides.  ``last_window_F`` is the HRfeat rectangle (fy0, fx0, fh, fw) of the last window decoded and
        ``window_peak_scratch_bytes`` the largest per-pass HRfeat + flow scratch of the call (items x |F| x 272 B)."""
        if torch.cuda.is_current_stream_capturing():
            raise L.StifError(_NO_CAPTURE)
        B = self._feat.shape[1]   # every entry of tvs holds (or, a field without item stride, serves) B items
        region = check_window((0, 0, HH, WW) if window is None else window, HH, WW)

        def steps(proj, ts, views, r, a, b):
            img = image.items(a, b) if image is not None else None
            return self._window_steps(proj, ts, HH, WW, tab, views, r, img)
        return self._decode_tiles(
            tvs, B, region, [region] if tile is None else tile_windows(region, tile), steps, image is None, 2,
            "windowed decode: stage 2 gathered outside its HRfeat rectangle (stif_dec_bounds and stage 2 disagree): "
            "the result is wrong")

    # ------------------------------------------------------------------ local ensemble over windows
    def _ensemble_steps(self, proj, tvs, HH, WW, tabs, outs, rect):
        """The local ensemble of every query time for the window ``rect`` into ``outs`` ([n,3,hh,ww] views;
        generator).  Per time and per shift k (``tabs``: the four shifted tables in the reference's order): HRfeat
        of the shifted query over the remap rectangle R_k, which the host knows from the monotone hr_y / hr_x tables;
        the flow over W with its HRfeat operand read at (hr_y, hr_x) from R_k; F = box U R_k (``_window_F``), and
        HRfeat over F if that is larger than R_k; stage 2 over W, blending w_k rgb into ``out`` in place (the first
        stores, the others accumulate -- the four launches of a window follow each other on one stream, in
        ops.ENSEMBLE_BLEND_ORDER, the order that gives stif_dec_blend4's roundings).  One shift's HRfeat and flow
        are alive at a time.  A window that is the whole grid takes F = the whole grid and reads nothing back."""
        n = proj.shape[0]
        _, _, hh, ww = rect
        whole = rect == (0, 0, HH, WW)
        mlp, kw = self.layers["dec.mlp"], dict(flags=self._dec_flags, status=self._status)
        win = ops.dec_window(rect, HH, WW)
        blends ={k: ops.dec_blend(k, tabs, accumulate=i > 0) for i, k in enumerate(ops.ENSEMBLE_BLEND_ORDER)}
        box = None if whole else torch.empty(4, device=self.device, dtype=torch.int32)
        for t, out in zip(tvs, outs):
            largest = None
            for k in ops.ENSEMBLE_BLEND_ORDER:
                tab = tabs[k]
                rrect = rect if whole else tab.remap_rect(rect)
                flow = self._empty(n, hh, ww, 4)
                hrf = self._empty(n, rrect[2], rrect[3], 64)   # feat_imnet at the shifted query over R_k
                ops.dec_stage1(proj, mlp, tab.plain, t, hrf, None, window=ops.dec_window(rrect, HH, WW), **kw)
                ops.dec_flow_win(proj, mlp, tab, t, hrf, flow, window=ops.dec_window(rect, HH, WW, rrect), **kw)
                frect = rrect if whole else self._window_F(flow, tab, box, win, rrect)
                per = max(1, self.dec_chunk_px // (frect[2] * frect[3]))
                if largest is None or frect[2] * frect[3] > largest[2] * largest[3]:
                    largest = frect
                self.window_peak_scratch_bytes = max(
                    self.window_peak_scratch_bytes, n * (rrect[2] * rrect[3] * 256 + hh * ww * 16),
                    min(n, per) * frect[2] * frect[3] * 256 + n * hh * ww * 16)
                if frect != rrect:
                    hrf = None
                self._stage2_given_F(proj, mlp, tab, tab.plain, t, hrf, flow, out, rect, frect, per, kw,
                                     blend=blends[k])
                del hrf, flow
            self.last_window_F = largest
            yield

    def _decode_ensemble(self, tvs, H, Wd, HH, WW, window, tile):
        """``decoding(ensemble=True)`` over ``window`` (None: the whole grid) by tiles of at most ``tile`` (None:
        one), each a window blended in place into the output through its strides (``_ensemble_steps``).
        ``last_window_F`` is the largest HRfeat rectangle of the four shifts of the last window decoded and
        ``window_peak_scratch_bytes`` the largest HRfeat + flow scratch alive in the call (one shift's)."""
        B = tvs[0].shape[0] if tvs else self._feat.shape[1]
        region = check_window((0, 0, HH, WW) if window is None else window, HH, WW)
        rects = [region] if tile is None else tile_windows(region, tile)
        # with F the whole grid no index can leave it: nothing to read back, and the call may be being captured
        whole = rects == [(0, 0, HH, WW)]
        if not whole and torch.cuda.is_current_stream_capturing():
            raise L.StifError(_NO_CAPTURE)
        tabs = [self._tab(H, Wd, HH, WW, s) for s in ops.ENSEMBLE_SHIFTS]
        return self._decode_tiles(
            tvs, B, region, rects,
            lambda proj, ts, views, r, a, b: self._ensemble_steps(proj, ts, HH, WW, tabs, views, r), True,
            0 if whole else 6,
            "windowed ensemble decode: a gather left its HRfeat rectangle (the remap rectangle or stif_dec_bounds "
            "disagrees with the kernels): the result is wrong")

    def decoding_window(self, times=None, scale=None, center=(0.0, 0.0), size=None):
        """The reference's zoom call (decoding_memory, Sakuya_arch_test.py:600-861): the ``size`` (default 4H x 4W)
        rectangle of the virtual ``scale`` grid around ``center`` = (row, col) in [-1, 1]^2, placed by
        ``coords.window_from_center`` -- the reference's rectangle arithmetic (:639-652).  The pixels are defined
        as that crop of ``decoding``; the reference's decoding_memory builds its warp base from make_coord
        (``warpgrid2``) instead of torch.linspace, i.e. it evaluates a slightly different function, which this
        call does not reproduce."""
        if self._feat is None:
            raise RuntimeError("decoding needs gen_feat first")
        _, _, H, Wd, _ = self._feat.shape
        HH, WW = _hr_size(H, Wd, scale)
        size = (4 * H, 4 * Wd) if size is None else size
        return self.decoding(times, scale, window=window_from_center(center, HH, WW, size))

    @staticmethod
    def _no_fields(times, where):
        for tq in times or ():
            if isinstance(tq, (torch.Tensor, np.ndarray)) and int(np.prod(tuple(tq.shape))) > 1:
                raise ValueError(f"a time field is not supported in {where}: its times are floats, decoded as the batch")

    def decoding_fasttest(self, times=None, scale=None):
        """LunaTokis.decoding_fasttest (:863-960): `times` is a list of floats, the latent a batch of
        one; all times come back as one batch [len(times), 3, HH, WW]."""
        return self._call(self._decoding_fasttest, times, scale)

    def _decoding_fasttest(self, times=None, scale=None):
        if self._feat is None:
            raise RuntimeError("decoding needs gen_feat first")
        if self._feat.shape[1] != 1:
            raise ValueError("decoding_fasttest batches the query times: the latent must have batch 1")
        self._no_fields(times, "decoding_fasttest")
        tq = [torch.tensor([[float(t)]]) for t in times]
        return torch.cat(self._decoding(tq, scale), 0)

    def decoding_localensemble(self, times=None, scale=None):
        """LunaTokis.decoding_localensemble (:962-1085): four decodes with the query shifted by
        (+-1/H, +-1/W), blended per HR pixel by the diagonally opposite |rel_y rel_x| area; batch-1
        latent, `times` a list of floats -> [len(times), 3, HH, WW]."""
        return self._call(self._decoding_localensemble, times, scale)

    def _decoding_localensemble(self, times=None, scale=None):
        if self._feat is None:
            raise RuntimeError("decoding needs gen_feat first")
        if self._feat.shape[1] != 1:
            raise ValueError("decoding_localensemble batches the query times: the latent must have batch 1")
        self._no_fields(times, "decoding_localensemble")
        proj = self._projection()
        _, H, Wd, _ = proj.shape
        HH, WW = _hr_size(H, Wd, scale)
        key = ("ens", str(self.device), H, Wd, HH, WW)
        if key not in self._tables:
            self._tables[key] = [torch.from_numpy(a).to(self.device) for a in ensemble_weights(H, Wd, HH, WW)]
        wts = self._tables[key]
        tq = [torch.tensor([[float(t)]]) for t in times]
        decs = [torch.cat(self._decode(proj, tq, HH, WW, self._tab(H, Wd, HH, WW, (vx, vy))), 0)
                for vx in (-1, 1) for vy in (-1, 1)]
        out = self._empty(len(times), 3, HH, WW)
        ops.dec_blend4(decs, wts, out)
        return out

    def forward(self, x, times=None, scale=None, test=False, center=None, index=0):
        """LunaTokis.forward (:1222-1231): decoding, or decoding_test with test=True."""
        return self._call(self._forward, x, times, scale, test)

    def _forward(self, x, times, scale, test):
        self._gen_feat(x)
        if test:
            return self._decoding_test(times, scale)
        return self._decoding(times, scale)
