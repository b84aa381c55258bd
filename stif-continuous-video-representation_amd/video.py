"""custom_video_test-style driver (codes/custom_video_test.py:41-110) on the engine.

``single_forward`` keeps the harness's behaviour: zero-pad H, W up to a multiple
of 4 on the bottom/right (:44-48), query the eight times i/8 (:50), return the
uncropped [1,3,4h_n,4w_n] outputs.  ``run_sequence`` is the harness's pair loop
(:81-97) as one batched window: every adjacent pair of a frame sequence, with the
per-frame encoder shared between the two pairs that use a frame.

The harness's data formats either side of the model run on the GPU too:
``resize_frames`` = ``data.util.imresize_np(frame, 1/2, True)`` on cv2-style uint8 BGR frames
+ ``/255`` + BGR->RGB + NCHW (:88-93), ``frames_to_u8`` = ``(clamp(0,1)*255).astype(uint8)`` HWC
(:101-102); ``run_folder`` is the whole script (LR / HR / bicubic outputs, PIL file I/O).

``evaluate_sequence`` / ``evaluate_folder`` add the reference's evaluation loop (myutils.py:1151-1174):
run_sequence, then PSNR / SSIM of every output frame that has a ground truth, scored on the device
(stif_amd.metrics), and the "AVG PSNR / AVG SSIM" means; ``metric="float"`` scores with the float protocol of
myutils.eval_metrics (:234-241: calc_psnr beside ssim_matlab) instead of the quantised one.

``frame_schedule`` / ``render_stream`` / ``render_y4m`` render whole videos: any length in bounded memory (frames
are taken a chunk at a time, each encoded once), any rational output frame rate (every pair gets its own query
times), raw YUV4MPEG2 in and out (stif_amd.y4m, ops.yuv_to_rgb / rgb_to_yuv).  They compose gen_feat_window and
decoding; the harness functions above keep the reference's behaviour, truncating quantisation included.
Optionally they detect scene cuts on the device (ops.scene_sad, ``scene_scores``) or take them from the caller,
and repeat a real frame across a cut instead of interpolating between two unrelated pictures.
"""
from __future__ import annotations

import ctypes as C
import math
import os

import numpy as np
import torch

from . import _lib as L

HARNESS_TIMES = [i / 8 for i in range(8)]


def pad_to_4(imgs: torch.Tensor) -> torch.Tensor:
    """imgs [..., h, w] -> zero-padded to multiples of 4 (custom_video_test.py:44-48)."""
    h, w = imgs.shape[-2:]
    hn, wn = int(4 * math.ceil(h / 4)), int(4 * math.ceil(w / 4))
    if (hn, wn) == (h, w):
        return imgs
    out = imgs.new_zeros(*imgs.shape[:-2], hn, wn)
    out[..., :h, :w] = imgs
    return out


def single_forward(model, imgs_in: torch.Tensor, times=None):
    """imgs_in [1,2,3,h,w] RGB in [0,1] -> list over times of [1,3,4h_n,4w_n]."""
    with torch.no_grad():
        x = pad_to_4(imgs_in)
        ts = HARNESS_TIMES if times is None else times
        return model(x, [torch.tensor([t])[None] for t in ts])


def run_sequence(model, frames: torch.Tensor, times=None, scale=None, window=None, ensemble=False):
    """frames [F,3,h,w] -> list over the F-1 pairs of lists over times of [3,HH,WW]; window=(y0, x0, hh, ww):
    only that rectangle of every output frame, [3,hh,ww] (LunaTokis.decoding's window); ensemble: every frame
    decoded with the local ensemble (LunaTokis.decoding's ensemble).  A tensor entry of ``times`` is passed to
    ``decoding`` as it is -- e.g. a time field ([HH, WW], [HH, 1], ...: every pixel of every pair at its own time)."""
    with torch.no_grad():
        fr = pad_to_4(frames)
        model.gen_feat_window(fr)
        ts = HARNESS_TIMES if times is None else times
        kw = {} if window is None else {"window": window}
        if ensemble:
            kw["ensemble"] = True
        preds = model.decoding([t if isinstance(t, torch.Tensor) else torch.tensor([t])[None] for t in ts], scale, **kw)
    return [[p[i] for p in preds] for i in range(frames.shape[0] - 1)]


# ----------------------------------------------------------------------------- harness I/O
F32 = np.float32


def _cubic(x):
    ax = np.abs(x).astype(F32)
    ax2 = (ax * ax).astype(F32)
    ax3 = (ax2 * ax).astype(F32)
    a = ((F32(1.5) * ax3 - F32(2.5) * ax2 + F32(1)) * (ax <= 1)).astype(F32)
    b = ((F32(-0.5) * ax3 + F32(2.5) * ax2 - F32(4) * ax + F32(2)) * ((ax > 1) & (ax <= 2))).astype(F32)
    return (a + b).astype(F32)


def resize_tables(in_len: int, out_len: int, scale: float, antialias: bool = True):
    """calculate_weights_indices (data/util.py:248-300) in fp32 -> (weights [out, P], first
    symmetric-padded index per output [out], top/left padding sym_len_s)."""
    kw = 4.0 / scale if (scale < 1 and antialias) else 4.0
    x = np.linspace(1, out_len, out_len, dtype=np.float64).astype(F32)
    u = (x / F32(scale) + F32(0.5 * (1 - 1 / scale))).astype(F32)
    left = np.floor(u - F32(kw / 2)).astype(F32)
    P = int(math.ceil(kw)) + 2
    ind = (left[:, None] + np.arange(P, dtype=F32)[None, :]).astype(F32)
    dist = (u[:, None] - ind).astype(F32)
    w = (F32(scale) * _cubic((dist * F32(scale)).astype(F32))).astype(F32) if (scale < 1 and antialias) else _cubic(dist)
    w = (w / w.sum(1, dtype=F32)[:, None]).astype(F32)
    zeros = (w == 0).sum(0)                     # counted before either narrow (:286-291)
    if zeros[0] != 0:
        ind, w = ind[:, 1:P - 1], w[:, 1:P - 1]
    if zeros[-1] != 0:
        ind, w = ind[:, :P - 2], w[:, :P - 2]
    s0 = int(-ind.min() + 1)
    return np.ascontiguousarray(w, F32), (ind[:, 0] + s0 - 1).astype(np.int32), s0


_RESIZE_CACHE = {}


def resize_frames(frames_bgr_u8, scale: float = 0.5, device="cuda") -> torch.Tensor:
    """imresize_np(frame, scale, True).astype(float32) / 255, BGR -> RGB, HWC -> CHW for a stack of
    cv2-style uint8 BGR frames [n, H, W, 3] (numpy or torch) -> device float [n, 3, oH, oW]."""
    fr = torch.as_tensor(frames_bgr_u8).to(device=device, dtype=torch.uint8).contiguous()
    n, H, W, c = fr.shape
    if c != 3:
        raise ValueError("frames must be [n, H, W, 3] uint8 (BGR, as cv2.imread)")
    oH, oW = int(math.ceil(H * scale)), int(math.ceil(W * scale))
    key = (H, W, scale, str(device))
    if key not in _RESIZE_CACHE:
        wH, iH, sH = resize_tables(H, oH, scale)
        wW, iW, sW = resize_tables(W, oW, scale)
        dev = [torch.from_numpy(a).to(device) for a in (wH, iH, wW, iW)]
        _RESIZE_CACHE[key] = (dev, wH.shape[1], sH, wW.shape[1], sW)
    (twH, tiH, twW, tiW), PH, sH, PW, sW = _RESIZE_CACHE[key]
    out = torch.empty(n, 3, oH, oW, device=device, dtype=torch.float32)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    L.check(L.lib().stif_resize_frames(fr.data_ptr(), out.data_ptr(), n, H, W, oH, oW, twH.data_ptr(), tiH.data_ptr(),
                                       PH, sH, twW.data_ptr(), tiW.data_ptr(), PW, sW, st), "stif_resize_frames")
    return out


def frames_to_u8(frames: torch.Tensor) -> torch.Tensor:
    """(clamp(frames, 0, 1) * 255).astype(uint8), NCHW float -> HWC uint8 [n, H, W, 3] on the device."""
    f = frames.contiguous()
    n, c, H, W = f.shape
    if c != 3:
        raise ValueError("frames must be [n, 3, H, W]")
    out = torch.empty(n, H, W, 3, device=f.device, dtype=torch.uint8)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    L.check(L.lib().stif_frames_to_u8(f.data_ptr(), out.data_ptr(), n, H, W, st), "stif_frames_to_u8")
    return out


def run_folder(model, in_dir: str, out_dir: str, times=None):
    """custom_video_test.py:60-110 for one folder of frames: every adjacent pair is resized by 1/2
    (imresize_np), run at the eight harness times, and written as JPGs under out_dir/HR; the LR
    frames go to out_dir/LR and the PIL-bicubic x4 baseline to out_dir/bicubic.  Frames are read with
    PIL and flipped to BGR so the data path matches cv2.imread's."""
    from PIL import Image

    names = sorted(os.listdir(in_dir))
    for sub in ("HR", "bicubic", "LR"):
        os.makedirs(os.path.join(out_dir, sub), exist_ok=True)
    idx_hr = idx_bic = 0
    for i in range(len(names) - 1):
        bgr = np.stack([np.asarray(Image.open(os.path.join(in_dir, names[i + k])).convert("RGB"))[:, :, ::-1]
                        for k in range(2)])
        lr = resize_frames(bgr)                                           # [2,3,h,w] RGB
        lr_u8 = frames_to_u8(lr).cpu().numpy()
        Image.fromarray(lr_u8[0]).save(os.path.join(out_dir, "LR", names[i]))
        outs = single_forward(model, lr[None], times)
        hr = frames_to_u8(torch.cat(outs, 0)).cpu().numpy()
        for k in range(hr.shape[0]):
            Image.fromarray(hr[k]).save(os.path.join(out_dir, "HR", f"{idx_hr}.jpg"))
            idx_hr += 1
        h, w = lr_u8.shape[1:3]
        for _ in range(len(outs)):
            Image.fromarray(lr_u8[0]).resize((4 * w, 4 * h), Image.BICUBIC).save(
                os.path.join(out_dir, "bicubic", f"{idx_bic}.jpg"))
            idx_bic += 1


# ----------------------------------------------------------------------------- evaluation
def _gt_float_planes(g: torch.Tensor, device) -> torch.Tensor:
    """The float protocol's ground truth [3, H, W] on the device: a float tensor is taken as RGB planes; uint8 BGR
    [H, W, 3] becomes RGB planes / 255 in fp32 (a 256-entry table of the correctly rounded quotients, gathered on
    the device)."""
    if g.is_floating_point():
        if g.dim() != 3 or g.shape[0] != 3:
            raise ValueError(f"a float ground truth must be RGB planes [3, H, W]; got {tuple(g.shape)}")
        return g.to(device)
    if g.dtype != torch.uint8 or g.dim() != 3 or g.shape[2] != 3:
        raise ValueError(f"gt must be uint8 BGR [H, W, 3] or float RGB [3, H, W]; got {g.dtype} {tuple(g.shape)}")
    lut = torch.from_numpy(np.arange(256, dtype=np.float32) / np.float32(255.0)).to(device)
    return lut[g.to(device).flip(2).permute(2, 0, 1).contiguous().long()]


def evaluate_sequence(model, frames: torch.Tensor, gt, times=None, scale=None, channels: str = "y",
                      metric: str = "quantised", ensemble=False):
    """run_sequence + the reference's scoring loop (myutils.py:1155-1174) on the device.  gt[pair][time] is the
    ground truth of that output frame, uint8 BGR [H, W, 3] (numpy or torch, as cv2.imread), or None to skip it.
    When pad_to_4 padded the input the outputs are larger than the ground truth: the top-left H x W crop of the
    output is scored in place, through the metric's stride arguments.  metric="float" scores with
    myutils.eval_metrics instead (metrics.eval_metrics: calc_psnr and ssim_matlab on the unquantised floats;
    `channels` does not apply); there a ground truth may also be a float RGB [3, H, W] tensor, and must be at
    least 11 x 11.  Returns {"psnr", "ssim": lists over pairs of lists over times (None where skipped),
    "avg_psnr", "avg_ssim": means over the scored frames (the reference's "AVG PSNR / AVG SSIM"), "count"}.
    ensemble: the frames scored are the local ensemble's (run_sequence)."""
    from . import metrics as M
    if metric not in ("quantised", "float"):
        raise ValueError('metric must be "quantised" or "float"')
    fl = metric == "float"
    outs = run_sequence(model, frames, times, scale, ensemble=ensemble)
    flags = M.mode_flags(channels, True)
    where, sums = [], []
    for i, row in enumerate(outs):
        for k, o in enumerate(row):
            g = gt[i][k] if i < len(gt) and k < len(gt[i]) else None
            if g is None:
                continue
            g = torch.as_tensor(np.ascontiguousarray(g) if isinstance(g, np.ndarray) else g)
            if fl:
                g = _gt_float_planes(g, o.device)
            H, W = g.shape[1:] if fl else g.shape[:2]
            if H > o.shape[1] or W > o.shape[2]:
                raise ValueError(f"gt[{i}][{k}] is {H}x{W}, larger than the {o.shape[1]}x{o.shape[2]} output")
            crop = o[None, :, :H, :W]
            sums.append(M.sums_float(crop, g[None]) if fl else M.sums(crop, g[None], flags))
            where.append((i, k))
    psnr = [[None] * len(row) for row in outs]
    ssim = [[None] * len(row) for row in outs]
    if sums:
        p, s = M.finish(torch.cat(sums, 0).cpu().numpy(), float_mode=fl)     # one read-back for the whole sequence
        for (i, k), pv, sv in zip(where, p, s):
            psnr[i][k], ssim[i][k] = float(pv), float(sv)
    n = len(where)
    return {"psnr": psnr, "ssim": ssim, "count": n,
            "avg_psnr": float(np.mean(p)) if n else float("nan"),
            "avg_ssim": float(np.mean(s)) if n else float("nan")}


def _frame_key(name: str):
    stem = os.path.splitext(name)[0]
    return (0, int(stem), name) if stem.isdigit() else (1, 0, name)


def evaluate_folder(model, lr_dir: str, gt_dir: str, times=None, scale=None, channels: str = "y",
                    metric: str = "quantised", ensemble=False):
    """evaluate_sequence for frames on disk: lr_dir holds the low-resolution input frames, gt_dir the ground
    truth of the output frames in output order (pair-major, then time: the numbering run_folder writes under
    HR/); output frames beyond the last file in gt_dir are not scored.  Files are read with PIL and flipped to
    BGR as run_folder does; numeric names sort by value.  `metric` and `ensemble` as in evaluate_sequence.  Prints the two
    averages in the reference's format."""
    from PIL import Image

    def read(d, name):
        return np.ascontiguousarray(np.asarray(Image.open(os.path.join(d, name)).convert("RGB"))[:, :, ::-1])

    lr = np.stack([read(lr_dir, nm) for nm in sorted(os.listdir(lr_dir), key=_frame_key)])
    dev = getattr(model, "device", "cuda")
    frames = torch.from_numpy(np.ascontiguousarray(lr[:, :, :, ::-1])).to(dev).permute(0, 3, 1, 2).float() / 255.0
    nt = len(HARNESS_TIMES if times is None else times)
    gts = [read(gt_dir, nm) for nm in sorted(os.listdir(gt_dir), key=_frame_key)]
    gt = [[gts[i * nt + k] if i * nt + k < len(gts) else None for k in range(nt)] for i in range(len(lr) - 1)]
    res = evaluate_sequence(model, frames.contiguous(), gt, times, scale, channels, metric, ensemble)
    print("AVG PSNR: {:.4f}, AVG SSIM: {:.4f}".format(res["avg_psnr"], res["avg_ssim"]))
    return res


# ----------------------------------------------------------------------------- streaming whole videos
def frame_schedule(fps_in, fps_out, n_frames=None):
    """Where the output frames of a frame-rate conversion fall, in exact Fraction arithmetic: yields (pair, t)
    for output frame j = 0, 1, ...: its instant j / fps_out lies in input pair p = floor(j fps_in / fps_out)
    (between input frames p and p + 1) at t = j fps_in / fps_out - p in [0, 1).  Any positive rational rates;
    with fps_out < fps_in some pairs receive no frame.  n_frames=None: endless, to be consumed as pairs become
    available.  n_frames = n: the floor((n - 1) fps_out / fps_in) + 1 frames of an n-frame clip, where an output
    falling exactly on the last input instant is pair n - 2 at t = 1 (there is no pair n - 1)."""
    from fractions import Fraction
    fi, fo = Fraction(fps_in), Fraction(fps_out)
    if fi <= 0 or fo <= 0:
        raise ValueError("frame rates must be positive")
    if n_frames is not None and n_frames < 2:
        raise ValueError("a clip needs at least two frames")
    step = fi / fo
    j = 0
    while True:
        pos = j * step
        p = pos.numerator // pos.denominator
        t = pos - p
        if n_frames is not None and p >= n_frames - 1:
            if p == n_frames - 1 and t == 0:
                yield n_frames - 2, Fraction(1)
            return
        yield p, t
        j += 1


def _padded_size(h, w):
    return int(4 * math.ceil(h / 4)), int(4 * math.ceil(w / 4))


def scene_scores(sad, h, w, prev=None):
    """Cut scores of consecutive pairs from their luma SADs (ops.scene_sad over h x w pixels; pure host code).
    m_p = sad_p / (255 h w) is the mean luma change of pair p in [0, 1], and score_p = min(m_p, |m_p - m_p-1|):
    a cut is a large change that the pair before it did not show.  The min tells a cut from what only looks like
    one: steady fast motion has a large m but a small change of m, and a one-frame flash gives two large m in a
    row, of which the second scores about 0.  ``prev`` is m of the pair before the first one -- the ``last``
    returned for the preceding chunk, so that scoring a clip in pieces equals scoring it at once; None at the start
    of a stream, where m_p-1 is taken as m_p itself and the very first pair scores 0.  Two consequences: a cut
    between frames 0 and 1 of a stream is never detected, and a scene that lasts one frame is detected once (at
    its first pair, not at the pair that leaves it).  Returns (scores, last): a list of floats and the last m
    (``prev`` itself for an empty ``sad``)."""
    area = 255 * int(h) * int(w)
    scores = []
    for s in sad:
        m = int(s) / area
        scores.append(min(m, abs(m - (m if prev is None else prev))))
        prev = m
    return scores, prev


def _render_chunks(model, chunks, h, w, fps_in, fps_out, out_hw, scene_threshold=None, hold_pairs=(), cuts=None,
                   ensemble=False):
    """render_stream's core.  ``chunks`` yields device tensors [k, 3, h_n, w_n] of new input frames, already
    zero-padded to a multiple of 4 (k >= 1; the pairs of a chunk are its frames plus the previous chunk's last).
    Gradients are switched off around the model calls only, never across a yield.  scene_threshold / hold_pairs /
    cuts: render_stream's; a cut pair is never fused, breaks the run of pairs on either side, and its outputs
    repeat the model's rendering of one of its two frames.  ensemble: every decode, the held frames' included, is
    the local ensemble's (LunaTokis.decoding_pairs)."""
    ekw = {"ensemble": True} if ensemble else {}
    hn, wn = _padded_size(h, w)
    OH, OW = out_hw
    grid = (int(round(OH * hn / h)), int(round(OW * wn / w)))      # virtual grid of the padded frame
    sched = frame_schedule(fps_in, fps_out)
    pending = next(sched)
    base = 0                      # index of the first pair of the current chunk
    last, last_feats = None, None
    B = 0                         # pairs of the latent the model holds after a chunk (for the closing t = 1 frame)
    forced = frozenset(int(p) for p in hold_pairs)
    prev_m = None                 # mean luma change of the previous chunk's last pair (scene_scores' prev)
    last_cut = False              # the last pair so far is a cut
    closing = None                # ... and this is its held frame p + 1, if an output showed it already

    def fuse(x, feats, a, b):
        with torch.no_grad():
            model.gen_feat_window(x[a:b + 1], frame_feats=tuple(f[a:b + 1] for f in feats))
        return b - a

    def held(x, feats, i):
        """The model's rendering of frame i of (x, feats) standing still: the degenerate pair (i, i) at t = 0."""
        with torch.no_grad():
            model.gen_feat_window(torch.cat([x[i:i + 1], x[i:i + 1]]),
                                  frame_feats=tuple(torch.cat([f[i:i + 1], f[i:i + 1]]) for f in feats))
            o = model.decoding_pairs([0], [torch.zeros(1, dtype=torch.float32)], grid, **ekw)[0][0]
        return o[:, :OH, :OW]

    for x in chunks:
        with torch.no_grad():
            feats = model.frame_features(x)                         # every frame is encoded exactly once
            if last is not None:
                x = torch.cat([last, x])
                feats = tuple(torch.cat([a, b]) for a, b in zip(last_feats, feats))
            last, last_feats = x[-1:].clone(), tuple(f[-1:].clone() for f in feats)
        P = x.shape[0] - 1
        if P == 0:
            continue                                                # a first chunk of one frame: no pair yet
        cut = [base + i in forced for i in range(P)]
        if scene_threshold is not None:
            from . import ops
            # one launch over the chunk (its P pairs are x's adjacent frames) and one read-back of P integers
            scores, prev_m = scene_scores(ops.scene_sad(x, h, w).tolist(), h, w, prev_m)
            cut = [c or s > scene_threshold for c, s in zip(cut, scores)]
        if cuts is not None:
            cuts.extend(base + i for i in range(P) if cut[i])
        per = [[] for _ in range(P)]                                # query times of each pair of the chunk
        while pending[0] < base + P:
            per[pending[0] - base].append(pending[1])
            pending = next(sched)
        last_cut, closing = cut[-1], None
        # runs of consecutive uncut pairs that have queries share one latent; pairs without an output are not run
        a = 0
        while a < P:
            if not per[a]:
                a += 1
                continue
            if cut[a]:
                # hold instead of blend: outputs before the middle of the pair show frame a, the others frame
                # a + 1, each rendered once and repeated as tensors of their own
                for i, ts in ((a, [t for t in per[a] if 2 * t < 1]), (a + 1, [t for t in per[a] if 2 * t >= 1])):
                    if ts:
                        o = held(x, feats, i)
                        if i == P and pending == (base + P, 0):
                            closing = o.clone()                     # the frame a closing t = 1 output would show
                        for _ in ts[1:]:
                            yield o.clone()
                        yield o
                        del o
                a += 1
                continue
            b = a
            while b < P and per[b] and not cut[b]:
                b += 1
            B = fuse(x, feats, a, b)
            yield from _decode_run(model, per[a:b], grid, OH, OW, ekw)
            a = b
        base += P
        if not per[-1] and not last_cut and pending == (base, 0):
            # the next output falls exactly on this chunk's last frame: if the stream ends here it is the last
            # pair at t = 1, so its latent is made now, while both of its frames are held (should the stream
            # go on, this one pair was fused for nothing; only a lower output rate can come here)
            B = fuse(x, feats, P - 1, P)
        del x, feats
    if base == 0:
        raise ValueError("render_stream needs at least two frames")
    if pending == (base, 0) and last_cut:
        # the stream ended on an output instant and on a cut: the last frame, held (the carried frame and features)
        yield closing if closing is not None else held(last, last_feats, 0)
    elif pending == (base, 0):
        # the stream ended on an output instant: the last pair (the last item of the model's latent) at t = 1
        yield from _decode_run(model, [[]] * (B - 1) + [[1]], grid, OH, OW, ekw)


def _decode_run(model, per, grid, OH, OW, ekw={}):
    """Decode the model's current latent (one item per entry of ``per``) at each item's own query times and yield
    the top-left OH x OW crops in display order.  Items are grouped by their number of queries, one decoding call
    per group with per-item times, so no frame is decoded that is not yielded.  ekw: further keywords of
    decoding_pairs (the local ensemble)."""
    groups = {}
    for i, ts in enumerate(per):
        if ts:
            groups.setdefault(len(ts), []).append(i)
    outs = {}
    for cnt, idx in groups.items():
        times = [torch.tensor([float(per[i][k]) for i in idx], dtype=torch.float32) for k in range(cnt)]
        with torch.no_grad():
            preds = model.decoding_pairs(idx, times, grid, **ekw)
        for j, i in enumerate(idx):
            outs[i] = [p[j] for p in preds]
        del preds
    for i in sorted(outs):
        for o in outs.pop(i):
            yield o[:, :OH, :OW]


def _out_size(h, w, scale, out_size):
    if out_size is not None:
        OH, OW = int(out_size[0]), int(out_size[1])
    else:
        OH, OW = int(round(h * scale)), int(round(w * scale))
    if OH < 1 or OW < 1:
        raise ValueError(f"bad output size {OH} x {OW}")
    return OH, OW


def render_stream(model, frames, fps_in, fps_out, scale=4, out_size=None, chunk_pairs=8, scene_threshold=None,
                  hold_pairs=(), cuts=None, ensemble=False):
    """Render a video of any length at any output frame rate in bounded memory.  ``frames``: an iterable of RGB
    float [3, h, w] frames in [0, 1] (host or device) at ``fps_in``; yields device float [3, OH, OW] frames
    (unclamped) at ``fps_out`` in display order, (OH, OW) = ``out_size`` or (h, w) * ``scale``.  The output frames
    are those of ``frame_schedule``; each equals the crop of ``run_sequence(model, clip, times=[t])[pair][0]`` bit
    for bit, whatever the chunking.

    Frames are taken ``chunk_pairs`` at a time (one more for the first chunk), padded to a multiple of 4 as the
    harness does, and encoded exactly once (``frame_features``); the last frame of a chunk and its features are
    carried into the next.  The decoder's virtual grid is that of the padded frame, (round(OH h_n / h),
    round(OW w_n / w)), and the yielded frame its top-left OH x OW crop -- for h, w multiples of 4 exactly
    ``decoding(scale=(OH, OW))``.  Alive at a time: at most chunk_pairs + 1 input frames, one chunk's features and
    latents, and the decoded frames of one chunk that have not been yielded yet.

    ``ensemble``: every frame, held frames at scene cuts included, is decoded with the local ensemble
    (``LunaTokis.decoding(ensemble=True)``: no seams at LR pixel borders, about four times the decode).

    Scene cuts (off by default).  ``scene_threshold``: a float switches the detector on -- one ``ops.scene_sad`` per
    chunk over its frames (the carried last frame first) and one read-back of its pair sums; pair p is a cut when
    ``scene_scores``' score_p > scene_threshold (see there for what is and is not detected).  ``hold_pairs``: pair
    indices that are cuts whatever the detector says, e.g. from an edit list (no detector, any device).  ``cuts``:
    a list that receives the index of every cut pair, in order.  The schedule does not change: an output (p, t) of
    a cut pair shows input frame p if t < 1/2 and frame p + 1 otherwise (the closing t = 1 frame of a stream that
    ends on a cut included), where "shows frame f" is the model's rendering of the degenerate pair (f, f) at t = 0,
    bit for bit the crop of ``run_sequence(model, stack([frame_f, frame_f]), times=[0.0])[0][0]`` -- the same size
    and the same network as its neighbours.  A cut pair is never fused and splits the runs either side of it; a
    held frame is fused and decoded once per pair and repeated as separate tensors; the memory bound grows by one
    pair (the two-frame window of a held frame) and at most one output frame."""
    import itertools
    if chunk_pairs < 1:
        raise ValueError("chunk_pairs must be >= 1")
    it = iter(frames)
    head = list(itertools.islice(it, 1))
    if not head:
        raise ValueError("render_stream needs at least two frames")
    if head[0].dim() != 3 or head[0].shape[0] != 3:
        raise ValueError(f"frames must be [3, h, w], got {tuple(head[0].shape)}")
    h, w = head[0].shape[1:]
    hn, wn = _padded_size(h, w)
    dev = getattr(model, "device", "cuda")

    def chunks():
        want = chunk_pairs + 1
        while True:
            new = head + list(itertools.islice(it, want - len(head)))
            if not new:
                return
            head.clear()
            want = chunk_pairs
            x = torch.zeros(len(new), 3, hn, wn, device=dev, dtype=torch.float32)
            while new:
                f = new.pop()
                if tuple(f.shape) != (3, h, w):
                    raise ValueError(f"frame of shape {tuple(f.shape)} in a {h} x {w} stream")
                x[len(new), :, :h, :w] = f
                del f
            yield x

    return _render_chunks(model, chunks(), h, w, fps_in, fps_out, _out_size(h, w, scale, out_size), scene_threshold,
                          hold_pairs, cuts, ensemble)


def render_y4m(model, src, dst, fps_out=None, multiplier=8, scale=4, chunk_pairs=8, matrix="auto", out_size=None,
               scene_threshold=None, hold_pairs=(), cuts=None, ensemble=False):
    """Render a YUV4MPEG2 stream to another: reader -> upload -> yuv_to_rgb -> render_stream -> rgb_to_yuv ->
    download -> writer.  src / dst: paths or binary file objects (pipes work: nothing seeks).  The output runs at
    ``fps_out`` (default: ``multiplier`` x the input rate) and (h, w) * ``scale`` (or ``out_size`` = (OH, OW)); it
    keeps the input's chroma layout, depth, range, matrix ("auto": BT.709 for an input luma >= 1280 wide or >= 720
    high, else BT.601) and X tags, so colours survive the round trip.  Uploads and downloads go through pinned host
    buffers, one chunk of input frames / one chunk's worth of output frames at a time.  scene_threshold / hold_pairs / cuts:
    render_stream's scene-cut arguments (the detector scores the converted RGB frames); ensemble: render_stream's.  Returns (frames read,
    frames written)."""
    from fractions import Fraction

    from . import ops, y4m
    reader = y4m.Y4MReader(src, matrix)
    try:
        fmt = reader.fmt
        fps_in = reader.fps
        fps_o = Fraction(fps_out) if fps_out is not None else fps_in * Fraction(multiplier)
        h, w = fmt.height, fmt.width
        hn, wn = _padded_size(h, w)
        OH, OW = _out_size(h, w, scale, out_size)
        fmt_out = fmt.resized(OW, OH)
        dev = getattr(model, "device", "cuda")
        first_n = chunk_pairs + 1
        pin_in = torch.empty(first_n, fmt.frame_bytes, dtype=torch.uint8).pin_memory()
        host_in = pin_in.numpy()
        uploaded = torch.cuda.Event()

        def chunks():
            want = first_n
            while True:
                k = 0
                uploaded.synchronize()                    # the previous chunk has left the pinned buffer
                while k < want:
                    fr = reader.read_frame()
                    if fr is None:
                        break
                    host_in[k] = fr
                    k += 1
                if k == 0:
                    return
                want = chunk_pairs
                yuv = pin_in[:k].to(dev, non_blocking=True)
                uploaded.record()
                x = torch.zeros(k, 3, hn, wn, device=dev, dtype=torch.float32)
                ops.yuv_to_rgb(yuv, fmt, out=x)            # straight into the padded model input
                del yuv
                yield x

        per_chunk = max(1, math.ceil(chunk_pairs * fps_o / fps_in))
        ybuf = torch.empty(per_chunk, fmt_out.frame_bytes, device=dev, dtype=torch.uint8)
        pin_out = torch.empty(per_chunk, fmt_out.frame_bytes, dtype=torch.uint8).pin_memory()
        writer = y4m.Y4MWriter(dst, fmt_out, fps_o, reader.extra_tags, reader.interlace, reader.aspect,
                               reader.range_tagged)
        try:
            def flush(k):
                pin_out[:k].copy_(ybuf[:k], non_blocking=True)
                torch.cuda.current_stream().synchronize()
                host = pin_out.numpy()
                for j in range(k):
                    writer.write(host[j])

            k = 0
            for frame in _render_chunks(model, chunks(), h, w, fps_in, fps_o, (OH, OW), scene_threshold, hold_pairs,
                                        cuts, ensemble):
                ops.rgb_to_yuv(frame[None], fmt_out, out=ybuf[k:k + 1])   # the crop, converted in place
                del frame
                k += 1
                if k == per_chunk:
                    flush(k)
                    k = 0
            if k:
                flush(k)
            return reader.frames_read, writer.frames_written
        finally:
            writer.close()
    finally:
        reader.close()
