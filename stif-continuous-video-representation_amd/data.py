"""Training batches from frame folders: the reference's arbitrary-scale data path (``mode: Adobe_a``) on the engine.

What the reference does per batch in ``data/__init__.py:124-154`` (``collate_function2``) and ``data/util.py:126-140``
(``augment_a2``), restated here:

* one ``d_scale ~ U(2, 4)`` per batch, a crop side ``G = floor(lq_size * d)`` and one crop position for the whole batch;
* the two input frames of every item become the LQ pair, ``imresize_np(crop, 1 / (2 d))``, and its three sampled
  in-between frames the GT, ``imresize_np(crop, 1 / 2)``;
* one flip-W / flip-H / transpose draw for the whole batch, then BGR -> RGB and HWC -> CHW;
* ``GT.shape[-2:]`` is the decoder's query size.

``resize_geometry`` / ``draw_collate_params`` are the sizes and the random draws (the draw order of the reference, so
``random.seed(s)`` there and ``random.Random(s)`` here give the same batch), ``ClipIndex`` the window list of
``Adobe_arbitrary.AdobeDataset.__init__`` (:90-108), ``build_batch`` the batch on the device -- two launches of
``stif_build_batch`` (csrc/resample.hip), one for the LQ frames and one for the GT frames, no
host synchronisation -- and ``build_batch_host`` the same function in numpy, which is what the tests compare the
kernel with and what runs without a GPU.  ``BatchLoader`` decodes frame files on worker threads and builds batches
ahead of the training loop on a side stream; batch ``i`` is a pure function of ``(seed, i)``, so a run resumed at
iteration ``i`` needs no sampler state.

Not reproduced: lmdb / memcached sources, ``Vimeo7Dataset`` / ``Adobe_dataset``, and the draws of the reference's
``__getitem__`` whose results it never uses (see ``ClipIndex.sample``).
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import math
import os
import queue
import random
import threading

import numpy as np

LQ_SIZE = 64                 # collate_function2's LQ_size
MAX_WORKERS = 16
_EXTS = (".png", ".jpg", ".jpeg")


@dataclasses.dataclass(frozen=True)
class Geometry:
    """Sizes of one batch: crop side, the two imresize scales and the two output sides."""
    G: int
    lq_scale: float
    gt_scale: float
    lq: int
    gt: int


def resize_geometry(lq_size: int = LQ_SIZE, d_scale: float = 2.0) -> Geometry:
    """G = floor(lq_size d); the LQ frames are the crop resized by 1 / (2 d) to ceil(G / (2 d)) = lq_size / 2, the GT
    frames the crop resized by 1 / 2 to ceil(G / 2).  The output sides are computed as imresize_np computes them,
    ceil(G * scale) in double precision.  lq_size must be a positive multiple of 8, so that the LQ side is a multiple
    of 4 (three pyramid levels)."""
    if int(lq_size) != lq_size or lq_size < 8 or lq_size % 8:
        raise ValueError(f"lq_size must be a positive multiple of 8 (the LQ side lq_size / 2 a multiple of 4), got {lq_size}")
    d = float(d_scale)
    if not d >= 1.0:
        raise ValueError(f"d_scale must be >= 1 (the reference draws U(2, 4)), got {d_scale}")
    G = int(np.floor(lq_size * d))
    lq_scale, gt_scale = 1 / (2 * d), 1 / 2
    return Geometry(G, lq_scale, gt_scale, int(math.ceil(G * lq_scale)), int(math.ceil(G * gt_scale)))


@dataclasses.dataclass(frozen=True)
class CollateParams:
    """The random draws of one batch.  ``x`` was drawn along the frame's short side and ``y`` along its long side."""
    d_scale: float
    G: int
    x: int
    y: int
    hflip: bool
    vflip: bool
    rot90: bool
    lq_size: int = LQ_SIZE

    @property
    def flags(self) -> int:
        """stif_build_batch's flags word: bit 0 hflip, bit 1 vflip, bit 2 rot90."""
        return int(self.hflip) | int(self.vflip) << 1 | int(self.rot90) << 2

    @property
    def geometry(self) -> Geometry:
        return resize_geometry(self.lq_size, self.d_scale)

    def crop_origin(self, H: int, W: int):
        """(row, col) of the crop in an H x W frame: (x, y) for a landscape or square frame, (y, x) for a portrait
        one (the reference's ``shape[0] == 720`` branch)."""
        return (self.x, self.y) if H <= W else (self.y, self.x)


def draw_collate_params(rng: random.Random, H: int, W: int, lq_size: int = LQ_SIZE) -> CollateParams:
    """The draws of collate_function2 + augment_a2 in their order: uniform(2, 4); randint(0, max(0, S - G));
    randint(0, max(0, Lg - G)); then random() < 0.5 three times (hflip, vflip, rot90 -- all three always drawn).  S / Lg
    are the frame's short / long side, where the reference hard-codes 720 and 1280."""
    d = rng.uniform(2, 4)
    G = resize_geometry(lq_size, d).G
    S, Lg = min(H, W), max(H, W)
    x = rng.randint(0, max(0, S - G))
    y = rng.randint(0, max(0, Lg - G))
    hflip = rng.random() < 0.5
    vflip = rng.random() < 0.5
    rot90 = rng.random() < 0.5
    return CollateParams(d, G, x, y, hflip, vflip, rot90, int(lq_size))


def stream_rng(seed, kind: str, i: int) -> random.Random:
    """The independent stream ``Random(seed, i)`` of the loader: seeded by a string (hashed with SHA-512 by the
    standard library, the same on every platform).  ``kind`` is "batch" (the collate stream of batch i) or "epoch"
    (the permutation of epoch i)."""
    return random.Random(f"stif-data/{seed}/{kind}/{int(i)}")


class ClipIndex:
    """The window list of Adobe_arbitrary.AdobeDataset.__init__ (:90-108).  ``videos`` are folder names under
    ``root``; each folder's frames are named by integers and sorted by value (``10.png`` after ``9.png``).  There is
    one window per ``index`` with ``index + 8 < n``: the inputs are frames ``index`` and ``index + 8`` and the GT
    candidates the nine frames from one to the other, inclusive."""

    INTERVAL = 7

    def __init__(self, root: str, videos):
        self.root = root
        self.inputs, self.candidates = [], []
        for video in videos:
            video = video.strip()
            if not video:
                continue
            names = [f for f in os.listdir(os.path.join(root, video)) if f.lower().endswith(_EXTS)]
            bad = [f for f in names if not os.path.splitext(f)[0].isdigit()]
            if bad:
                raise ValueError(f"frame files are named by integers; {os.path.join(root, video, bad[0])} is not")
            names.sort(key=lambda f: int(os.path.splitext(f)[0]))
            paths = [os.path.join(root, video, f) for f in names]
            index = 0
            while index + self.INTERVAL + 1 < len(paths):
                self.inputs.append((paths[index], paths[index + 1 + self.INTERVAL]))
                self.candidates.append(tuple(paths[index:index + 2 + self.INTERVAL]))
                index += 1

    def __len__(self):
        return len(self.inputs)

    def sample(self, i: int, rng: random.Random):
        """Window i with three of its nine candidates: ``sorted(rng.sample(range(9), 3))`` as __getitem__ (:189) draws
        them.  Returns (the five paths -- two inputs, three GTs --, the three times k / 8).  The reference's
        __getitem__ also draws ``center_frame_idx``, ``interval`` and the reverse flag (:154-183) and uses none of
        them; those draws are not reproduced."""
        ks = sorted(rng.sample(range(9), 3))
        return list(self.inputs[i]) + [self.candidates[i][k] for k in ks], [k / 8 for k in ks]


# ----------------------------------------------------------------------------- batches
def _is_tensor(a):
    return type(a).__module__.startswith("torch") and hasattr(a, "data_ptr")


def _check_frame(fr):
    if str(fr.dtype) not in ("uint8", "torch.uint8"):
        raise ValueError(f"frames must be uint8 (BGR, as cv2.imread), got {str(fr.dtype).replace('torch.', '')}")
    if len(fr.shape) != 3 or fr.shape[2] != 3:
        raise ValueError(f"frames must be [H, W, 3], got {tuple(fr.shape)}")


def _frame_grid(frames):
    """frames -> a [B][5] list of lists of arrays / tensors, each checked to be uint8 [H, W, 3]."""
    grid = [list(item) for item in frames]
    if not grid or any(len(item) != 5 for item in grid):
        raise ValueError("frames must be [B][5]: two input frames and three ground-truth frames per item")
    for item in grid:
        for fr in item:
            _check_frame(fr)
        if len({tuple(fr.shape) for fr in item}) != 1:
            raise ValueError(f"the five frames of an item must share a size, got {[tuple(fr.shape) for fr in item]}")
    return grid


def _origin(shape, params: CollateParams):
    """(row, col) of the crop in a frame of ``shape``: a G x G frame is the crop itself."""
    H, W = int(shape[0]), int(shape[1])
    G = params.G
    if (H, W) == (G, G):
        return 0, 0
    r, c = params.crop_origin(H, W)
    if r < 0 or c < 0 or r + G > H or c + G > W:
        raise ValueError(f"the {G} x {G} crop at ({r}, {c}) does not fit the {H} x {W} frame")
    return r, c


def _times(times, B):
    t = np.asarray(times, np.float32)
    if t.shape != (B, 3):
        raise ValueError(f"times must be [B][3], got {t.shape}")
    return t


def _resize_host(crop, scale, o):
    """imresize_np(crop, scale, True).astype(float32) / 255 for a uint8 [G, G, 3] crop, with the engine's fp32 tables
    and fp64 accumulation (H pass, then W pass)."""
    from .video import resize_tables
    G = crop.shape[0]
    w, idx, s0 = resize_tables(G, o, scale)
    P = w.shape[1]
    k = idx[:, None].astype(np.int64) + np.arange(P)[None, :] - s0                # [o, P] in the unpadded crop
    src = np.where(k < 0, -k - 1, np.where(k >= G, 2 * G - 1 - k, k))
    if src.min() < 0 or src.max() >= G:
        raise ValueError(f"the symmetric padding ({s0}) is wider than the {G} x {G} crop")
    wd = w.astype(np.float64)
    h = np.einsum("ip,ipxc->ixc", wd, crop.astype(np.float64)[src])              # [o, G, 3]
    out = np.einsum("jp,ijpc->ijc", wd, h[:, src])                                # [o, o, 3]
    return out.astype(np.float32) / np.float32(255.0)


def _augment_host(img, params: CollateParams):
    """augment_a2 on one HWC image, then BGR -> RGB, HWC -> CHW."""
    if params.hflip:
        img = img[:, ::-1]
    if params.vflip:
        img = img[::-1]
    if params.rot90:
        img = img.transpose(1, 0, 2)
    return np.ascontiguousarray(img[:, :, ::-1].transpose(2, 0, 1))


def build_batch_host(frames, params: CollateParams, times=None):
    """``build_batch`` in numpy on the CPU: the same dictionary with host tensors.  ``frames`` [B][5] uint8 BGR crops
    (G x G) or whole frames, numpy arrays or host tensors; ``times`` [B][3] (default: all zero)."""
    import torch
    grid = _frame_grid(frames)
    geo, G, B = params.geometry, params.G, len(grid)
    lq = np.empty((B, 2, 3, geo.lq, geo.lq), np.float32)
    gt = np.empty((B, 3, 3, geo.gt, geo.gt), np.float32)
    for b, item in enumerate(grid):
        r, c = _origin(item[0].shape, params)
        for k, fr in enumerate(item):
            crop = np.asarray(fr)[r:r + G, c:c + G]
            if k < 2:
                lq[b, k] = _augment_host(_resize_host(crop, geo.lq_scale, geo.lq), params)
            else:
                gt[b, k - 2] = _augment_host(_resize_host(crop, geo.gt_scale, geo.gt), params)
    t = torch.from_numpy(_times(np.zeros((B, 3)) if times is None else times, B))
    return {"LQs": torch.from_numpy(lq), "GT": torch.from_numpy(gt), "time": [t[:, k:k + 1].clone() for k in range(3)],
            "shape": (geo.gt, geo.gt)}


_TABLES = {}      # (G, o, scale) -> (weights [o, P], indices [o], P, s0)


def _tables(G, o, scale):
    from .video import resize_tables
    key = (G, o, scale)
    hit = _TABLES.get(key)
    if hit is None:
        w, idx, s0 = resize_tables(G, o, scale)
        if s0 > G:
            raise ValueError(f"the symmetric padding ({s0}) is wider than the {G} x {G} crop")
        if len(_TABLES) > 256:
            _TABLES.clear()
        hit = _TABLES[key] = (w, idx, w.shape[1], s0)
    return hit


def _same_device(t, dev):
    return t.device == dev or (dev.index is None and t.device.type == dev.type)


def _sources(frames, params, dev):
    """Where the 5 B crops are: (keep-alive, base pointer, crop_off [5 B], row_stride [5 B]) with the frames in
    (item, frame) order.  Device frames are addressed in place, relative to the lowest of their addresses; host
    frames are cropped into one pinned staging buffer and uploaded (a pinned [B, 5, G, G, 3] tensor is uploaded as
    it is).  One stacked [B, 5, H, W, 3] array or tensor is handled without a loop over its frames."""
    import torch
    G = params.G
    if hasattr(frames, "shape") and len(frames.shape) == 5:
        B, five, H, W, ch = (int(v) for v in frames.shape)
        if five != 5:
            raise ValueError("frames must be [B][5]: two input frames and three ground-truth frames per item")
        _check_frame(frames[0][0])
        r, c = _origin((H, W), params)
        if _is_tensor(frames) and frames.is_cuda:
            if not _same_device(frames, dev):
                raise ValueError(f"the frames are on {frames.device}, the batch is built on {dev}")
            sb, sk, sr, sp, sc = frames.stride()
            if sc != 1 or sp != 3:
                raise ValueError("device frames must have contiguous pixels (strides [row, 3, 1])")
            off = (np.arange(B, dtype=np.int64)[:, None] * sb + np.arange(5, dtype=np.int64)[None, :] * sk).ravel()
            return frames, frames.data_ptr(), off + (r * sr + 3 * c), np.full(5 * B, sr, np.int64)
        if _is_tensor(frames) and (H, W) == (G, G) and frames.is_pinned() and frames.is_contiguous():
            stage = frames                                            # the loader's staging buffer, as it is
        else:
            stage = torch.empty(B, 5, G, G, 3, dtype=torch.uint8, pin_memory=True)
            stage.numpy()[...] = np.asarray(frames)[:, :, r:r + G, c:c + G]
    else:
        grid = [list(item) for item in frames]
        B = len(grid)
        if not grid or any(len(item) != 5 for item in grid):
            raise ValueError("frames must be [B][5]: two input frames and three ground-truth frames per item")
        flat = [fr for item in grid for fr in item]
        on_dev = _is_tensor(flat[0]) and flat[0].is_cuda
        origin = {}
        off, stride = np.empty(5 * B, np.int64), np.empty(5 * B, np.int64)
        stage = None if on_dev else torch.empty(B, 5, G, G, 3, dtype=torch.uint8, pin_memory=True)
        sv = None if on_dev else stage.numpy().reshape(5 * B, G, G, 3)
        for k, fr in enumerate(flat):
            shape = tuple(fr.shape)
            rc = origin.get(shape)
            if rc is None:
                _check_frame(fr)
                rc = origin[shape] = _origin(shape, params)
            if k % 5 and shape != last:
                raise ValueError(f"the five frames of an item must share a size, got {shape} after {last}")
            last = shape
            if (_is_tensor(fr) and fr.is_cuda) != on_dev:
                raise ValueError("frames must be all on the host or all on the device")
            if str(fr.dtype) not in ("uint8", "torch.uint8"):
                _check_frame(fr)
            if on_dev:
                sr, sp, sc = fr.stride()
                if sc != 1 or sp != 3:
                    raise ValueError("device frames must have contiguous pixels (strides [row, 3, 1])")
                if not _same_device(fr, dev):
                    raise ValueError(f"a frame is on {fr.device}, the batch is built on {dev}")
                off[k] = fr.data_ptr() + rc[0] * sr + 3 * rc[1]
                stride[k] = sr
            else:
                sv[k] = np.asarray(fr)[rc[0]:rc[0] + G, rc[1]:rc[1] + G]
        if on_dev:
            base = int(off.min())
            return flat, base, off - base, stride
    crops = stage.to(dev, non_blocking=True)
    return crops, crops.data_ptr(), np.arange(5 * B, dtype=np.int64) * (G * G * 3), np.full(5 * B, 3 * G, np.int64)


def build_batch(frames, params: CollateParams, device="cuda", times=None):
    """One training batch on the device: ``{'LQs': [B, 2, 3, l, l], 'GT': [B, 3, 3, g, g], 'time': three [B, 1],
    'shape': (g, g)}`` in the layouts train.LunaTokis and TimesLoss take, on the current stream of ``device``.

    ``frames`` [B][5] (two inputs, three ground truths per item) are uint8 BGR [H, W, 3]: G x G crops or whole
    frames of which the crop at ``params.crop_origin`` is taken; numpy arrays / host tensors (their crops go up
    through one pinned staging buffer) or device tensors (read in place, whatever their row stride), as nested lists
    or as one stacked [B, 5, H, W, 3].  ``times`` [B][3] are the query times of the ground truths (default zeros).
    Two launches of stif_build_batch, one for the 2 B LQ frames and one for the 3 B GT frames.  The two table pairs
    (video.resize_tables), the crop offsets and row strides and the times go up in one asynchronous copy from one
    pinned buffer; nothing synchronises."""
    import torch
    from . import _lib as L
    dev = torch.device(device)
    geo, G = params.geometry, params.G
    keep, src_ptr, off, stride = _sources(frames, params, dev)
    B = off.shape[0] // 5
    tabs = [_tables(G, geo.lq, geo.lq_scale), _tables(G, geo.gt, geo.gt_scale)]
    tt = _times(np.zeros((B, 3)) if times is None else times, B)
    # one upload: [crop_off | row_stride] (int64, LQ frames first, then GT frames) | times | w, idx of each group
    order = np.arange(5 * B).reshape(B, 5)
    order = np.concatenate([order[:, :2].ravel(), order[:, 2:].ravel()])
    parts = [off[order], stride[order], tt]
    for w, idx, _, _ in tabs:
        parts += [w, idx]
    starts = np.cumsum([0] + [(a.nbytes + 15) // 16 * 16 for a in parts])
    up = torch.empty(int(starts[-1]), dtype=torch.uint8, pin_memory=True)
    uv = up.numpy()
    for a, o in zip(parts, starts):
        uv[o:o + a.nbytes] = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
    dup = up.to(dev, non_blocking=True)
    p0 = dup.data_ptr()
    lq = torch.empty(B, 2, 3, geo.lq, geo.lq, device=dev, dtype=torch.float32)
    gt = torch.empty(B, 3, 3, geo.gt, geo.gt, device=dev, dtype=torch.float32)
    with torch.cuda.device(lq.device):
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        fn = L.lib().stif_build_batch
        for out, o, (w, idx, P, s0), first, n, tab in ((lq, geo.lq, tabs[0], 0, 2 * B, 3),
                                                       (gt, geo.gt, tabs[1], 2 * B, 3 * B, 5)):
            L.check(fn(src_ptr, p0 + int(starts[0]) + 8 * first, p0 + int(starts[1]) + 8 * first, out.data_ptr(), n, G,
                       o, p0 + int(starts[tab]), p0 + int(starts[tab + 1]), P, s0, params.flags, st),
                    "stif_build_batch")
    del keep
    tdev = dup[int(starts[2]):int(starts[2]) + 12 * B].view(torch.float32).view(B, 3)
    return {"LQs": lq, "GT": gt, "time": [tdev[:, k:k + 1] for k in range(3)], "shape": (geo.gt, geo.gt)}


# ----------------------------------------------------------------------------- loader
def _read_size(path):
    from PIL import Image
    with Image.open(path) as im:
        return im.size[1], im.size[0]


def _decode_crop(path, r, c, G, dst):
    """Decode one frame with PIL and copy its crop, in BGR order, into ``dst`` [G, G, 3]."""
    from PIL import Image
    with Image.open(path) as im:
        rgb = np.asarray(im.convert("RGB"))
    dst[...] = rgb[r:r + G, c:c + G, ::-1]


def rank_items(batch_size: int, world: int, rank: int):
    """The items [a, b) of a global batch that ``rank`` of ``world`` trains on: contiguous slices, the first
    ``batch_size % world`` ranks one item longer.  More ranks than items is refused: a rank with nothing to do would
    still have to enter every collective."""
    batch_size, world, rank = int(batch_size), int(world), int(rank)
    if world < 1 or not 0 <= rank < world:
        raise ValueError(f"rank {rank} of world {world}")
    if world > batch_size:
        raise ValueError(f"{world} ranks cannot share a batch of {batch_size}: every rank needs at least one item")
    base, rem = divmod(batch_size, world)
    a = rank * base + min(rank, rem)
    return a, a + base + (1 if rank < rem else 0)


class BatchLoader:
    """Training batches built ahead of the loop.  Batch ``i`` (0-based, counted over epochs) is a pure function of
    ``(seed, i)``: epoch ``e = i // (len(index) // batch_size)`` uses the permutation of ``stream_rng(seed, "epoch",
    e)`` (partial batches are dropped), and the collate stream ``stream_rng(seed, "batch", i)`` gives first the batch's
    ``draw_collate_params`` and then each item's ``ClipIndex.sample``, in item order.  So ``workers=0`` and
    ``workers=4`` yield the same bytes in the same order, and a loop resumed at iteration ``i`` passes ``start=i``.

    Worker threads decode PNG / JPG files with PIL into a pinned uint8 staging buffer -- only the crop is copied, in
    BGR order.  A consumer thread uploads the crops on a side stream, launches ``build_batch`` there and hands the
    batch over behind an event, which the iterating thread's current stream waits on (no host wait).  ``workers`` is
    capped at 16 and never derived from the machine's CPU count; ``workers=0`` builds every batch in the iterating
    thread.  ``device=None`` or "cpu" yields ``build_batch_host`` batches (no GPU needed).  All frames of a batch
    must share a size: otherwise ValueError names the paths.

    ``rank`` / ``world`` (data-parallel training): ``batch_size`` stays the global batch and
    ``plan(i)`` is computed for all of it exactly as with one process -- one ``draw_collate_params``, then every item's
    ``sample`` in item order, so the collate stream is the same -- but only the items ``rank_items(batch_size, world,
    rank)`` are decoded, staged and built.  The rank's batch is rows [a, b) of the single-process batch bit for bit
    (``LQs``, ``GT``, ``time``) with the same ``shape``; every rank decodes at the batch's one scale, and ``per_epoch``
    stays global."""

    def __init__(self, index: ClipIndex, batch_size: int, seed, lq_size: int = LQ_SIZE, workers: int = 4,
                 prefetch: int = 2, device="cuda", start: int = 0, rank: int = 0, world: int = 1):
        resize_geometry(lq_size, 2.0)
        self.rank, self.world = int(rank), int(world)
        self.items = rank_items(batch_size, world, rank) if batch_size >= 1 else (0, 0)
        if batch_size < 1 or len(index) < batch_size:
            raise ValueError(f"{len(index)} windows cannot fill a batch of {batch_size}")
        if workers < 0 or prefetch < 1:
            raise ValueError("workers must be >= 0 and prefetch >= 1")
        self.index, self.batch_size, self.seed, self.lq_size = index, int(batch_size), seed, int(lq_size)
        self.workers, self.prefetch = min(int(workers), MAX_WORKERS), int(prefetch)
        self.device = None if device is None or str(device) == "cpu" else device
        self.start = int(start)
        self.per_epoch = len(index) // self.batch_size
        self._perm = (None, None)

    def plan(self, i: int):
        """What batch i is made of: (paths [B][5], times [B][3], CollateParams)."""
        e, k = divmod(int(i), self.per_epoch)
        if self._perm[0] != e:
            perm = list(range(len(self.index)))
            stream_rng(self.seed, "epoch", e).shuffle(perm)
            self._perm = (e, perm)
        items = self._perm[1][k * self.batch_size:(k + 1) * self.batch_size]
        rng = stream_rng(self.seed, "batch", i)
        first = self.index.inputs[items[0]][0]
        H, W = _read_size(first)
        params = draw_collate_params(rng, H, W, self.lq_size)
        paths, times = [], []
        for it in items:
            p, t = self.index.sample(it, rng)
            paths.append(p)
            times.append(t)
        return paths, times, params

    def _stage(self, paths, params, pool):
        """Decode the batch's files into one staging buffer [B, 5, G, G, 3] (pinned when a device is used)."""
        import torch
        G, B = params.G, len(paths)
        flat = [p for item in paths for p in item]
        sizes = [_read_size(p) for p in flat]
        if len(set(sizes)) != 1:
            raise ValueError("frames of one batch must share a size: " + ", ".join(
                f"{p} is {h} x {w}" for p, (h, w) in zip(flat, sizes)))
        H, W = sizes[0]
        if G > min(H, W):
            raise ValueError(f"the {G} x {G} crop does not fit the {H} x {W} frames (e.g. {flat[0]}); lower lq_size")
        r, c = params.crop_origin(H, W)
        stage = torch.empty(B, 5, G, G, 3, dtype=torch.uint8, pin_memory=self.device is not None)
        sv = stage.numpy().reshape(5 * B, G, G, 3)
        if pool is None:
            for k, p in enumerate(flat):
                _decode_crop(p, r, c, G, sv[k])
        else:
            for fut in [pool.submit(_decode_crop, p, r, c, G, sv[k]) for k, p in enumerate(flat)]:
                fut.result()
        return stage

    def build(self, i: int, pool=None):
        """Batch i on the current stream (or on the host)."""
        paths, times, params = self.plan(i)
        a, b = self.items
        paths, times = paths[a:b], times[a:b]
        stage = self._stage(paths, params, pool)
        if self.device is None:
            return build_batch_host(stage.numpy(), params, times)
        return build_batch(stage, params, self.device, times)

    def __iter__(self):
        if self.workers == 0:
            i = self.start
            while True:
                yield self.build(i)
                i += 1
        import torch
        from concurrent.futures import ThreadPoolExecutor
        q = queue.Queue(maxsize=self.prefetch)
        stop = threading.Event()
        gpu = self.device is not None

        def consume():
            i = self.start
            try:
                with ThreadPoolExecutor(max_workers=self.workers) as pool:
                    side = torch.cuda.Stream(device=self.device) if gpu else None
                    while not stop.is_set():
                        if gpu:
                            with torch.cuda.stream(side):
                                item = self.build(i, pool)
                                ev = torch.cuda.Event()
                                ev.record(side)
                        else:
                            item, ev = self.build(i, pool), None
                        while not stop.is_set():
                            try:
                                q.put((item, ev), timeout=0.1)
                                break
                            except queue.Full:
                                pass
                        i += 1
            except BaseException as exc:      # handed to the iterating thread
                while not stop.is_set():
                    try:
                        q.put((exc, None), timeout=0.1)
                        break
                    except queue.Full:
                        pass

        th = threading.Thread(target=consume, name="stif-batch-loader", daemon=True)
        th.start()
        try:
            while True:
                item, ev = q.get()
                if isinstance(item, BaseException):
                    raise item
                if ev is not None:
                    main = torch.cuda.current_stream(item["LQs"].device)
                    main.wait_event(ev)
                    for t in [item["LQs"], item["GT"]] + item["time"]:
                        t.record_stream(main)      # allocated on the side stream, used on this one
                yield item
        finally:
            stop.set()
            th.join()
