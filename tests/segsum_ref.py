"""The value of stif_segsum in numpy, from its definition in include/stif.h and nothing else (shared by
tests/test_deterministic_host.py, which pins it, and tests/test_gpu_deterministic.py, which holds the kernels to it).

Entry e has a packed word (key << 32) | e, a weight w[e] and a source sub-row rows[e >> 2].  For every destination row
d < D: the entries with key == d in ascending e, in chunks of CHUNK; inside a chunk acc = acc + (w * v) from +0, both
operations rounded to float32 (numpy rounds every float32 operation, so nothing is fused); the row is the first
partial plus the following partials in chunk order.  Empty list: +0."""
import numpy as np

CHUNK = 512


def pack(key):
    key = np.asarray(key, np.int64)
    return (key << 32) | np.arange(key.size, dtype=np.int64)


def sub_rows(src, E, row_stride, K, C, col0):
    """[ceil(E / 4), C]: the source sub-row of every group of four entries, src a flat float32 array"""
    s = np.arange((E + 3) // 4, dtype=np.int64)
    start = (s // K) * row_stride + (s % K) * C + col0
    return np.asarray(src, np.float32).reshape(-1)[start[:, None] + np.arange(C)]


def sorted_segments(words, D):
    srt = np.sort(np.asarray(words, np.int64))
    return srt, np.searchsorted(srt, np.arange(D + 1, dtype=np.int64) << 32).astype(np.int64)


def emulate(words, w, rows, D, sort=True, reverse=False):
    """dst [D, C] float32.  ``words`` in any storage order; ``sort=False`` takes the lists in the order given (what a
    kernel that skipped the sort would add), ``reverse`` walks every list backwards (another order of the same terms)."""
    words = np.asarray(words, np.int64)
    w, rows = np.asarray(w, np.float32), np.asarray(rows, np.float32)
    if sort:
        words = np.sort(words)
    else:
        words = words[np.argsort(words >> 32, kind="stable")]   # grouped by key, the given order kept inside a list
    key, e = words >> 32, words & 0xffffffff
    live = key < D
    key, e = key[live], e[live]
    starts = np.searchsorted(key, np.arange(D + 1))
    lens = np.diff(starts)
    pos = np.arange(key.size) - starts[key]
    if reverse:
        pos = lens[key] - 1 - pos
    C = rows.shape[1]
    total, part = np.zeros((D, C), np.float32), np.zeros((D, C), np.float32)
    by_pos = np.argsort(pos, kind="stable")
    cuts = np.searchsorted(pos[by_pos], np.arange(int(lens.max(initial=0)) + 1))
    for t in range(len(cuts) - 1):
        sel = by_pos[cuts[t]:cuts[t + 1]]          # one entry per row that has a t-th entry
        r, ee = key[sel], e[sel]
        prod = (w[ee][:, None] * rows[ee >> 2]).astype(np.float32)
        part[r] = (part[r] + prod).astype(np.float32)
        done = ((t + 1) % CHUNK == 0) | (t == lens[r] - 1)
        rd = r[done]
        first = t < CHUNK
        total[rd] = part[rd] if first else (total[rd] + part[rd]).astype(np.float32)
        part[rd] = 0
    return total
