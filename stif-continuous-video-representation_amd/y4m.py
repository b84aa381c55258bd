"""YUV4MPEG2 (.y4m) reader / writer, pure host: the one video format that needs no library.  Every ffmpeg build
reads and writes it, also through a pipe (``ffmpeg -i in.mp4 -f yuv4mpegpipe - | ... | ffmpeg -i - out.mp4``), so
both classes work on non-seekable streams: they read exact byte counts and never seek or tell.

A stream is ``YUV4MPEG2 W<w> H<h> F<num>:<den> [I<p>] [A<n>:<d>] [C<tag>] [X<...>]...\\n`` followed, per frame, by
``FRAME[ params]\\n`` and the planes Y | U | V, dense; samples above 8 bits are little-endian uint16.  Supported:
progressive (``Ip``, ``I?`` or no ``I``) 4:2:0 / 4:2:2 / 4:4:4 at 8, 10, 12, 14 or 16 bits.  The four 4:2:0 tags
(420jpeg, 420mpeg2, 420paldv, 420) differ only in where the chroma samples sit; the device conversion treats all of
them as centred (stif.h, stif_yuv_format), and the tag itself is passed through unchanged.

Y4M carries the colour range only as the de-facto ``XCOLORRANGE=FULL|LIMITED`` tag (limited when absent) and no
matrix at all: ``choose_matrix`` is the usual rule (BT.709 for HD sizes, BT.601 below).
"""
from __future__ import annotations

import re
from dataclasses import dataclass, replace
from fractions import Fraction

import numpy as np

MAGIC = b"YUV4MPEG2"
_SUBSAMPLING = {"420jpeg": (1, 1), "420mpeg2": (1, 1), "420paldv": (1, 1), "420": (1, 1), "422": (1, 0),
                "444": (0, 0)}
_DEPTHS = {"": 8, "p10": 10, "p12": 12, "p14": 14, "p16": 16}
_CTAG = re.compile(r"^(420jpeg|420mpeg2|420paldv|420|422|444)(p10|p12|p14|p16)?$")
_MAX_HEADER = 4096      # longest header / FRAME line accepted


@dataclass(frozen=True)
class YuvFormat:
    """Frame layout and colour description of planar YUV frames (what ops.yuv_to_rgb / rgb_to_yuv take).
    ``chroma`` is the Y4M ``C`` family without its depth suffix; it fixes sub_x / sub_y."""
    width: int
    height: int
    chroma: str = "420jpeg"
    depth: int = 8
    matrix: str = "bt601"        # "bt601" | "bt709"
    full_range: bool = False

    def __post_init__(self):
        if self.chroma not in _SUBSAMPLING:
            raise ValueError(f"unsupported chroma layout C{self.chroma}")
        if self.width < 1 or self.height < 1:
            raise ValueError(f"bad frame size W{self.width} H{self.height}")
        if not 8 <= self.depth <= 16:
            raise ValueError(f"unsupported depth {self.depth}")
        if self.matrix not in ("bt601", "bt709"):
            raise ValueError(f'matrix must be "bt601" or "bt709", got {self.matrix!r}')

    @property
    def sub_x(self) -> int:
        return _SUBSAMPLING[self.chroma][0]

    @property
    def sub_y(self) -> int:
        return _SUBSAMPLING[self.chroma][1]

    @property
    def bytes_per_sample(self) -> int:
        return 2 if self.depth > 8 else 1

    @property
    def chroma_size(self):
        """(width, height) of the U and V planes: ceil of the luma size over the subsampling."""
        return (self.width + self.sub_x) >> self.sub_x, (self.height + self.sub_y) >> self.sub_y

    @property
    def frame_bytes(self) -> int:
        cw, ch = self.chroma_size
        return (self.width * self.height + 2 * cw * ch) * self.bytes_per_sample

    @property
    def ctag(self) -> str:
        if self.depth == 8:
            return self.chroma
        suffix = {v: k for k, v in _DEPTHS.items()}.get(self.depth)
        if suffix is None:
            raise ValueError(f"Y4M has no C tag for {self.depth}-bit samples")
        return self.chroma + suffix

    def resized(self, width: int, height: int) -> "YuvFormat":
        return replace(self, width=int(width), height=int(height))

    def planes(self, payload):
        """(y, u, v) numpy views of one frame payload: uint8, or little-endian uint16 above 8 bits."""
        a = np.frombuffer(payload, np.uint8) if not isinstance(payload, np.ndarray) else payload
        if a.size != self.frame_bytes:
            raise ValueError(f"payload holds {a.size} bytes, a frame {self.frame_bytes}")
        a = a.view("<u2") if self.depth > 8 else a
        cw, ch = self.chroma_size
        ny, nc = self.width * self.height, cw * ch
        return (a[:ny].reshape(self.height, self.width), a[ny:ny + nc].reshape(ch, cw),
                a[ny + nc:].reshape(ch, cw))


def choose_matrix(width: int, height: int) -> str:
    """Y4M carries no matrix: BT.709 when the luma is at least 1280 wide or 720 high, else BT.601."""
    return "bt709" if width >= 1280 or height >= 720 else "bt601"


def _open(f, mode):
    if isinstance(f, (str, bytes)) or hasattr(f, "__fspath__"):
        return open(f, mode), True
    return f, False


def _read_exact(f, n):
    """n bytes, fewer only at the end of the stream (a pipe may return short reads)."""
    parts, got = [], 0
    while got < n:
        b = f.read(n - got)
        if not b:
            break
        parts.append(b)
        got += len(b)
    return parts[0] if len(parts) == 1 else b"".join(parts)


def _read_line(f, what):
    """One ``\\n``-terminated line without the terminator, b"" at a clean end of stream."""
    out = bytearray()
    while True:
        c = f.read(1)
        if not c:
            if out:
                raise ValueError(f"truncated {what}: {bytes(out)[:40]!r}")
            return b""
        if c == b"\n":
            return bytes(out)
        out += c
        if len(out) > _MAX_HEADER:
            raise ValueError(f"{what} longer than {_MAX_HEADER} bytes")


class Y4MReader:
    """Iterates the frames of a YUV4MPEG2 stream (a path or a binary file object; ``"-"`` is not special here)
    as numpy uint8 payloads of ``fmt.frame_bytes`` bytes.  After construction: ``fmt`` (YuvFormat, matrix chosen by
    ``matrix``: "auto" | "bt601" | "bt709"), ``fps`` (Fraction), ``interlace``, ``aspect`` (str or None),
    ``extra_tags`` (the ``X`` tags other than XCOLORRANGE, in order, for passing through), ``range_tagged`` (the
    header had an XCOLORRANGE tag) and ``frames_read``."""

    def __init__(self, src, matrix: str = "auto"):
        self._f, self._own = _open(src, "rb")
        try:
            self._parse_header(matrix)
        except Exception:
            self.close()
            raise
        self.frames_read = 0

    def _parse_header(self, matrix):
        line = _read_line(self._f, "stream header")
        toks = line.decode("ascii", "replace").split(" ")
        if toks[0] != MAGIC.decode():
            raise ValueError(f"not a YUV4MPEG2 stream: starts with {line[:16]!r}")
        w = h = None
        fps, ctag, full = None, "420", False
        self.interlace, self.aspect, self.extra_tags, self.range_tagged = "p", None, [], False
        for t in toks[1:]:
            if not t:
                continue
            k, val = t[0], t[1:]
            if k == "W":
                w = int(val)
            elif k == "H":
                h = int(val)
            elif k == "F":
                num, _, den = val.partition(":")
                if int(num) <= 0 or int(den or 1) <= 0:
                    raise ValueError(f"bad frame rate tag F{val}")
                fps = Fraction(int(num), int(den or 1))
            elif k == "I":
                if val not in ("p", "?"):
                    raise ValueError(f"interlaced streams are not supported: I{val}")
                self.interlace = val
            elif k == "A":
                self.aspect = val
            elif k == "C":
                ctag = val
            elif k == "X":
                if val.startswith("COLORRANGE="):
                    rng = val.split("=", 1)[1]
                    if rng not in ("FULL", "LIMITED"):
                        raise ValueError(f"bad tag X{val}")
                    full, self.range_tagged = rng == "FULL", True
                else:
                    self.extra_tags.append(t)
            else:
                raise ValueError(f"unknown stream header tag {t!r}")
        if w is None or h is None:
            raise ValueError("stream header lacks W or H")
        m = _CTAG.match(ctag)
        if not m:
            raise ValueError(f"unsupported chroma layout C{ctag} (supported: 420jpeg, 420mpeg2, 420paldv, 420, 422, "
                             f"444, each with an optional p10 / p12 / p14 / p16)")
        self.fps = fps if fps is not None else Fraction(25)
        mat = choose_matrix(w, h) if matrix == "auto" else matrix
        self.fmt = YuvFormat(w, h, m.group(1), _DEPTHS[m.group(2) or ""], mat, full)

    def read_frame(self):
        """The next frame's payload (numpy uint8, read-only view of the bytes read), or None at the end."""
        line = _read_line(self._f, "FRAME line")
        if not line:
            return None
        if line != b"FRAME" and not line.startswith(b"FRAME "):
            raise ValueError(f"expected a FRAME line after frame {self.frames_read}, got {line[:16]!r}")
        n = self.fmt.frame_bytes
        data = _read_exact(self._f, n)
        if len(data) != n:
            raise ValueError(f"truncated FRAME {self.frames_read}: {len(data)} of {n} bytes")
        self.frames_read += 1
        return np.frombuffer(data, np.uint8)

    def __iter__(self):
        while True:
            fr = self.read_frame()
            if fr is None:
                return
            yield fr

    def close(self):
        if self._own:
            self._f.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class Y4MWriter:
    """Writes a YUV4MPEG2 stream: the header at construction, then ``write(payload)`` per frame (bytes or a
    uint8 numpy array of ``fmt.frame_bytes`` bytes).  XCOLORRANGE is written for full-range formats (and when
    ``range_tag`` asks for it); ``extra_tags`` are written as given (``X...`` tokens of the input)."""

    def __init__(self, dst, fmt: YuvFormat, fps: Fraction, extra_tags=(), interlace: str = "p", aspect=None,
                 range_tag: bool = False):
        self._f, self._own = _open(dst, "wb")
        self.fmt, self.fps = fmt, Fraction(fps)
        toks = [MAGIC.decode(), f"W{fmt.width}", f"H{fmt.height}",
                f"F{self.fps.numerator}:{self.fps.denominator}", f"I{interlace}"]
        if aspect:
            toks.append(f"A{aspect}")
        toks.append(f"C{fmt.ctag}")
        if fmt.full_range or range_tag:
            toks.append("XCOLORRANGE=" + ("FULL" if fmt.full_range else "LIMITED"))
        for t in extra_tags:
            if not t.startswith("X") or " " in t or "\n" in t:
                raise ValueError(f"extra tags must be single X tokens, got {t!r}")
            toks.append(t)
        self._f.write(" ".join(toks).encode("ascii") + b"\n")
        self.frames_written = 0

    def write(self, payload):
        b = payload.tobytes() if isinstance(payload, np.ndarray) else bytes(payload)
        if len(b) != self.fmt.frame_bytes:
            raise ValueError(f"payload holds {len(b)} bytes, a frame {self.fmt.frame_bytes}")
        self._f.write(b"FRAME\n")
        self._f.write(b)
        self.frames_written += 1

    def close(self):
        if hasattr(self._f, "flush"):
            self._f.flush()
        if self._own:
            self._f.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
