"""YUV4MPEG2 (.y4m) streams on the host: a text header line, then `FRAME\\n` + raw planes per frame ("Planar YUV
and Y4M").  The format has no size limit, carries its frame rate, and is the bridge to every codec:

    ffmpeg -i out.y4m out.mp4                           (encode what write_y4m wrote)
    ffmpeg -i any.mp4 -f yuv4mpegpipe clip.y4m          (turn any footage into what Y4MReader reads; the target may be a FIFO)

Nothing here needs torch: payloads are bytes, the device side is ops.cl_to_yuv420 / ops.frames_u8_to_yuv420 (out) and
ops.yuv_to_frames_u8 (in)."""
from __future__ import annotations

import collections
from fractions import Fraction
from typing import Iterable, Iterator, List, Optional

MAGIC = b"YUV4MPEG2"
RANGES = ("limited", "full")
# header C tag -> layout name of ops.yuv_to_frames_u8 (ops.YUV_LAYOUTS); a bare C420 is C420jpeg, no C tag at all is 4:2:0 too
LAYOUT_OF_TAG = {"420jpeg": "420jpeg", "420": "420jpeg", "420mpeg2": "420mpeg2", "420paldv": "420paldv", "422": "422", "444": "444",
                 "mono": "mono"}
MAX_LINE = 4096      # a header or FRAME line longer than this is not one


def chroma_shape(layout: str, H: int, W: int):
    """(Hc, Wc) of a layout's chroma planes; (0, 0) for mono."""
    if layout == "mono":
        return 0, 0
    return (H if layout in ("422", "444") else (H + 1) // 2), (W if layout == "444" else (W + 1) // 2)


def frame_bytes(layout: str, H: int, W: int) -> int:
    """Payload bytes of one frame: the Y plane, then Cb, then Cr."""
    hc, wc = chroma_shape(layout, H, W)
    return H * W + 2 * hc * wc


def _fraction(value, what: str) -> Fraction:
    if isinstance(value, bool):
        raise ValueError(f"{what}: {value!r} is not a frame rate")
    try:
        if isinstance(value, (tuple, list)) and len(value) == 2:
            return Fraction(int(value[0]), int(value[1]))
        if isinstance(value, str) and ":" in value:
            num, den = value.split(":")
            return Fraction(int(num), int(den))
        return Fraction(value)
    except (ValueError, TypeError, ZeroDivisionError):
        raise ValueError(f"{what}: {value!r} is not a frame rate") from None


def write_y4m(path, frames_bytes_iter: Iterable, W: int, H: int, fps=Fraction(16), range: str = "limited") -> int:
    """Write I420 payloads (bytes-like, frame_bytes("420jpeg", H, W) each: a row of the device buffer's host copy) as a .y4m, frame by
    frame, and return the file's size in bytes.  `path` may be an open binary file."""
    if range not in RANGES:
        raise ValueError(f"range: {range!r} is not one of {', '.join(RANGES)}")
    rate = _fraction(fps, "fps")
    if rate <= 0:
        raise ValueError(f"fps: {fps!r} must be positive")
    if int(W) < 1 or int(H) < 1:
        raise ValueError(f"W, H: {W!r} x {H!r} is not a frame size")
    want = frame_bytes("420jpeg", int(H), int(W))
    header = f"YUV4MPEG2 W{int(W)} H{int(H)} F{rate.numerator}:{rate.denominator} Ip A1:1 C420jpeg XCOLORRANGE={range.upper()}\n"
    f = open(path, "wb") if isinstance(path, (str, bytes)) or hasattr(path, "__fspath__") else path
    size = 0
    try:
        f.write(header.encode("ascii"))
        size += len(header)
        for k, payload in enumerate(frames_bytes_iter):
            data = memoryview(payload).cast("B") if not isinstance(payload, (bytes, bytearray)) else payload
            if len(data) != want:
                raise ValueError(f"frame {k}: {len(data)} bytes, a {W}x{H} I420 frame holds {want}")
            f.write(b"FRAME\n")
            f.write(data)
            size += 6 + want
    finally:
        if f is not path:
            f.close()
    return size


class Y4MReader:
    """Strictly sequential reader (a FIFO works): `for payload in reader` yields each frame's packed planes as bytes.

    width, height, layout (a name of ops.YUV_LAYOUTS), fps (Fraction, or None for F0:0 / no F tag; rate() refuses that), interlace,
    aspect, range ("limited" | "full": the XCOLORRANGE tag, else `input_range`, else limited), tags (every header token), frame_bytes,
    frames_read.  Refused with a ValueError naming the tag: a missing magic, W or H, interlaced streams (It, Ib, Im), a C value outside
    the six layouts (C420p10, C444alpha, ...), a payload shorter than the header promises (at which frame)."""

    def __init__(self, path_or_file, input_range: Optional[str] = None):
        if input_range is not None and input_range not in RANGES:
            raise ValueError(f"input_range: {input_range!r} is not one of {', '.join(RANGES)}")
        self._own = isinstance(path_or_file, (str, bytes)) or hasattr(path_or_file, "__fspath__")
        self._f = open(path_or_file, "rb") if self._own else path_or_file
        self.frames_read = 0
        try:
            self._parse(self._line("the header"), input_range)
        except Exception:
            self.close()
            raise

    def _line(self, what: str) -> Optional[bytes]:
        """One line without its newline; None at a clean end of the stream."""
        out = bytearray()
        while True:
            c = self._f.read(1)
            if not c:
                if not out:
                    return None
                raise ValueError(f"y4m: the stream ends inside {what}")
            if c == b"\n":
                return bytes(out)
            out += c
            if len(out) > MAX_LINE:
                raise ValueError(f"y4m: {what} is longer than {MAX_LINE} bytes: YUV4MPEG2 magic not found" if what == "the header"
                                 else f"y4m: {what} is longer than {MAX_LINE} bytes")

    def _parse(self, line: Optional[bytes], input_range: Optional[str]) -> None:
        tokens = (line or b"").split(b" ")
        if not line or tokens[0] != MAGIC:
            raise ValueError(f"y4m: the stream does not start with the YUV4MPEG2 magic (got {bytes(line or b'')[:16]!r})")
        self.tags = [t.decode("ascii", "replace") for t in tokens[1:] if t]
        self.width = self.height = None
        self.fps, self.interlace, self.aspect, ctag, xrange = None, "p", None, None, None
        for tag in self.tags:
            key, val = tag[0], tag[1:]
            if key in "WH":
                if not val.isdigit() or int(val) < 1:
                    raise ValueError(f"y4m: {key} tag {tag!r} is not a positive size")
                if key == "W":
                    self.width = int(val)
                else:
                    self.height = int(val)
            elif key == "F":
                parts = val.split(":")
                if len(parts) != 2 or not all(p.isdigit() for p in parts):
                    raise ValueError(f"y4m: F tag {tag!r} is not num:den")
                num, den = int(parts[0]), int(parts[1])
                self.fps = Fraction(num, den) if num > 0 and den > 0 else None
            elif key == "I":
                if val not in ("p", "?"):
                    raise ValueError(f"y4m: I tag {tag!r}: interlaced streams (It, Ib, Im) are not read, only progressive ones (Ip)")
                self.interlace = val
            elif key == "A":
                self.aspect = val
            elif key == "C":
                ctag = val
            elif key == "X" and val.upper().startswith("COLORRANGE="):
                xrange = val.split("=", 1)[1].lower()
                if xrange not in RANGES:
                    raise ValueError(f"y4m: X tag {tag!r}: XCOLORRANGE is LIMITED or FULL")
        for key, got in (("W", self.width), ("H", self.height)):
            if got is None:
                raise ValueError(f"y4m: the header has no {key} tag")
        if ctag is not None and ctag not in LAYOUT_OF_TAG:
            raise ValueError(f"y4m: C tag 'C{ctag}' is not one of the layouts read ({', '.join('C' + t for t in LAYOUT_OF_TAG)}); "
                             f"10-bit and alpha layouts such as C420p10 or C444alpha are not")
        self.layout = LAYOUT_OF_TAG[ctag or "420"]
        self.range = xrange or input_range or "limited"
        self.frame_bytes = frame_bytes(self.layout, self.height, self.width)

    def rate(self) -> Fraction:
        """The header's frame rate; a stream without one (F0:0, or no F tag) is refused."""
        if self.fps is None:
            raise ValueError("y4m: the header's rate is F0:0 (unknown): a rate is needed to select frames by rate")
        return self.fps

    def __iter__(self) -> Iterator[bytes]:
        while True:
            line = self._line(f"the FRAME line of frame {self.frames_read}")
            if line is None:
                return
            if line != b"FRAME" and not line.startswith(b"FRAME "):            # parameters on a FRAME line are tolerated
                raise ValueError(f"y4m: frame {self.frames_read}: expected a FRAME line, got {line[:16]!r}")
            data = self._f.read(self.frame_bytes)
            while len(data) < self.frame_bytes:                                 # a pipe hands over what it has
                more = self._f.read(self.frame_bytes - len(data))
                if not more:
                    raise ValueError(f"y4m: frame {self.frames_read}: the payload holds {len(data)} bytes, the header promises "
                                     f"{self.frame_bytes} ({self.width}x{self.height} C{self.layout})")
                data += more
            self.frames_read += 1
            yield data

    def read_last(self, n: Optional[int] = None) -> List[bytes]:
        """Read to the end of the stream and return its last n payloads (all of them for None): only a ring of n frames is ever held.
        frames_read then counts the whole stream."""
        if n is not None and (isinstance(n, bool) or int(n) < 1):
            raise ValueError(f"read_last: n={n!r} must be an integer >= 1")
        ring = collections.deque(maxlen=None if n is None else int(n))
        for payload in self:
            ring.append(payload)
        return list(ring)

    def close(self) -> None:
        if self._own and self._f is not None:
            self._f.close()
        self._f = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _rnd(x: Fraction) -> int:
    return (2 * x.numerator + x.denominator) // (2 * x.denominator)          # floor(x + 1/2), exact


def select_frames_at_rate(total: int, src_fps, dst_fps=16, cap: Optional[int] = None) -> List[int]:
    """Which frames of a `total`-frame clip at src_fps are continued at dst_fps: output frame j, counted back from the clip's last frame,
    is source frame last - rnd(j src / dst) -- the END of the clip is what gets continued.  1 + 4k indices with the largest k that
    fits the clip and the cap, ascending.  src >= dst never repeats an index (frames are dropped); src < dst repeats some
    (duplication, as ffmpeg's fps filter does); equal rates give cli.select_clip_frames."""
    if isinstance(total, bool) or not isinstance(total, int) or total < 1:
        raise ValueError(f"input_video: the clip holds {total!r} frames, at least 1 is needed")
    src, dst = _fraction(src_fps, "src_fps"), _fraction(dst_fps, "dst_fps")
    if src <= 0 or dst <= 0:
        raise ValueError(f"input_rate: rates {src_fps!r} -> {dst_fps!r} must be positive")
    if cap is not None and (isinstance(cap, bool) or not isinstance(cap, int) or cap < 1):
        raise ValueError(f"input_frames: {cap!r} must be an integer >= 1")
    step, last = src / dst, total - 1
    fit = (last * dst.numerator * src.denominator) // (src.numerator * dst.denominator) + 1      # a lower bound on the frames that fit
    while _rnd(fit * step) <= last:
        fit += 1
    while fit > 1 and _rnd((fit - 1) * step) > last:
        fit -= 1
    room = fit if cap is None else min(fit, cap)
    used = 1 + 4 * ((room - 1) // 4)
    return [last - _rnd(j * step) for j in range(used - 1, -1, -1)]


def frames_spanned(count: int, src_fps, dst_fps=16) -> int:
    """How many trailing source frames select_frames_at_rate can touch when it returns `count` indices (the ring a reader keeps)."""
    return _rnd((count - 1) * (_fraction(src_fps, "src_fps") / _fraction(dst_fps, "dst_fps"))) + 1
