"""Clip intake, host side (numpy, no GPU): walks the markers of baseline JPEG files and packs what csrc/jpeg_dec.hip reads -- the
entropy-coded bytes, per-frame quantisation and Huffman tables, and the table of restart segments (one lane decodes one).

Accepted: SOF0, 8-bit samples, 8-bit quantisation tables, 1 component (grey) or 3 (taken as YCbCr: the first of the frame header is
Y, whatever the ids) with luma sampling 1x1, 2x1 or 2x2 and chroma 1x1, one scan holding all components (Ss = 0, Se = 63,
Ah = Al = 0, components in the frame header's order), Huffman table ids 0 and 1, any restart interval, 0xFF fill bytes before
markers.  Everything else is refused with a ValueError naming the frame and the reason; nothing is guessed."""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35,
                   42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62,
                   63])
SAMPLINGS = ((1, 1), (2, 1), (2, 2))
_SOF_NAMES = {0xC1: "extended sequential (SOF1)", 0xC2: "progressive (SOF2)", 0xC3: "lossless (SOF3)"}


@dataclass
class JpegInfo:
    """One parsed file.  qt [3, 64] uint16 per component in natural order; huff [4, 272] uint8 = (BITS[16], HUFFVAL[256]) of DC id 0,
    DC id 1, AC id 0, AC id 1; sel [4] uint8 = (AC id << 4) | DC id per component; segments = (offset, length, first MCU, MCU count)
    with offsets into the file."""
    height: int
    width: int
    components: int
    hs: int
    vs: int
    restart_interval: int
    qt: np.ndarray
    huff: np.ndarray
    sel: np.ndarray
    segments: List[Tuple[int, int, int, int]]

    @property
    def grid(self) -> Tuple[int, int, int]:
        """(MCU rows, MCU columns, blocks per MCU)."""
        return mcu_grid(self.height, self.width, self.components, self.hs, self.vs)


def mcu_grid(H: int, W: int, components: int, hs: int, vs: int) -> Tuple[int, int, int]:
    return -(-H // (8 * vs)), -(-W // (8 * hs)), (1 if components == 1 else hs * vs + 2)


def _u16(data: bytes, p: int) -> int:
    return (data[p] << 8) | data[p + 1]


def parse_jpeg(data: bytes, frame: int = 0) -> JpegInfo:
    def bad(why: str):
        return ValueError(f"frame {frame}: {why}")

    data = bytes(data)
    n = len(data)
    if n < 4 or data[0] != 0xFF or data[1] != 0xD8:
        raise bad("no SOI marker: not a JPEG file")
    qts, huffs = {}, {}
    sof: Optional[tuple] = None
    ri, adobe_transform = 0, None
    p = 2
    while True:
        if p >= n:
            raise bad("the file ends before a scan (no SOS)")
        if data[p] != 0xFF:
            raise bad(f"byte {p}: expected a marker")
        while p < n and data[p] == 0xFF:                # fill bytes
            p += 1
        if p >= n:
            raise bad("the file ends inside a marker")
        m = data[p]
        p += 1
        if m == 0xD8 or m == 0x01 or 0xD0 <= m <= 0xD7:
            continue
        if m == 0xD9:
            raise bad("EOI before any scan")
        if p + 2 > n:
            raise bad("the file ends inside a segment header")
        L = _u16(data, p)
        if L < 2 or p + L > n:
            raise bad(f"marker FF{m:02X}: its length {L} passes the end of the file")
        body = data[p + 2:p + L]
        if m == 0xC0:
            if sof is not None:
                raise bad("two frame headers")
            if len(body) < 6 or len(body) != 6 + 3 * body[5]:
                raise bad("malformed SOF0")
            if body[0] != 8:
                raise bad(f"{body[0]}-bit samples: only 8-bit baseline is decoded")
            comps = [(body[6 + 3 * i], body[7 + 3 * i] >> 4, body[7 + 3 * i] & 15, body[8 + 3 * i]) for i in range(body[5])]
            sof = (_u16(body, 1), _u16(body, 3), comps)
        elif m in _SOF_NAMES or m in (0xC5, 0xC6, 0xC7):
            raise bad(f"{_SOF_NAMES.get(m, 'differential')} JPEG: only baseline (SOF0) is decoded")
        elif m in (0xC9, 0xCA, 0xCB, 0xCD, 0xCE, 0xCF, 0xCC):
            raise bad("arithmetic coding: only Huffman-coded baseline is decoded")
        elif m == 0xDB:
            q = 0
            while q < len(body):
                pq, tq = body[q] >> 4, body[q] & 15
                if pq != 0:
                    raise bad("16-bit quantisation table (Pq = 1): only 8-bit tables are decoded")
                if tq > 3 or q + 65 > len(body):
                    raise bad("malformed DQT")
                tab = np.zeros(64, dtype=np.uint16)
                tab[ZIGZAG] = np.frombuffer(body, dtype=np.uint8, count=64, offset=q + 1)
                qts[tq] = tab
                q += 65
        elif m == 0xC4:
            q = 0
            while q < len(body):
                if q + 17 > len(body):
                    raise bad("malformed DHT")
                tc, th = body[q] >> 4, body[q] & 15
                bits = list(body[q + 1:q + 17])
                count = sum(bits)
                if tc > 1 or th > 1:
                    raise bad(f"Huffman table class {tc} id {th}: baseline has classes 0, 1 and ids 0, 1")
                if q + 17 + count > len(body) or count > 256:
                    raise bad("malformed DHT")
                space = 0                               # Kraft sum in units of 2^-16; the all-ones code stays free in a legal table
                for length, c in enumerate(bits, 1):
                    space += c << (16 - length)
                if space > 1 << 16:
                    raise bad(f"Huffman table class {tc} id {th}: its BITS list over-subscribes the code space")
                if tc == 0 and count > 16:
                    raise bad(f"DC Huffman table id {th} lists {count} symbols: baseline has 12 categories")
                tab = np.zeros(272, dtype=np.uint8)
                tab[:16] = bits
                tab[16:16 + count] = np.frombuffer(body, dtype=np.uint8, count=count, offset=q + 17)
                huffs[(tc, th)] = tab
                q += 17 + count
        elif m == 0xDD:
            if len(body) != 2:
                raise bad("malformed DRI")
            ri = _u16(body, 0)
        elif m == 0xEE and body[:5] == b"Adobe" and len(body) >= 12:
            adobe_transform = body[11]
        elif m == 0xDA:
            break
        # APPn, COM and anything else with a length: skipped
        p += L
    if sof is None:
        raise bad("SOS before a frame header (SOF0)")
    H, W, comps = sof
    if H == 0 or W == 0:
        raise bad(f"H = {H}, W = {W}: a size of 0 (DNL-defined height included) is not decoded")
    nc = len(comps)
    if nc not in (1, 3):
        raise bad(f"{nc} components: 1 (grey) or 3 (YCbCr) are decoded")
    if nc == 3 and adobe_transform == 0:
        raise bad("Adobe APP14 with transform 0 (RGB or CMYK samples, not YCbCr)")
    if nc == 1:
        hs = vs = 1                                     # a single component is never interleaved: its factors do not matter
    else:
        hs, vs = comps[0][1], comps[0][2]
        if (hs, vs) not in SAMPLINGS or any((c[1], c[2]) != (1, 1) for c in comps[1:]):
            raise bad("sampling factors " + ", ".join(f"{c[1]}x{c[2]}" for c in comps) + ": luma 1x1, 2x1 or 2x2 with chroma 1x1 is decoded")
    if len(body) < 1 or len(body) != 4 + 2 * body[0]:
        raise bad("malformed SOS")
    if body[0] != nc:
        raise bad(f"a scan of {body[0]} of the {nc} components: several scans are not decoded")
    if [body[1 + 2 * i] for i in range(nc)] != [c[0] for c in comps]:
        raise bad("the scan's components are not the frame header's, in its order")
    ss, se, aa = body[1 + 2 * nc], body[2 + 2 * nc], body[3 + 2 * nc]
    if (ss, se, aa) != (0, 63, 0):
        raise bad(f"scan parameters Ss = {ss}, Se = {se}, Ah/Al = {aa:#x}: a baseline scan has 0, 63, 0")
    qt = np.zeros((3, 64), dtype=np.uint16)
    huff = np.zeros((4, 272), dtype=np.uint8)
    sel = np.zeros(4, dtype=np.uint8)
    for i, c in enumerate(comps):
        if c[3] not in qts:
            raise bad(f"quantisation table {c[3]} is referenced but never defined")
        qt[i] = qts[c[3]]
        td, ta = body[2 + 2 * i] >> 4, body[2 + 2 * i] & 15
        if td > 1 or ta > 1:
            raise bad(f"Huffman table ids {td} / {ta}: baseline has ids 0 and 1")
        for tc, th in ((0, td), (1, ta)):
            if (tc, th) not in huffs:
                raise bad(f"Huffman table class {tc} id {th} is referenced but never defined")
            huff[2 * tc + th] = huffs[(tc, th)]
        sel[i] = (ta << 4) | td
    if nc == 1:
        qt[1:] = 1

    rows, cols, _ = mcu_grid(H, W, nc, hs, vs)
    total = rows * cols
    start = p + L
    a = np.frombuffer(data, dtype=np.uint8, offset=start)
    marks = np.flatnonzero((a[:-1] == 0xFF) & (a[1:] != 0) & (a[1:] != 0xFF)) if a.size > 1 else np.zeros(0, dtype=np.int64)
    codes = a[marks + 1]
    other = np.flatnonzero((codes < 0xD0) | (codes > 0xD7))
    if other.size == 0:
        raise bad("no EOI marker after the scan")
    last = int(other[0])
    if codes[last] != 0xD9:
        raise bad(f"marker FF{int(codes[last]):02X} after the scan: several scans or tables between scans are not decoded")
    rst, ends = codes[:last], marks[:last + 1]
    per = ri if ri > 0 else total
    nseg = -(-total // per)
    if ri == 0 and rst.size:
        raise bad("a restart marker without a restart interval (DRI absent or 0)")
    if rst.size != nseg - 1:
        raise bad(f"{rst.size} restart markers where {total} MCUs at an interval of {per} need {nseg - 1}")
    if rst.size and not np.array_equal(rst, 0xD0 + (np.arange(rst.size) & 7)):
        k = int(np.flatnonzero(rst != 0xD0 + (np.arange(rst.size) & 7))[0])
        raise bad(f"restart marker {k} is RST{int(rst[k]) - 0xD0}, out of sequence (RST{k & 7} expected)")
    segments, begin = [], 0
    for i in range(nseg):
        end = int(ends[i])
        while end > begin and a[end - 1] == 0xFF:       # fill bytes before the marker
            end -= 1
        segments.append((start + begin, end - begin, i * per, min(per, total - i * per)))
        begin = int(ends[i]) + 2
    return JpegInfo(H, W, nc, hs, vs, ri, qt, huff, sel, segments)


@dataclass
class PackedJpegs:
    """What one decode call reads, as host arrays: data uint8 [nbytes] (entropy bytes of all frames, still stuffed), qt uint16
    [T, 3, 64], huff uint8 [T, 4, 272], sel uint8 [T, 4], segs int32 [S, 5] = byte offset into data, byte length, frame, first MCU,
    MCU count."""
    frames: int
    height: int
    width: int
    components: int
    hs: int
    vs: int
    data: np.ndarray
    qt: np.ndarray
    huff: np.ndarray
    sel: np.ndarray
    segs: np.ndarray

    @property
    def grid(self) -> Tuple[int, int, int]:
        return mcu_grid(self.height, self.width, self.components, self.hs, self.vs)


def split_segments(pk: PackedJpegs, sub_bytes: int) -> np.ndarray:
    """The split table of csrc/jpeg_dec.hip's parallel entropy route: int32 [nsub, 3] = (segment, byte offset inside the segment,
    byte length).  Every segment of at least 4 * sub_bytes is cut at the multiples of sub_bytes from its start (the last row takes
    the remainder, so it is shorter than 2 * sub_bytes); a cut that lands on a stuffing 00 (the byte before it is FF) moves one byte
    on, so no row starts on one.  Shorter segments get no rows: they decode serially.  sub_bytes: a multiple of 4, at least 8 (a
    symbol with its amplitude is at most 26 bits, so every row holds a symbol boundary)."""
    if isinstance(sub_bytes, bool) or not isinstance(sub_bytes, (int, np.integer)) or sub_bytes < 8 or sub_bytes % 4:
        raise ValueError(f"split_segments: sub_bytes={sub_bytes!r} must be a multiple of 4, at least 8")
    sub = int(sub_bytes)
    lens = pk.segs[:, 1].astype(np.int64)
    n = np.where(lens >= 4 * sub, lens // sub, 0)
    total = int(n.sum())
    if total == 0:
        return np.zeros((0, 3), dtype=np.int32)
    seg = np.repeat(np.arange(len(n), dtype=np.int64), n)
    j = np.arange(total, dtype=np.int64) - np.repeat(np.cumsum(n) - n, n)
    at = pk.segs[seg, 0].astype(np.int64) + j * sub
    off = j * sub + ((j > 0) & (pk.data[at] == 0) & (pk.data[np.maximum(at - 1, 0)] == 0xFF))
    end = np.append(off[1:], 0)
    last = j == n[seg] - 1
    end[last] = lens[seg][last]
    return np.stack([seg, off, end - off], 1).astype(np.int32)


def pack_jpegs(files: Sequence[bytes]) -> PackedJpegs:
    if len(files) < 1:
        raise ValueError("pack_jpegs: no frames")
    infos = [parse_jpeg(f, t) for t, f in enumerate(files)]
    first = infos[0]
    key = lambda i: (i.height, i.width, i.components, i.hs, i.vs)      # noqa: E731
    for t, info in enumerate(infos):
        if key(info) != key(first):
            raise ValueError(f"frame {t}: {info.width}x{info.height}, {info.components} components, luma sampling {info.hs}x{info.vs} "
                             f"differs from frame 0 ({first.width}x{first.height}, {first.components}, {first.hs}x{first.vs})")
    chunks, rows, pos = [], [], 0
    for t, (info, f) in enumerate(zip(infos, files)):
        lo = info.segments[0][0]
        hi = info.segments[-1][0] + info.segments[-1][1]
        chunks.append(np.frombuffer(bytes(f), dtype=np.uint8, count=hi - lo, offset=lo))
        rows += [(pos + off - lo, length, t, m0, mc) for off, length, m0, mc in info.segments]
        pos += hi - lo
    if pos > 0x7FFFFFFF:
        raise ValueError(f"pack_jpegs: {pos} bytes of entropy data are more than one call covers (2^31 - 1)")
    data = np.concatenate(chunks) if pos else np.zeros(0, dtype=np.uint8)
    return PackedJpegs(len(files), first.height, first.width, first.components, first.hs, first.vs, data,
                       np.stack([i.qt for i in infos]), np.stack([i.huff for i in infos]), np.stack([i.sel for i in infos]),
                       np.array(rows, dtype=np.int32).reshape(-1, 5))
