"""Restatement of the split route through the entropy stage (csrc/jpeg_dec.h: jd_sub_scan / jd_sub_emit and the speculation policy;
csrc/jpeg_dec.hip: pass 0, the rounds, block scan, emit, DC pass; longlive_amd/jpeg_files.py: split_segments) in plain Python over bit
strings, in the style of tests/jpeg_dec_ref.py, whose header parser and code tables it uses.  Nothing is shared with the library.

A state is (bit position in the DE-STUFFED segment, block index inside the MCU, next coefficient with 0 = DC), or END once a bit
past the data was consumed.  A raw byte offset that is no stuffing byte maps to one de-stuffed byte, so the library's canonical
(raw offset, bit) positions and these bit positions order and compare alike."""
import bisect

import numpy as np

import jpeg_dec_ref as D
import jpeg_ref as J

END = ("end",)


def raw_segments(data: bytes):
    """The scan's restart segments as they lie in the file, still stuffed, without the fill bytes before a marker."""
    p = 2
    while True:
        while data[p] == 0xFF:
            p += 1
        m, p = data[p], p + 1
        L = int.from_bytes(data[p:p + 2], "big")
        p += L
        if m == 0xDA:
            break
    segs, begin = [], p
    while True:
        q = data.index(b"\xff", p)
        nxt = data[q + 1]
        if nxt == 0:
            p = q + 2
            continue
        end = q
        while data[q + 1] == 0xFF:
            q += 1
        segs.append(data[begin:end])
        if data[q + 1] == 0xD9:
            return segs
        assert 0xD0 <= data[q + 1] <= 0xD7
        begin = p = q + 2


def split_table(segs, sub: int):
    """[(segment, byte offset, byte length)]: segments of at least 4 * sub bytes cut at multiples of sub, a cut on a stuffing 00
    moved one byte on, the last row taking the remainder."""
    assert sub >= 8 and sub % 4 == 0
    rows = []
    for s, raw in enumerate(segs):
        if len(raw) < 4 * sub:
            continue
        cuts = [0]
        for j in range(1, len(raw) // sub):
            c = j * sub
            cuts.append(c + 1 if raw[c] == 0 and raw[c - 1] == 0xFF else c)
        cuts.append(len(raw))
        rows += [(s, a, b - a) for a, b in zip(cuts, cuts[1:])]
    return rows


def nominal_cuts_on_stuffing(segs, sub: int) -> int:
    """How many nominal cuts (multiples of sub) of the split segments land on a stuffing byte."""
    return sum(1 for raw in segs if len(raw) >= 4 * sub for j in range(1, len(raw) // sub) if raw[j * sub] == 0 and raw[j * sub - 1] == 0xFF)


def textured(H: int, W: int, seed: int = 0) -> np.ndarray:
    """Smooth content under a quarter of white noise: what busy footage looks like to the coder."""
    return (0.75 * J.smooth_noise(H, W, seed) + 0.25 * J.noise(H, W, seed + 1)).astype(np.uint8)


def _specs() -> dict:
    """name -> (Image -> files of one clip, subsequence size in bytes, rounds).  Pillow files of every sampling without DRI (optimised
    tables, grey); noise, textured and flat content, 40 x 56 to 96 x 136; files with a DRI of 3 blocks, whose segments are all too
    short to cut; this project's own files; a clip that mixes frames with different Huffman tables.  The rounds leave room over what
    the restatement needs (measured with Pillow 12.2: at most 29 of 64 at 8 bytes, 31 of 64 at 16, 10 of 16 at 64 and 512; noise
    at quality 90 in 8-byte subsequences needs 146, because a block without EOB gives a wrong coefficient index nothing to settle
    on, hence quality 30); test_jpeg_split_host.py asserts that it settles, so that a fallback cannot hide a wrong split route."""
    out = {}
    for s in D.PIL_SAMPLINGS:
        out[f"noise_40x56_{s}_sub8"] = (lambda Image, s=s: [D.pil_file(Image, J.noise(40, 56, 3), s, quality=30)], 8, 64)
        out[f"noise_56x72_{s}_opt_sub16"] = (lambda Image, s=s: [D.pil_file(Image, J.noise(56, 72, 4), s, quality=30, optimize=True)], 16, 64)
        out[f"textured_96x136_{s}_sub64"] = (lambda Image, s=s: [D.pil_file(Image, textured(96, 136, 5), s, quality=90, optimize=(s == 1))], 64, 16)
        out[f"flat_96x136_{s}_sub8"] = (lambda Image, s=s: [D.pil_file(Image, J.flat(96, 136), s, quality=95)], 8, 64)
    out["noise_96x136_0_sub512"] = (lambda Image: [D.pil_file(Image, J.noise(96, 136, 6), 0, quality=95)], 512, 16)
    out["restart3_72x88_sub512"] = (lambda Image: [D.pil_file(Image, J.noise(72, 88, 7), 2, quality=95, restart_marker_blocks=3)], 512, 12)
    out["own_64x96_sub16"] = (lambda Image: [J.encode(textured(64, 96, s), q) for s, q in ((8, 90), (9, 50))], 16, 64)
    frames = [J.smooth_noise(48, 80, 1), J.noise(48, 80, 2), J.flat(48, 80), textured(48, 80, 3)]
    kws = [dict(quality=30), dict(quality=60, optimize=True), dict(quality=75, restart_marker_blocks=2), dict(quality=60, optimize=True)]
    out["mixed_tables_48x80_sub16"] = (lambda Image: [D.pil_file(Image, f, 1, **kw) for f, kw in zip(frames, kws)], 16, 64)
    return out


def clip_names():
    return sorted(_specs())


def clips(Image) -> dict:
    """name -> (files of one clip, subsequence size in bytes, rounds)."""
    return {name: (make(Image), sub, rounds) for name, (make, sub, rounds) in _specs().items()}


STUFFED = "noise_40x56_0_sub8"                       # a nominal cut of this clip lands on a stuffing byte


UNSETTLED = "noise_40x56_2_sub8"                      # with rounds = 1 the restatement leaves this clip's segment unsettled


class Segment:
    """One segment: its de-stuffed bits and the walk that scan and emit share."""

    def __init__(self, raw: bytes, info: dict):
        self.raw = raw
        self.stuff = [i + 1 for i in range(len(raw) - 1) if raw[i] == 0xFF and raw[i + 1] == 0]      # raw offsets of the stuffing bytes
        self.bits = "".join(format(b, "08b") for b in raw.replace(b"\xff\x00", b"\xff"))
        self.padded = self.bits + "1" * 16
        self.bpm = D.grid(info)[2]
        self.ny = 1 if self.bpm == 1 else self.bpm - 2
        self.dc = [{code: sym for sym, code in J.huffman_codes(*t).items()} for t in info["dc"]]
        self.ac = [{code: sym for sym, code in J.huffman_codes(*t).items()} for t in info["ac"]]
        self.memo = {}

    def bit_of(self, raw_offset: int) -> int:
        assert raw_offset not in self.stuff
        return 8 * (raw_offset - bisect.bisect_left(self.stuff, raw_offset))

    def _symbol(self, inv, pos):
        for n in range(1, 17):
            sym = inv.get(self.padded[pos:pos + n])
            if sym is not None:
                return sym, n
        return None, 16

    def walk(self, entry, end=None, count=None):
        """end given: the scan -> (exit, blocks begun, dirty).  count given: the emit -> `count` blocks of 64 (DC = the difference)."""
        scan = end is not None
        if entry == END:
            assert scan
            return END, 0, False
        pos, bi, k = entry
        s, n = self.bits, len(self.bits)
        begun, dirty, blocks, cur, storing = 0, False, [], None, k == 0
        if not scan and count == 0:
            return []
        while True:
            if scan:
                if pos >= end:
                    return (pos, bi, k), begun, dirty
            elif k == 0 and storing and len(blocks) >= count:
                return blocks
            c = 0 if bi < self.ny else bi - self.ny + 1
            sym, L = self._symbol(self.dc[c] if k == 0 else self.ac[c], pos)
            over = n - pos < L
            resync = endblk = False
            if over:
                pass
            elif sym is None or (k == 0 and sym > 11):
                resync = True
            elif k == 0:
                if n - pos - L < sym:
                    over = True
                else:
                    diff = D._extend(int(s[pos + L:pos + L + sym], 2), sym) if sym else 0
                    pos += L + sym
                    begun += 1
                    if storing:
                        cur = [0] * 64
                        cur[0] = diff
                    k = 1
            else:
                pos += L
                r, size = sym >> 4, sym & 15
                if size == 0:
                    if r == 0:
                        endblk = True
                    elif r != 15 or k + 16 > 64:
                        dirty = endblk = True
                    else:
                        k += 16
                else:
                    if size > 10:
                        dirty = True
                    if k + r > 63:
                        dirty = endblk = True
                    elif n - pos < size:
                        over = True
                    else:
                        k += r
                        if storing:
                            cur[k] = D._extend(int(s[pos:pos + size], 2), size)
                        pos += size
                        k += 1
                if k >= 64:
                    endblk = True
            if over:
                assert scan, "the emit ran past the data"
                return END, begun, dirty
            if resync:
                dirty, pos, bi, k, storing = True, pos + 1, 0, 0, True
            elif endblk:
                if not scan and storing:
                    blocks.append(cur)
                storing, bi, k = True, (bi + 1) % self.bpm, 0
            assert scan or not dirty, "the emit met an event of the speculation policy"

    def scan(self, entry, end):
        key = (entry, end)
        if key not in self.memo:
            self.memo[key] = self.walk(entry, end=end)
        return self.memo[key]


def settle(seg: Segment, rows, cap: int = 1000):
    """The rounds over one segment's rows [(offset, length)]: (round in which it settles, final entries, final scans).  Pass 0 scans
    every subsequence from the guess (its first byte, block 0, DC); round r rescans subsequence i from the exit i - 1 held after round
    r - 1; the segment settles in the first round in which no exit changes."""
    ends = [seg.bit_of(o + n) if o + n < len(seg.raw) else len(seg.bits) for o, n in rows]
    entries = [(seg.bit_of(o), 0, 0) for o, _ in rows]
    res = [seg.scan(e, end) for e, end in zip(entries, ends)]
    for r in range(1, cap + 1):
        entries = [entries[0]] + [x[0] for x in res[:-1]]
        new = [seg.scan(e, end) for e, end in zip(entries, ends)]
        changed = any(a[0] != b[0] for a, b in zip(new, res))
        res = new
        if not changed:
            return r, entries, res
    raise AssertionError(f"not settled after {cap} rounds")


def decode(data: bytes, sub: int):
    """(info, coefficients int16 [rows, cols, bpm, 64] through the split route, settle round per segment with 0 = no rows, split table).
    Segments without rows are taken from the serial restatement."""
    info = D.parse(data)
    rows_, cols, bpm = D.grid(info)
    ny = 1 if bpm == 1 else bpm - 2
    raws = raw_segments(data)
    table = split_table(raws, sub)
    serial = D.coefficients(data)[1].reshape(rows_ * cols, bpm, 64)
    out = np.zeros_like(serial)
    per = info["ri"] or rows_ * cols
    rounds = []
    for s, raw in enumerate(raws):
        m0, mc = s * per, min(per, rows_ * cols - s * per)
        mine = [(o, n) for g, o, n in table if g == s]
        if not mine:
            out[m0:m0 + mc] = serial[m0:m0 + mc]
            rounds.append(0)
            continue
        seg = Segment(raw, info)
        r, entries, res = settle(seg, mine)
        rounds.append(r)
        assert not any(d for _, _, d in res) and sum(b for _, b, _ in res) == mc * bpm, "a valid segment was flagged"
        blocks = [blk for e, (_, b, _) in zip(entries, res) for blk in seg.walk(e, count=b)]
        pred = [0, 0, 0]
        for j, blk in enumerate(blocks):
            c = 0 if j % bpm < ny else j % bpm - ny + 1
            pred[c] += blk[0]
            assert -32768 <= pred[c] <= 32767
            out[m0 + j // bpm, j % bpm] = [pred[c]] + blk[1:]
    return info, out.reshape(rows_, cols, bpm, 64), rounds, table
