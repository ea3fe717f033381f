"""The PNG encoder of csrc/png.hip and csrc/png.h restated in numpy / Python, bit for bit: filter choice, span cutter, code lengths and
their limiting, the block writer with its stored fallback and sync blocks, the container, CRC-32 and Adler-32.  It is the expected
value of the GPU tests and is itself checked by decoders this project did not write (zlib.decompress, PIL) in test_png_host.py."""
import struct
import zlib

import numpy as np

CHUNK = 16384
LITLEN = 286
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
SIGNATURE = b"\x89PNG\r\n\x1a\n"


# ---- filter -------------------------------------------------------------------------------------------------------------------------
def filter_frames(frames):
    """uint8 [T, H, W, 3] -> uint8 [T, H, 1 + 3W]: per row the type with the smallest sum of min(b, 256 - b), the lower type on a tie."""
    frames = np.asarray(frames)
    T, H, W, _ = frames.shape
    x = frames.reshape(T, H, 3 * W).astype(np.int64)
    a = np.zeros_like(x)
    a[:, :, 3:] = x[:, :, :-3]
    b = np.zeros_like(x)
    b[:, 1:] = x[:, :-1]
    c = np.zeros_like(x)
    c[:, 1:, 3:] = x[:, :-1, :-3]
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    forms = np.stack([x, x - a, x - b, x - ((a + b) >> 1), x - paeth]) & 255                # [5, T, H, 3W]
    cost = np.minimum(forms, 256 - forms).sum(-1)                                            # [5, T, H]
    kind = cost.argmin(0)                                                                    # first minimum: the lower type
    chosen = np.take_along_axis(forms, kind[None, ..., None], 0)[0]
    return np.concatenate([kind[..., None], chosen], -1).astype(np.uint8)


# ---- parse --------------------------------------------------------------------------------------------------------------------------
def span_token(k, L):
    """Position k of a span of L repeats: ("none" | "lit" | "match", length)."""
    k0 = k - k % 258
    piece = min(258, L - k0)
    if piece < 3:
        return "lit", 0
    return ("match", piece) if k == k0 else ("none", 0)


LENGTH_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LENGTH_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)


def length_symbol(n):
    """RFC 1951's table: (symbol, extra bits, extra value) of a match length."""
    if n == 258:
        return 285, 0, 0
    i = max(j for j in range(28) if LENGTH_BASE[j] <= n)
    return 257 + i, LENGTH_EXTRA[i], n - LENGTH_BASE[i]


_LEN_SYM = np.array([0, 0, 0] + [length_symbol(n)[0] for n in range(3, 259)])
_LEN_EB = np.array([0, 0, 0] + [length_symbol(n)[1] for n in range(3, 259)])
_LEN_EV = np.array([0, 0, 0] + [length_symbol(n)[2] for n in range(3, 259)])


def tokens(chunk, prev):
    """The chunk's tokens in order: (symbols, match lengths (0 for a literal)).  `prev` is the byte before the chunk, or None."""
    d = np.asarray(chunk, dtype=np.int64)
    n = d.size
    rep = np.zeros(n, bool)
    rep[1:] = d[1:] == d[:-1]
    rep[0] = prev is not None and d[0] == prev
    idx = np.arange(n)
    start = np.maximum.accumulate(np.where(~rep, idx, -1)) + 1              # first position of the span a repeat is in
    end = np.minimum.accumulate(np.where(~rep, idx, n)[::-1])[::-1]         # the next position that is no repeat
    k, L = idx - start, end - start
    k0 = k - k % 258
    piece = np.minimum(258, L - k0)
    lit = ~rep | (piece < 3)
    match = rep & (piece >= 3) & (k == k0)
    keep = lit | match
    mlen = np.where(match, piece, 0)[keep]
    sym = np.where(mlen > 0, _LEN_SYM[mlen], d[keep])
    return sym, mlen


# ---- code lengths -------------------------------------------------------------------------------------------------------------------
def code_lengths(count, maxbits):
    """Lengths of a length-limited prefix code: symbols sorted by (count, index), a two-queue merge with the leaf queue first on equal
    weight, nodes deeper than `maxbits` held there and folded back as zlib's gen_bitlen does, lengths handed out along the sorted order."""
    count = [int(c) for c in count]
    order = sorted((i for i in range(len(count)) if count[i]), key=lambda i: (count[i], i))
    lens = [0] * len(count)
    used = len(order)
    if used == 0:
        return lens
    if used == 1:
        lens[order[0]] = 1
        return lens
    weight = [count[i] for i in order]
    parent = {}
    leaf, inner = 0, used
    for nxt in range(used, 2 * used - 1):
        total = 0
        for _ in range(2):
            if leaf < used and (inner >= nxt or weight[leaf] <= weight[inner]):
                pick, leaf = leaf, leaf + 1
            else:
                pick, inner = inner, inner + 1
            total += weight[pick]
            parent[pick] = nxt
        weight.append(total)
    depth = {2 * used - 2: 0}
    overflow = 0
    for node in range(2 * used - 3, -1, -1):            # every node below the limit, inner ones too, is held at it and counted
        depth[node] = depth[parent[node]] + 1
        if depth[node] > maxbits:
            depth[node], overflow = maxbits, overflow + 1
    per = [0] * (maxbits + 1)
    for i in range(used):
        per[depth[i]] += 1
    while overflow > 0:
        bits = maxbits - 1
        while per[bits] == 0:
            bits -= 1
        per[bits] -= 1
        per[bits + 1] += 2
        per[maxbits] -= 1
        overflow -= 2
    at = 0
    for bits in range(maxbits, 0, -1):
        for _ in range(per[bits]):
            lens[order[at]] = bits
            at += 1
    return lens


def unlimited_depth(count):
    """The longest code of the unlimited Huffman code (what the tests use to show that a histogram needs the limiting)."""
    return max(code_lengths(count, 64))


def canonical_codes(lens):
    """RFC 1951 3.2.2, each code bit-reversed (the stream is packed from bit 0 up)."""
    per = [0] * 17
    for v in lens:
        per[v] += 1
    per[0] = 0
    nxt, c = [0] * 17, 0
    for b in range(1, 17):
        c = (c + per[b - 1]) << 1
        nxt[b] = c
    out = []
    for v in lens:
        if v == 0:
            out.append(0)
            continue
        out.append(int(format(nxt[v], f"0{v}b")[::-1], 2))
        nxt[v] += 1
    return out


# ---- block --------------------------------------------------------------------------------------------------------------------------
def rle_lengths(seq):
    """[(symbol 0..18, extra value)]: zeros as 18 (138 at a time) while 11 or more remain, then 17 for 3..10, then single zeros; another
    length once, then 16 (6 at a time) while 3 or more remain, then single lengths."""
    out, i, n = [], 0, len(seq)
    while i < n:
        v, run = seq[i], 1
        while i + run < n and seq[i + run] == v:
            run += 1
        i += run
        if v == 0:
            while run >= 11:
                t = min(run, 138)
                out.append((18, t - 11))
                run -= t
            if run >= 3:
                out.append((17, run - 3))
                run = 0
            out += [(0, 0)] * run
        else:
            out.append((v, 0))
            run -= 1
            while run >= 3:
                t = min(run, 6)
                out.append((16, t - 3))
                run -= t
            out += [(v, 0)] * run
    return out


CL_EXTRA = {16: 2, 17: 3, 18: 7}


class Bits:
    def __init__(self):
        self.values, self.widths = [], []

    def put(self, v, n):
        if n:
            self.values.append(int(v))
            self.widths.append(int(n))

    def extend(self, values, widths):
        self.values += [int(v) for v in values]
        self.widths += [int(n) for n in widths]

    def count(self):
        return int(sum(self.widths))

    def pad(self):
        self.put(0, -self.count() % 8)

    def tobytes(self):
        v, w = np.array(self.values, np.int64), np.array(self.widths, np.int64)
        total = int(w.sum())
        first = np.cumsum(w) - w
        k = np.arange(total) - np.repeat(first, w)
        bits = ((np.repeat(v, w) >> k) & 1).astype(np.uint8)
        return np.packbits(bits, bitorder="little").tobytes()


def header(lens):
    """(hlit, hclen, rle, cl_lens, cl_codes, bits) of a block whose literal / length code is `lens`; the distance code is one code of
    length 1, match or no match."""
    hlit = LITLEN
    while hlit > 257 and lens[hlit - 1] == 0:
        hlit -= 1
    rle = rle_lengths(list(lens[:hlit]) + [1])
    count = [0] * 19
    for s, _ in rle:
        count[s] += 1
    cl = code_lengths(count, 7)
    hclen = 19
    while hclen > 4 and cl[CL_ORDER[hclen - 1]] == 0:
        hclen -= 1
    bits = 14 + 3 * hclen + sum(count[s] * (cl[s] + CL_EXTRA.get(s, 0)) for s in range(19))
    return hlit, hclen, rle, cl, canonical_codes(cl), bits


def deflate_chunk(chunk, prev, final, info=None):
    """One chunk as one block and its sync block, or as a stored block when that is shorter: bytes."""
    chunk = np.asarray(chunk, np.uint8)
    n = chunk.size
    sym, mlen = tokens(chunk, prev)
    count = np.bincount(sym, minlength=LITLEN)
    count[256] = 1
    lens = code_lengths(count, 15)
    codes = canonical_codes(lens)
    hlit, hclen, rle, cl, clc, hbits = header(lens)
    extra = [0 if s < 265 or s == 285 else (s - 261) >> 2 for s in range(LITLEN)]
    bits = 3 + hbits + sum(int(count[s]) * (lens[s] + (extra[s] + 1 if s > 256 else 0)) for s in range(LITLEN))
    size = (bits + 7) // 8 if final else (bits + 3 + 7) // 8 + 4
    if info is not None:
        info.update(lens=lens, cl=cl, stored=size > n + 5, hlit=hlit, hclen=hclen, rle=rle, matches=int((mlen > 0).sum()))
    if size > n + 5:
        return bytes([1 if final else 0]) + struct.pack("<HH", n, n ^ 0xFFFF) + chunk.tobytes()
    w = Bits()
    w.put(1 if final else 0, 1)
    w.put(2, 2)
    w.put(hlit - 257, 5)
    w.put(0, 5)
    w.put(hclen - 4, 4)
    for i in range(hclen):
        w.put(cl[CL_ORDER[i]], 3)
    for s, e in rle:
        w.put(clc[s], cl[s])
        w.put(e, CL_EXTRA.get(s, 0))
    L, Cd = np.array(lens), np.array(codes)
    value = Cd[sym] | (_LEN_EV[mlen] << L[sym])                             # code, extra bits, and for a match the distance code's 0
    width = L[sym] + np.where(mlen > 0, _LEN_EB[mlen] + 1, 0)
    w.extend(value, width)
    w.put(codes[256], lens[256])
    assert w.count() == bits
    if not final:
        w.put(0, 3)
        w.pad()
        w.put(0xFFFF0000, 32)
    else:
        w.pad()
    out = w.tobytes()
    assert len(out) == size
    return out


def deflate_pieces(row, chunk=CHUNK, info=None):
    """The chunks of one byte row as independent byte strings."""
    row = np.asarray(row, np.uint8).reshape(-1)
    n = row.size
    assert n >= 1
    out = []
    for at in range(0, n, chunk):
        i = {} if info is not None else None
        out.append(deflate_chunk(row[at:at + chunk], int(row[at - 1]) if at else None, at + chunk >= n, i))
        if info is not None:
            info.append(i)
    return out


def adler32(row):
    """Adler-32 joined from the chunks' partial sums, as the GPU does it."""
    row = np.asarray(row, np.uint8).reshape(-1).astype(np.int64)
    A, B = 1, 0
    for at in range(0, row.size, CHUNK):
        d = row[at:at + CHUNK]
        m = d.size
        a, b = int(d.sum()) % 65521, int(((m - np.arange(m)) * d).sum()) % 65521
        B = (B + (m % 65521) * A + b) % 65521
        A = (A + a) % 65521
    return (B << 16) | A


def zlib_compress(row, info=None):
    """ops.zlib_compress of one row: 78 01, the chunks, Adler-32."""
    return b"\x78\x01" + b"".join(deflate_pieces(row, info=info)) + struct.pack(">I", adler32(row))


def zlib_capacity(n):
    """ll_zlib_sizes' out_stride: header, every chunk stored (5 bytes each), Adler-32, rounded up to 16."""
    return -(-(2 + n + 5 * -(-n // CHUNK) + 4) // 16) * 16


# ---- container ------------------------------------------------------------------------------------------------------------------------
def png_chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data))


def png_file(frame, info=None):
    """One uint8 [H, W, 3] frame as the file ll_png_encode_u8 writes: IHDR, one IDAT per deflate chunk (the first carries 78 01), one
    IDAT of the Adler-32, IEND."""
    frame = np.asarray(frame)
    H, W, _ = frame.shape
    stream = filter_frames(frame[None])[0].reshape(-1)
    pieces = deflate_pieces(stream, info=info)
    pieces[0] = b"\x78\x01" + pieces[0]
    out = SIGNATURE + png_chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0))
    out += b"".join(png_chunk(b"IDAT", p) for p in pieces)
    out += png_chunk(b"IDAT", struct.pack(">I", adler32(stream))) + png_chunk(b"IEND", b"")
    return out


def png_capacity(H, W):
    """ll_png_sizes' out_stride: signature and IHDR (33), per chunk 12 bytes of IDAT framing and 5 of a stored block around its bytes,
    78 01, the Adler-32's IDAT (16), IEND (12), rounded up to 16."""
    n = H * (1 + 3 * W)
    return -(-(33 + n + 17 * -(-n // CHUNK) + 2 + 16 + 12) // 16) * 16


def read_chunks(data):
    """[(kind, payload, crc_ok)] of a PNG file."""
    assert data[:8] == SIGNATURE
    at, out = 8, []
    while at < len(data):
        n, = struct.unpack(">I", data[at:at + 4])
        kind, payload = data[at + 4:at + 8], data[at + 8:at + 8 + n]
        crc, = struct.unpack(">I", data[at + 8 + n:at + 12 + n])
        out.append((kind, payload, crc == zlib.crc32(kind + payload)))
        at += 12 + n
    assert at == len(data)
    return out
