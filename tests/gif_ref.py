"""numpy restatement of csrc/gif.h ("Animated previews: GIF"): histogram, median cut, nearest-entry table, ordered
dither, LZW in independently coded chunks, the single-image GIF89a file.  Written from the format's description, not from the C text:
the matrix is built by its recursion, the dictionary is a Python dict, the bits are a string.  test_gif_host.py checks it against
Pillow's decoder; the GPU and csrc/gif.h as a host program are then compared with it byte for byte."""
import numpy as np

BINS, COLORS, CHUNK = 32768, 256, 3584
CLEAR, EOI, FIRST = 256, 257, 258
HEAD = 800
PALETTES = ("clip", "frame")
DITHERS = ("none", "bayer")


def bayer(n=8):
    """The n x n matrix of B(2n) = [[4B, 4B + 2], [4B + 3, 4B + 1]] from B(1) = [0]."""
    b = np.zeros((1, 1), np.int64)
    while b.shape[0] < n:
        b = np.block([[4 * b, 4 * b + 2], [4 * b + 3, 4 * b + 1]])
    return b


def dither_offsets(H, W, dither):
    """int64 [H, W]: what is added to every channel of a pixel before binning."""
    if dither == "none":
        return np.zeros((H, W), np.int64)
    assert dither == "bayer"
    d = (2 * bayer(8) - 63) >> 3
    return d[np.arange(H)[:, None] & 7, np.arange(W)[None, :] & 7]


def bins_of(px):
    """The bin of uint8 pixels [..., 3]."""
    p = px.astype(np.int64) >> 3
    return (p[..., 0] << 10) | (p[..., 1] << 5) | p[..., 2]


def histogram(frames):
    """(count, sums [BINS, 3]) over every pixel of uint8 [..., 3]."""
    px = frames.reshape(-1, 3)
    b = bins_of(px)
    count = np.bincount(b, minlength=BINS).astype(np.int64)
    sums = np.stack([np.bincount(b, weights=px[:, k].astype(np.float64), minlength=BINS) for k in range(3)], -1)
    return count, np.rint(sums).astype(np.int64)                  # float64 sums are exact under 2^53


def coords(bins):
    return np.stack([bins >> 10, (bins >> 5) & 31, bins & 31], -1)


def cut_items(xyz, cnt, sums, info=None):
    """The median cut over a list of occupied items -- coordinates int [n, 3], pixel counts [n], colour sums [n, 3] -> (palette uint8
    [256, 3], used).  `info` collects (box, axis, cut) per split."""
    box = np.zeros(cnt.size, np.int64)
    boxes = 1
    while boxes < COLORS:
        held = np.bincount(box, weights=cnt.astype(np.float64), minlength=boxes)
        items = np.bincount(box, minlength=boxes)
        ok = np.flatnonzero(items > 1)
        if ok.size == 0:
            break
        pick = int(ok[np.argmax(held[ok])])                         # argmax takes the first of equals: the lowest index
        m = box == pick
        ext = [int(xyz[m, a].max() - xyz[m, a].min()) for a in range(3)]
        axis = max((1, 0, 2), key=lambda a: ext[a])                 # max takes the first of equals: G, then R, then B
        marg = np.bincount(xyz[m, axis], weights=cnt[m].astype(np.float64), minlength=64).astype(np.int64)
        total = int(marg.sum())
        cum = np.cumsum(marg)
        cut = int(np.flatnonzero(2 * cum >= total)[0])
        present = np.flatnonzero(marg)
        if cut >= present[-1]:
            cut = int(present[-2])
        if info is not None:
            info.append((pick, axis, cut))
        box[m & (xyz[:, axis] > cut)] = boxes
        boxes += 1
    pal = np.zeros((COLORS, 3), np.uint8)
    for i in range(boxes):
        m = box == i
        n = int(cnt[m].sum())
        for k in range(3):
            pal[i, k] = (2 * int(sums[m, k].sum()) + n) // (2 * n)
    return pal, boxes


def median_cut(count, sums, info=None):
    """The median cut over the occupied bins of a histogram."""
    occ = np.flatnonzero(count)
    return cut_items(coords(occ), count[occ], sums[occ], info)


def few_colours(count):
    """Fewer than 256 occupied bins: the palette is made over the bins' 6-bit cells and looked up by 6-bit key."""
    return np.count_nonzero(count) < COLORS


def keys6_of(px):
    p = px.astype(np.int64) >> 2
    return (p[..., 0] << 12) | (p[..., 1] << 6) | p[..., 2]


def median_cut_cells(frames, info=None):
    """The median cut over the occupied (r >> 2, g >> 2, b >> 2) cells of uint8 pixels [..., 3]."""
    px = frames.reshape(-1, 3).astype(np.int64)
    keys, inv, cnt = np.unique(keys6_of(px), return_inverse=True, return_counts=True)
    sums = np.stack([np.rint(np.bincount(inv.reshape(-1), weights=px[:, k].astype(np.float64))).astype(np.int64) for k in range(3)], -1)
    xyz = np.stack([keys >> 12, (keys >> 6) & 63, keys & 63], -1)
    return cut_items(xyz, cnt.astype(np.int64), sums, info)


def nearest_of_keys6(pal, used, keys):
    """For each 6-bit key's cell centre ((c6 << 2) | 2) the used entry at the smallest squared distance, the lowest index on a tie."""
    centre = (np.stack([keys >> 12, (keys >> 6) & 63, keys & 63], -1) << 2) | 2
    d = ((centre[:, None, :].astype(np.int64) - pal[None, :used, :].astype(np.int64)) ** 2).sum(-1)
    return np.argmin(d, axis=1).astype(np.uint8)


def nearest_table(pal, used):
    """uint8 [BINS]: for each bin centre the used entry at the smallest squared distance, the lowest index on a tie."""
    centre = (coords(np.arange(BINS)) << 3) | 4
    d = ((centre[:, None, :].astype(np.int64) - pal[None, :used, :].astype(np.int64)) ** 2).sum(-1)
    return np.argmin(d, axis=1).astype(np.uint8)


def quantize(frames, palette="clip", dither="bayer"):
    """frames uint8 [T, H, W, 3] -> (indices uint8 [T, H, W], palettes uint8 [T or 1, 256, 3], used int32 [T or 1])."""
    assert palette in PALETTES and dither in DITHERS
    T, H, W, _ = frames.shape
    groups = [frames] if palette == "clip" else [frames[t:t + 1] for t in range(T)]
    pals, used, fine = [], [], []
    for g in groups:
        count, sums = histogram(g)
        fine.append(few_colours(count))
        p, u = median_cut_cells(g) if fine[-1] else median_cut(count, sums)
        pals.append(p), used.append(u)
    d = dither_offsets(H, W, dither)
    idx = np.empty((T, H, W), np.uint8)
    for t in range(T):
        k = t if palette == "frame" else 0
        px = np.clip(frames[t].astype(np.int64) + d[..., None], 0, 255)
        if fine[k]:
            keys, inv = np.unique(keys6_of(px), return_inverse=True)
            idx[t] = nearest_of_keys6(pals[k], used[k], keys)[inv.reshape(H, W)]
        else:
            idx[t] = nearest_table(pals[k], used[k])[bins_of(px)]
    return idx, np.stack(pals), np.asarray(used, np.int32)


def lzw_chunk_codes(idx, first, last):
    """[(code, width)] of one chunk of indices coded from a cleared dictionary."""
    out = [(CLEAR, 9)] if first else []
    table, width, nxt = {}, 9, FIRST
    prefix = int(idx[0])
    for b in idx[1:].tolist():
        key = (prefix, b)
        if key in table:
            prefix = table[key]
            continue
        out.append((prefix, width))
        table[key] = nxt
        if nxt == 1 << width:
            width += 1
        nxt += 1
        prefix = b
    out.append((prefix, width))
    if nxt == 1 << width:                                         # the entry the decoder adds for the last code
        width += 1
    out.append((EOI if last else CLEAR, width))
    assert width <= 12 and nxt <= FIRST + CHUNK - 1
    return out


def lzw(row, info=None):
    """The LZW byte stream of one row of indices (before sub-blocking).  `info` collects per chunk {"bits", "max_width", "codes"}."""
    row = np.asarray(row, np.uint8).reshape(-1)
    n = row.size
    chunks = -(-n // CHUNK)
    bits = []
    for c in range(chunks):
        codes = lzw_chunk_codes(row[c * CHUNK:(c + 1) * CHUNK], c == 0, c == chunks - 1)
        if info is not None:
            info.append({"bits": sum(w for _, w in codes), "max_width": max(w for _, w in codes), "codes": len(codes)})
        bits.extend(format(code, f"0{w}b")[::-1] for code, w in codes)          # least significant bit first
    s = "".join(bits)
    s += "0" * (-len(s) % 8)
    return bytes(int(s[i:i + 8][::-1], 2) for i in range(0, len(s), 8))


def lzw_capacity(n):
    return -(-((9 + 12 * n + 12 * -(-n // CHUNK) + 7) // 8) // 16) * 16


def file_capacity(H, W):
    b = (9 + 12 * H * W + 12 * -(-(H * W) // CHUNK) + 7) // 8
    return -(-(HEAD + b + -(-b // 255) + 2) // 16) * 16


def _up(v, a):
    return -(-v // a) * a


def lzw_scratch_bytes(T, n, base=0):
    """The coder's scratch: per chunk a slot of ceil((9 + 12 * 3584 + 12) / 32) words, a bit count (int32) and a bit offset (int64), per
    row a byte count (int64), each array rounded up to 256 bytes."""
    blocks = T * -(-n // CHUNK)
    words = -(-(9 + 12 * CHUNK + 12) // 32)
    return base + _up(4 * words * blocks, 256) + _up(4 * blocks, 256) + _up(8 * blocks, 256) + _up(8 * T, 256)


def scratch_bytes(T, H, W, palette):
    """The encoder's scratch.  Per palette: the histogram (4 x 32768 x 8) and the few-colour one (4 x 2048 x 8), their lists of occupied
    items (uint16 each), the table by bin and the one by 6-bit key; then flags (2 x int32), palettes (768) and used counts (int32) per
    palette, each array rounded up to 256; the indices; the coder's share."""
    P = T if palette == "frame" else 1
    per = 4 * BINS * 8 + 4 * 2048 * 8 + 2 * BINS + 2 * 2048 + BINS + 64 ** 3
    return lzw_scratch_bytes(T, H * W, P * per + _up(8 * P, 256) + _up(768 * P, 256) + _up(4 * P, 256) + _up(T * H * W, 256))


def sub_blocks(data):
    out = bytearray()
    for at in range(0, len(data), 255):
        piece = data[at:at + 255]
        out.append(len(piece))
        out += piece
    out.append(0)
    return bytes(out)


def gif_file(indices, pal):
    """The single-image GIF89a file of indices uint8 [H, W] under palette uint8 [256, 3]."""
    H, W = indices.shape
    size = W.to_bytes(2, "little") + H.to_bytes(2, "little")
    head = (b"GIF89a" + size + bytes([0x70, 0, 0]) + bytes([0x21, 0xF9, 4, 0x04, 0, 0, 0, 0]) +
            bytes([0x2C, 0, 0, 0, 0]) + size + bytes([0x87]) + pal.tobytes() + bytes([8]))
    assert len(head) == HEAD
    return head + sub_blocks(lzw(indices)) + b"\x3B"


def encode(frames, palette="clip", dither="bayer"):
    """[file bytes] of frames uint8 [T, H, W, 3]."""
    idx, pals, _ = quantize(frames, palette, dither)
    return [gif_file(idx[t], pals[t if palette == "frame" else 0]) for t in range(frames.shape[0])]


def images(data):
    """[{"delay", "local_table", "min_code", "stream", "blocks"}] of any GIF file: a walk over its blocks, a foreign writer's too."""
    assert data[:6] in (b"GIF89a", b"GIF87a")
    at = 13 + (3 * (2 << (data[10] & 7)) if data[10] & 0x80 else 0)
    out, delay = [], None

    def blocks(at):
        sizes, parts = [], []
        while data[at]:
            sizes.append(data[at])
            parts.append(data[at + 1:at + 1 + data[at]])
            at += 1 + data[at]
        return at + 1, sizes, b"".join(parts)

    while data[at] != 0x3B:
        if data[at] == 0x21:
            label = data[at + 1]
            at, _, payload = blocks(at + 2)
            if label == 0xF9:
                delay = int.from_bytes(payload[1:3], "little")
        else:
            assert data[at] == 0x2C
            flags = data[at + 9]
            at += 10
            table = None
            if flags & 0x80:
                table = data[at:at + 3 * (2 << (flags & 7))]
                at += len(table)
            min_code = data[at]
            at, sizes, stream = blocks(at + 1)
            out.append({"delay": delay, "local_table": table, "min_code": min_code, "stream": stream, "blocks": sizes})
    assert at == len(data) - 1
    return out


def psnr(a, b):
    mse = ((a.astype(np.float64) - b.astype(np.float64)) ** 2).mean()
    return float("inf") if mse == 0 else 10 * np.log10(255.0 ** 2 / mse)
