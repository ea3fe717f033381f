"""Inputs that reach the edges of the PNG encoder (csrc/png.h, csrc/png.hip), shared by test_png_host.py (the restatement against
zlib and PIL, csrc/png.h as a host program) and test_png_gpu.py (the GPU against the restatement).  Everything is built from counters
and one seeded generator, so both files see the same bytes."""
import numpy as np

import png_ref as R

C = R.CHUNK


def background(n, phase=0):
    """n bytes in which no byte equals the one before it (and byte 0 is never `phase`'s neighbour by accident): no repeat anywhere."""
    return ((np.arange(n) + phase) % 251).astype(np.uint8)


def arranged(counts):
    """A row with symbol s exactly counts[s] times and no two equal neighbours (the largest count is at most half, rounded up): the
    symbols, most frequent first, laid on the even positions and then on the odd ones."""
    items = sorted(counts.items(), key=lambda kv: (-kv[1], kv[0]))
    n = sum(counts.values())
    assert items[0][1] <= (n + 1) // 2
    row = np.zeros(n, np.uint8)
    row[list(range(0, n, 2)) + list(range(1, n, 2))] = np.concatenate([np.full(c, s, np.uint8) for s, c in items])
    assert (row[1:] != row[:-1]).all()
    return row


def fibonacci_row():
    """18 literals with counts 1, 2, 3, 5, .. 4181 (10944 bytes, one chunk); with the end-of-block code's 1 in front the histogram is
    the Fibonacci sequence, whose unlimited Huffman code is 18 bits deep."""
    fib = [1, 2]
    while len(fib) < 18:
        fib.append(fib[-1] + fib[-2])
    return arranged({10 + 3 * i: c for i, c in enumerate(fib)})                 # 4181 of 10944: under half, so `arranged` can place it


# Codes per length of a literal code (found by search) whose run-length coded header uses eleven code-length symbols with counts
# 1, 1, 1, 2, 3, 4, 5, 9, 14, 33, 59, 126: the unlimited code of the 19-symbol alphabet is 8 bits deep.  With counts 2^(14 - length)
# the literal code has exactly these lengths (the distribution is dyadic), the end-of-block code being one of the 14-bit ones.
DEEP_CL_PER_LENGTH = {2: 1, 3: 3, 4: 2, 5: 5, 6: 4, 8: 1, 10: 9, 11: 14, 13: 33, 14: 125}


def deep_code_length_row():
    """C - 1 bytes, one chunk, no repeat: drives the code-length code past 7 bits."""
    lens = [ln for ln, c in sorted(DEEP_CL_PER_LENGTH.items()) for _ in range(c)]
    counts = {(k * 97) % 256: 1 << (14 - ln) for k, ln in enumerate(lens)}
    assert len(counts) == len(lens) and sum(counts.values()) == C - 1
    return arranged(counts)


def span_row(L, n=1500, at=100):
    """A background row with one span of exactly L repeats: L + 1 equal bytes from `at`."""
    row = background(n)
    row[at:at + L + 1] = 253
    return row


def compressor_rows():
    """{name: uint8 row}: the compressor's edge list."""
    g = np.random.default_rng(7)
    rows = {}
    for n in (1, 2, 3, C - 1, C, C + 1, 2 * C, 2 * C + 1):
        rows[f"few_values_{n}"] = g.integers(0, 4, n, dtype=np.uint8)          # matches and literals, dynamic blocks
    for L in (2, 3, 257, 258, 259, 260, 261, 516, 517):
        rows[f"span_{L}"] = span_row(L)
    row = background(3 * C)
    row[C - 10:C] = 252                 # a span that ends exactly at a chunk's end (byte C differs)
    row[2 * C - 1:2 * C + 20] = 253     # a span that starts at a chunk's start: its first repeat looks back into the previous block
    rows["span_at_chunk_ends"] = row
    row = background(2 * C)
    row[C - 300:C + 300] = 254          # a span across a chunk boundary: cut there, both parts longer than 258
    rows["span_across_chunks"] = row
    rows["all_equal_1000"] = np.full(1000, 9, np.uint8)               # one literal, three matches of 258 and one of 225, end of block
    rows["all_equal_C_plus_5"] = np.full(C + 5, 9, np.uint8)
    rows["noise"] = g.integers(0, 256, C + 77, dtype=np.uint8)          # no gain: the stored fallback, twice
    rows["one_literal_no_match_2"] = np.full(2, 65, np.uint8)           # "AA": one repeat, too short for a match
    rows["one_literal_no_match_3"] = np.full(3, 65, np.uint8)
    rows["one_literal_last_chunk"] = np.concatenate([background(C), np.full(2, 255, np.uint8)])
    rows["two_literals_no_match"] = np.tile(np.array([1, 2], np.uint8), 300)      # two codes of length 1, and no match: the distance code
    rows["fibonacci"] = fibonacci_row()
    rows["deep_code_lengths"] = deep_code_length_row()
    return rows


def winner_frame(kind):
    """A 3 x 8 frame whose last row is won by filter `kind` by exactly 1 over the runner-up (checked by the caller), the rows above
    being what makes Up / Average / Paeth cheap or dear."""
    f = np.zeros((3, 8, 3), np.uint8)
    g = np.random.default_rng(100 + kind)
    f[:2] = g.integers(0, 256, (2, 8, 3))
    up = f[1].astype(int).reshape(-1)
    if kind == 0:
        row = np.array([1, 255, 2, 254, 1, 255] * 4)                 # small magnitudes, alternating sign: every predictor hurts
    elif kind == 1:
        row = (np.arange(24) // 3 * 40 + np.array([7, 90, 200] * 8)) % 256      # each pixel = the one to its left + 40
    elif kind == 2:
        row = (up + 1) % 256
    elif kind == 3:
        left = np.zeros(24, int)
        row = np.zeros(24, int)
        for i in range(24):
            left[i] = row[i - 3] if i >= 3 else 0
            row[i] = ((left[i] + up[i]) >> 1) % 256
    else:
        row = np.zeros(24, int)
        prev = f[1].astype(int).reshape(-1)
        for i in range(24):
            a = row[i - 3] if i >= 3 else 0
            b, c = prev[i], (prev[i - 3] if i >= 3 else 0)
            p = a + b - c
            pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
            row[i] = a if pa <= pb and pa <= pc else b if pb <= pc else c
    f[2] = np.asarray(row, np.uint8).reshape(8, 3)
    return f


def costs(frame):
    """[H, 5]: the filter heuristic's cost of every type for every row."""
    x = frame.reshape(frame.shape[0], -1).astype(np.int64)
    a = np.zeros_like(x)
    a[:, 3:] = x[:, :-3]
    b = np.zeros_like(x)
    b[1:] = x[:-1]
    c = np.zeros_like(x)
    c[1:, 3:] = x[:-1, :-3]
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    pae = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    forms = np.stack([x, x - a, x - b, x - ((a + b) >> 1), x - pae], -1) & 255
    return np.minimum(forms, 256 - forms).sum(1)


def by_one(kind):
    """winner_frame(kind) with bytes of its last row changed, one at a time and never when that takes the margin further from 1, until `kind`
    wins that row by exactly 1 (a seeded walk: the same frame every time)."""
    f = winner_frame(kind)
    g = np.random.default_rng(200 + kind)

    def margin(frame):
        cst = costs(frame)[2]
        return int(np.delete(cst, kind).min() - cst[kind])

    m = margin(f)
    for _ in range(20000):
        if m == 1:
            return f
        trial = f.copy()
        trial[2].reshape(-1)[g.integers(24)] = g.integers(256)
        t = margin(trial)
        if abs(t - 1) <= abs(m - 1):
            f, m = trial, t
    raise AssertionError(f"no frame in which filter {kind} wins by 1")


def tie_frame():
    """Row 0 of a one-row frame: Up, Average and Paeth see a zero row above, so None = Up and Sub = Paeth cost the same; a constant
    row makes Sub (1) and Paeth (4) tie for the win and the lower type must be taken."""
    return np.full((1, 8, 3), 100, np.uint8)


def filter_frames():
    """{name: uint8 [T, H, W, 3]}: the filter's edge list."""
    g = np.random.default_rng(11)
    out = {}
    for W in (1, 2, 21, 22, 64, 85, 86):
        for H in (1, 2, 3, 17):
            yy, xx = np.mgrid[0:H, 0:W]
            f = np.stack([(5 * xx + 3 * yy) % 256, (7 * yy + xx // 2) % 256, (xx * yy) % 256], -1) + g.integers(0, 3, (H, W, 3))
            out[f"shape_{H}x{W}"] = (f % 256).astype(np.uint8)[None]
    for k in range(5):
        out[f"wins_by_one_{k}"] = by_one(k)[None]
    out["tie"] = tie_frame()[None]
    return out


def whole_frames():
    """{name: uint8 [H, W, 3]}: constant, noise and gradient at 16x16, 17x33 and 64x96."""
    g = np.random.default_rng(13)
    out = {}
    for H, W in ((16, 16), (17, 33), (64, 96)):
        yy, xx = np.mgrid[0:H, 0:W]
        out[f"constant_{H}x{W}"] = np.full((H, W, 3), 77, np.uint8)
        out[f"noise_{H}x{W}"] = g.integers(0, 256, (H, W, 3), dtype=np.uint8)
        out[f"gradient_{H}x{W}"] = np.stack([2 * xx + yy, 255 - 3 * yy, xx + 2 * yy], -1).astype(np.uint8)
    return out


def synthetic_frame(seed, H=480, W=832):
    """A frame of the kinds of content generated video has: smooth gradients, flat regions, hard edges, mild noise."""
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    base = np.stack([128 + 100 * np.sin(xx / 97 + seed) * np.cos(yy / 61), 0.25 * xx + 0.1 * yy, 255 - 0.4 * yy + 0.05 * xx], -1)
    base[H // 8:H // 3, W // 10:W // 2] = (40, 90, 200)                          # a flat region
    base[H // 2:H // 2 + 60, W // 3:W - 50] = (250, 250, 245)                    # another, with hard edges
    base[(yy > 0.6 * H) & ((xx // 16 + yy // 16) % 2 == 0) & (xx > 0.6 * W)] += 60       # a checkerboard: edges every 16 pixels
    noise = g.normal(0, 1.5, base.shape) * (xx[..., None] > W / 2)               # mild noise on the right half
    return np.clip(np.rint(base + noise), 0, 255).astype(np.uint8)
