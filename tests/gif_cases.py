"""Inputs that reach the edges of the GIF encoder (csrc/gif.h, csrc/gif.hip), shared by test_gif_host.py (the restatement against
Pillow, csrc/gif.h as a host program) and test_gif_gpu.py (the GPU against the restatement).  Everything is built from counters and
seeded generators, so both files see the same bytes."""
import functools

import numpy as np

import gif_ref as R
from png_cases import synthetic_frame  # noqa: F401  (the quality cases take it from here)

C = R.CHUNK


@functools.lru_cache(maxsize=None)
def rows_of_stream_length(k=1):
    """{name: row}: prefixes of one seeded row over four values whose LZW streams are 255 k - 1, 255 k and 255 k + 1 bytes long: the
    last sub-block of the file is one byte short of full, full, and followed by a block of one byte.  Found by search with the
    restatement (a stream never shrinks when the row grows, and grows by less than two bytes per index)."""
    g = np.random.default_rng(41)
    base = g.integers(0, 4, 4000, dtype=np.uint8)
    out, n = {}, 1
    for want in (255 * k - 1, 255 * k, 255 * k + 1):
        while len(R.lzw(base[:n])) < want:
            n += 1
        assert len(R.lzw(base[:n])) == want, (want, n)
        out[f"stream_{want}_bytes"] = base[:n].copy()
    return out


def lzw_rows():
    """{name: uint8 row}: the coder's edge list."""
    g = np.random.default_rng(43)
    rows = {}
    for n in (1, 2, C - 1, C, C + 1, 2 * C + 1):
        rows[f"random_{n}"] = g.integers(0, 256, n, dtype=np.uint8)          # hardly a pair repeats: a code per index, every width step
        rows[f"few_values_{n}"] = g.integers(0, 3, n, dtype=np.uint8)        # long matches
    for n in (1, 2, 1000, C, C + 1, 2 * C + 1):
        rows[f"all_equal_{n}"] = np.full(n, 201, np.uint8)                    # the run grows by one per code: the KwKwK case throughout
    rows["ramp_7169"] = (np.arange(2 * C + 1) % 256).astype(np.uint8)         # distinct neighbours that repeat every 256
    rows.update(rows_of_stream_length(1))
    return rows


def smooth(T, H, W, seed):
    """T frames of gradients with a flat patch and mild noise, drifting over time."""
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    out = []
    for t in range(T):
        f = np.stack([128 + 100 * np.sin((xx + 3 * t) / 17) * np.cos(yy / 11), 2.5 * xx + 1.5 * yy + 4 * t, 255 - 3 * yy + 0.5 * xx], -1)
        f[H // 4:H // 2, W // 5:W // 2] = (40, 90, 200)
        out.append(np.clip(np.rint(f + g.normal(0, 1.5, f.shape)), 0, 255))
    return np.stack(out).astype(np.uint8)


def distinct_bin_colours(n, seed):
    """n colours in n different histogram bins."""
    g = np.random.default_rng(seed)
    bins = g.choice(R.BINS, n, replace=False)
    c = (R.coords(bins) << 3) | g.integers(0, 8, (n, 3))
    return c.astype(np.uint8)


def quantiser_frames():
    """{name: uint8 [T, H, W, 3]}: the quantiser's edge list."""
    g = np.random.default_rng(47)
    out = {"one_pixel": np.array([[[[9, 200, 31]]]], np.uint8),
           "one_colour_5x7": np.full((1, 5, 7, 3), (12, 250, 99), np.uint8),
           "smooth_7x9": smooth(1, 7, 9, 1),
           "smooth_56x64": smooth(1, 56, 64, 2),                              # exactly one chunk
           "smooth_61x131": smooth(1, 61, 131, 3),                            # three chunks, the last partial
           "noise_40x50": g.integers(0, 256, (1, 40, 50, 3), dtype=np.uint8),   # 2000 occupied bins: all 255 splits
           "smooth_T3_33x47": smooth(3, 33, 47, 4)}
    colours = distinct_bin_colours(100, 5)
    out["hundred_colours_16x16"] = colours[g.integers(0, 100, (1, 16, 16))]
    corners = np.array([[0, 0, 0], [255, 255, 255], [0, 255, 255], [255, 0, 0]], np.uint8)
    out["cube_corners_4x4"] = corners[(np.arange(16) % 4).reshape(1, 4, 4)]   # equal extents, equal counts: the tie rules
    two = np.array([[0, 0, 0], [4, 4, 4]], np.uint8)                           # two cells of one bin: the few-colour route's tie
    out["nearest_tie_8x8"] = two[((np.arange(64) // 8 + np.arange(64)) % 2).reshape(1, 8, 8)]
    return out


def block_edge_frames():
    """{name: uint8 [1, 1, n, 3]}: four-colour frames of one row whose streams end one byte before, at, and one byte after a sub-block's
    end (every colour has its own bin, so the indices are the colours relabelled and the stream's length is the searched row's)."""
    colours = distinct_bin_colours(4, 9)
    return {name: colours[row][None, None] for name, row in rows_of_stream_length(1).items()}
