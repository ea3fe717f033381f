"""Restatement of csrc/jpeg.hip in numpy, fp64: the tables of ITU T.81 Annex K, the 613-byte header, the coefficient stage (colour
conversion, 4:2:0 means, orthonormal 8 x 8 DCT-II, IJG-scaled quantisation, zigzag) and a bit-serial entropy coder with restart
intervals of one MCU row that can also report which symbols it emitted.  Nothing here is shared with the library: the tables are typed
in a second time, the DCT is the cosine matrix itself, the bit stream is built one bit string at a time."""
import numpy as np

Q_LUM = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
         18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100,
         103, 99]
Q_CHR = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32
ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49,
          56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]

DC_LUM_BITS = [0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]
DC_CHR_BITS = [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0]
DC_VALS = list(range(12))
AC_LUM_BITS = [0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d]
AC_LUM_VALS = [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91,
    0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a,
    0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53,
    0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79,
    0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5,
    0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9,
    0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2,
    0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa]
AC_CHR_BITS = [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77]
AC_CHR_VALS = [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14,
    0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17,
    0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a,
    0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78,
    0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
    0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7,
    0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2,
    0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa]

HEADER_BYTES = 613


def quant_tables(quality: int):
    """(luminance, chrominance) as int arrays of 64 in NATURAL order: Annex K scaled by the IJG rule."""
    assert 1 <= quality <= 100
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple(np.clip((np.array(b, dtype=np.int64) * s + 50) // 100, 1, 255) for b in (Q_LUM, Q_CHR))


def huffman_codes(bits, vals):
    """symbol -> bit string (canonical codes, Annex C)."""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = format(code, "b").zfill(length)
            code += 1
            k += 1
        code <<= 1
    assert k == len(vals)
    return out


def mcu_grid(H: int, W: int):
    return (H + 15) // 16, (W + 15) // 16


def header(W: int, H: int, quality: int) -> bytes:
    ql, qc = quant_tables(quality)
    _, cols = mcu_grid(H, W)
    b = bytearray(b"\xff\xd8\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    b += b"\xff\xdb\x00\x84\x00" + bytes(int(ql[z]) for z in ZIGZAG) + b"\x01" + bytes(int(qc[z]) for z in ZIGZAG)
    b += b"\xff\xc0\x00\x11\x08" + H.to_bytes(2, "big") + W.to_bytes(2, "big") + b"\x03\x01\x22\x00\x02\x11\x01\x03\x11\x01"
    b += b"\xff\xc4\x01\xa2"
    for tc_th, bits, vals in ((0x00, DC_LUM_BITS, DC_VALS), (0x10, AC_LUM_BITS, AC_LUM_VALS), (0x01, DC_CHR_BITS, DC_VALS),
                              (0x11, AC_CHR_BITS, AC_CHR_VALS)):
        b += bytes([tc_th]) + bytes(bits) + bytes(vals)
    b += b"\xff\xdd\x00\x04" + cols.to_bytes(2, "big")
    b += b"\xff\xda\x00\x0c\x03\x01\x00\x02\x11\x03\x11\x00\x3f\x00"
    assert len(b) == HEADER_BYTES
    return bytes(b)


def _dct_matrix():
    n = np.arange(8)
    c = np.cos((2 * n[None, :] + 1) * n[:, None] * np.pi / 16) * 0.5
    c[0] = np.sqrt(1.0 / 8.0)
    return c


def quotients(frame: np.ndarray, quality: int) -> np.ndarray:
    """frame uint8 [H, W, 3] -> fp64 [rows, cols, 6, 64]: dct / q of every block (Y00 Y01 Y10 Y11 Cb Cr) in zigzag order, unrounded."""
    H, W, _ = frame.shape
    rows, cols = mcu_grid(H, W)
    yy = np.minimum(np.arange(16 * rows), H - 1)
    xx = np.minimum(np.arange(16 * cols), W - 1)
    px = frame[yy][:, xx].astype(np.float64)                       # edge replication
    R, G, B = px[..., 0], px[..., 1], px[..., 2]
    Y = 0.299 * R + 0.587 * G + 0.114 * B - 128.0
    Cb = -0.168735892 * R - 0.331264108 * G + 0.5 * B
    Cr = 0.5 * R - 0.418687589 * G - 0.081312411 * B
    mean = lambda p: p.reshape(8 * rows, 2, 8 * cols, 2).mean(axis=(1, 3))      # noqa: E731
    Cb, Cr = mean(Cb), mean(Cr)
    C = _dct_matrix()
    ql, qc = quant_tables(quality)
    out = np.empty((rows, cols, 6, 64), dtype=np.float64)
    for r in range(rows):
        for m in range(cols):
            blocks = [Y[16 * r + 8 * by:16 * r + 8 * by + 8, 16 * m + 8 * bx:16 * m + 8 * bx + 8] for by in (0, 1) for bx in (0, 1)]
            blocks += [Cb[8 * r:8 * r + 8, 8 * m:8 * m + 8], Cr[8 * r:8 * r + 8, 8 * m:8 * m + 8]]
            for b, blk in enumerate(blocks):
                d = (C @ blk @ C.T).reshape(64) / (ql if b < 4 else qc)
                out[r, m, b] = d[ZIGZAG]
    return out


def coefficients(frame: np.ndarray, quality: int) -> np.ndarray:
    """int16 [rows, cols, 6, 64]: round-to-nearest of `quotients` (the clamp is never reached from 8-bit pixels)."""
    q = np.rint(quotients(frame, quality))
    q[..., 0] = np.clip(q[..., 0], -1024, 1023)
    q[..., 1:] = np.clip(q[..., 1:], -1023, 1023)
    return q.astype(np.int16)


def _category(v: int) -> int:
    return int(abs(v)).bit_length()


def _amplitude(v: int, cat: int) -> str:
    if cat == 0:
        return ""
    return format(v if v >= 0 else v + (1 << cat) - 1, "b").zfill(cat)


def encode_from_coefficients(coef: np.ndarray, W: int, H: int, quality: int, histogram=None) -> bytes:
    """coef int [rows, cols, 6, 64] -> one JFIF file.  histogram (a dict) collects counts under ("dc", category), ("ac", symbol) --
    ZRL is ("ac", 0xF0), EOB ("ac", 0x00) -- and "ff00" (stuffed bytes)."""
    rows, cols = mcu_grid(H, W)
    assert coef.shape == (rows, cols, 6, 64), coef.shape
    dc = (huffman_codes(DC_LUM_BITS, DC_VALS), huffman_codes(DC_CHR_BITS, DC_VALS))
    ac = (huffman_codes(AC_LUM_BITS, AC_LUM_VALS), huffman_codes(AC_CHR_BITS, AC_CHR_VALS))

    def count(key):
        if histogram is not None:
            histogram[key] = histogram.get(key, 0) + 1

    out = bytearray(header(W, H, quality))
    for r in range(rows):
        pred = [0, 0, 0]
        bits = []
        for m in range(cols):
            for b in range(6):
                comp, tb = (0, 0) if b < 4 else (b - 3, 1)
                z = [int(v) for v in coef[r, m, b]]
                d = z[0] - pred[comp]
                pred[comp] = z[0]
                cat = _category(d)
                count(("dc", cat))
                bits.append(dc[tb][cat] + _amplitude(d, cat))
                run = 0
                for v in z[1:]:
                    if v == 0:
                        run += 1
                        continue
                    while run > 15:
                        count(("ac", 0xF0))
                        bits.append(ac[tb][0xF0])
                        run -= 16
                    cat = _category(v)
                    count(("ac", (run << 4) | cat))
                    bits.append(ac[tb][(run << 4) | cat] + _amplitude(v, cat))
                    run = 0
                if run:
                    count(("ac", 0x00))
                    bits.append(ac[tb][0x00])
        s = "".join(bits)
        s += "1" * (-len(s) % 8)
        for i in range(0, len(s), 8):
            byte = int(s[i:i + 8], 2)
            out.append(byte)
            if byte == 0xFF:
                out.append(0)
                count("ff00")
        if r < rows - 1:
            out += bytes([0xFF, 0xD0 + (r & 7)])
    out += b"\xff\xd9"
    return bytes(out)


def encode(frame: np.ndarray, quality: int, histogram=None) -> bytes:
    H, W, _ = frame.shape
    return encode_from_coefficients(coefficients(frame, quality), W, H, quality, histogram)


def worst_case_bytes(H: int, W: int) -> int:
    """ll_jpeg_sizes' out_stride: header + 416 bytes per block + restart markers + EOI, rounded up to 16."""
    rows, cols = mcu_grid(H, W)
    n = HEADER_BYTES + rows * cols * 6 * 416 + 2 * (rows - 1) + 2
    return (n + 15) // 16 * 16


def psnr(a: np.ndarray, b: np.ndarray) -> float:
    mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return float("inf") if mse == 0 else float(10 * np.log10(255.0 ** 2 / mse))


# ---- the contents the tests share ----------------------------------------------------------------------------------------------------
def smooth_noise(H: int, W: int, seed: int = 0) -> np.ndarray:
    """A colour gradient plus mild noise: what decoded video looks like to the encoder."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    base = np.stack([128 + 100 * np.sin(x / 9.0 + seed), 128 + 100 * np.cos(y / 7.0), 60 + 2.0 * x + 1.5 * y], -1)
    return np.clip(base + rng.normal(0, 6, (H, W, 3)), 0, 255).astype(np.uint8)


def noise(H: int, W: int, seed: int = 0) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def pixel_checkerboard(H: int, W: int) -> np.ndarray:
    y, x = np.mgrid[0:H, 0:W]
    return np.repeat((((x + y) & 1) * 255).astype(np.uint8)[..., None], 3, -1)


def block_checkerboard(H: int, W: int) -> np.ndarray:
    y, x = np.mgrid[0:H, 0:W]
    return np.repeat(((((x >> 3) + (y >> 3)) & 1) * 255).astype(np.uint8)[..., None], 3, -1)


def flat(H: int, W: int, value=(90, 140, 200)) -> np.ndarray:
    return np.broadcast_to(np.array(value, dtype=np.uint8), (H, W, 3)).copy()


QUALITIES = (10, 50, 90, 100)


def cases():
    """name -> frames uint8 [T, H, W, 3]: every shape edge (one pixel, one block, one MCU, one past an MCU in both directions, odd
    sizes, several frames, ten restart intervals so RST7 is followed by RST0) with every kind of content."""
    return {
        "1x1": smooth_noise(1, 1)[None],
        "8x8_noise": noise(8, 8, 1)[None],
        "16x16_flat": flat(16, 16)[None],
        "17x33_smooth": smooth_noise(17, 33, 2)[None],
        "23x37_noise": noise(23, 37, 3)[None],
        "48x64_x3": np.stack([smooth_noise(48, 64, 4), noise(48, 64, 5), pixel_checkerboard(48, 64)]),
        "160x16_smooth": smooth_noise(160, 16, 6)[None],
        "32x32_pixel_checkerboard": pixel_checkerboard(32, 32)[None],
        "32x32_block_checkerboard": block_checkerboard(32, 32)[None],
    }
