"""Restatement of csrc/jpeg_dec.hip and longlive_amd/jpeg_files.py in plain Python / numpy fp64: a marker walk, a bit-serial entropy
decoder over bit strings, the pixel arithmetic (dequantise, C^T F C, + 128, clamp, triangle chroma upsampling at the component's own
extent, YCbCr -> RGB) returning UNROUNDED values, and the antialiased resize formula.  Tables and test contents come from
tests/jpeg_ref.py; nothing is shared with the library."""
import numpy as np

import jpeg_ref as J


def parse(data: bytes) -> dict:
    """The header of one baseline file and its scan as a list of de-stuffed segments (split at RSTn)."""
    assert data[:2] == b"\xff\xd8"
    p, qt, huff, ri, sof = 2, {}, {}, 0, None
    while True:
        assert data[p] == 0xFF
        while data[p] == 0xFF:
            p += 1
        m, p = data[p], p + 1
        L = int.from_bytes(data[p:p + 2], "big")
        body = data[p + 2:p + L]
        if m == 0xDB:
            for q in range(0, len(body), 65):
                assert body[q] >> 4 == 0
                qt[body[q] & 15] = list(body[q + 1:q + 65])                      # zigzag order
        elif m == 0xC4:
            q = 0
            while q < len(body):
                bits = list(body[q + 1:q + 17])
                huff[(body[q] >> 4, body[q] & 15)] = (bits, list(body[q + 17:q + 17 + sum(bits)]))
                q += 17 + sum(bits)
        elif m == 0xC0:
            assert body[0] == 8
            sof = dict(H=int.from_bytes(body[1:3], "big"), W=int.from_bytes(body[3:5], "big"),
                       comps=[(body[6 + 3 * i], body[7 + 3 * i] >> 4, body[7 + 3 * i] & 15, body[8 + 3 * i]) for i in range(body[5])])
        elif m == 0xDD:
            ri = int.from_bytes(body, "big")
        elif m == 0xDA:
            ids = {body[1 + 2 * i]: (body[2 + 2 * i] >> 4, body[2 + 2 * i] & 15) for i in range(body[0])}
            p += L
            break
        else:
            assert m not in (0xC1, 0xC2, 0xC9, 0xCA), "not baseline"
        p += L
    segs, cur = [], bytearray()
    while True:
        b = data[p]
        if b != 0xFF:
            cur.append(b)
            p += 1
        elif data[p + 1] == 0:
            cur.append(0xFF)
            p += 2
        elif data[p + 1] == 0xFF:
            p += 1
        elif 0xD0 <= data[p + 1] <= 0xD7:
            segs.append(bytes(cur))
            cur = bytearray()
            p += 2
        else:
            assert data[p + 1] == 0xD9
            segs.append(bytes(cur))
            break
    comps = sof["comps"]
    nc = len(comps)
    hs, vs = (1, 1) if nc == 1 else (comps[0][1], comps[0][2])
    return dict(H=sof["H"], W=sof["W"], nc=nc, hs=hs, vs=vs, ri=ri, segs=segs,
                qt=[qt[c[3]] for c in comps], dc=[huff[(0, ids[c[0]][0])] for c in comps], ac=[huff[(1, ids[c[0]][1])] for c in comps])


def grid(info):
    H, W, hs, vs = info["H"], info["W"], info["hs"], info["vs"]
    return -(-H // (8 * vs)), -(-W // (8 * hs)), (1 if info["nc"] == 1 else hs * vs + 2)


def _decoder(bits, vals):
    inv = {code: sym for sym, code in J.huffman_codes(bits, vals).items()}

    def read(s, pos):
        for n in range(1, 17):
            sym = inv.get(s[pos:pos + n])
            if sym is not None and len(s) >= pos + n:
                return sym, pos + n
        raise ValueError("no code")
    return read


def _extend(v, s):
    return v if v >= 1 << (s - 1) else v - (1 << s) + 1


def coefficients(data: bytes):
    """(info, int16 [rows, cols, bpm, 64] in zigzag order, blocks in scan order)."""
    info = parse(data)
    rows, cols, bpm = grid(info)
    ny = 1 if bpm == 1 else bpm - 2
    dc = [_decoder(*t) for t in info["dc"]]
    ac = [_decoder(*t) for t in info["ac"]]
    out = np.zeros((rows * cols, bpm, 64), dtype=np.int16)
    per = info["ri"] or rows * cols
    assert len(info["segs"]) == -(-rows * cols // per)
    for i, seg in enumerate(info["segs"]):
        s = "".join(format(b, "08b") for b in seg)
        pos, pred = 0, [0, 0, 0]
        for mcu in range(i * per, min((i + 1) * per, rows * cols)):
            for b in range(bpm):
                c = 0 if b < ny else b - ny + 1
                cat, pos = dc[c](s, pos)
                if cat:
                    pred[c] += _extend(int(s[pos:pos + cat], 2), cat)
                    pos += cat
                out[mcu, b, 0] = pred[c]
                k = 1
                while k < 64:
                    rs, pos = ac[c](s, pos)
                    r, size = rs >> 4, rs & 15
                    if size == 0:
                        if r != 15:
                            break
                        k += 16
                        continue
                    k += r
                    out[mcu, b, k] = _extend(int(s[pos:pos + size], 2), size)
                    pos += size
                    k += 1
        assert len(s) - pos < 8 + 8 and set(s[pos:]) <= {"1"}, "segment not consumed"
    return info, out.reshape(rows, cols, bpm, 64)


def _dct_matrix():
    n = np.arange(8)
    c = np.cos((2 * n[None, :] + 1) * n[:, None] * np.pi / 16) * 0.5
    c[0] = np.sqrt(1.0 / 8.0)
    return c


def planes(info, coef):
    """fp64 component planes (MCU padded), each sample clamped to [0, 255], unrounded."""
    rows, cols, bpm = grid(info)
    hs, vs, C = info["hs"], info["vs"], _dct_matrix()
    ny = 1 if bpm == 1 else bpm - 2
    out = [np.zeros((rows * 8 * (vs if c == 0 else 1), cols * 8 * (hs if c == 0 else 1))) for c in range(info["nc"])]
    inv = np.argsort(J.ZIGZAG)
    for r in range(rows):
        for m in range(cols):
            for b in range(bpm):
                c = 0 if b < ny else b - ny + 1
                F = (coef[r, m, b].astype(np.float64) * np.array(info["qt"][c], dtype=np.float64))[inv].reshape(8, 8)
                px = np.clip(C.T @ F @ C + 128.0, 0.0, 255.0)
                y0, x0 = ((r * vs + b // hs) * 8, (m * hs + b % hs) * 8) if c == 0 else (r * 8, m * 8)
                out[c][y0:y0 + 8, x0:x0 + 8] = px
    return out


def _upsample(pl, n_out, axis):
    """Triangle filter 0.75 near + 0.25 far along `axis`, to n_out samples; pl is cut to the component's own extent first."""
    pl = np.moveaxis(pl, axis, 0)
    o = np.arange(n_out)
    near = o >> 1
    far = np.clip(near + np.where(o & 1, 1, -1), 0, pl.shape[0] - 1)
    return np.moveaxis(0.75 * pl[near] + 0.25 * pl[far], 0, axis)


def pixels_unrounded(data: bytes, coef=None) -> np.ndarray:
    """fp64 [H, W, 3] R, G, B before `clamp(floor(v + 0.5), 0, 255)`."""
    if coef is None:
        info, coef = coefficients(data)
    else:
        info = parse(data)
    H, W, hs, vs = info["H"], info["W"], info["hs"], info["vs"]
    pl = planes(info, coef)
    Y = pl[0][:H, :W]
    if info["nc"] == 1:
        return np.repeat(Y[..., None], 3, -1)
    ch = []
    for c in (1, 2):
        v = pl[c][:-(-H // vs), :-(-W // hs)]                                  # the component's own extent
        if vs == 2:
            v = _upsample(v, H, 0)
        if hs == 2:
            v = _upsample(v, W, 1)
        ch.append(v - 128.0)
    cb, cr = ch
    return np.stack([Y + 1.402 * cr, Y - 0.344136286 * cb - 0.714136286 * cr, Y + 1.772 * cb], -1)


def to_bytes(v: np.ndarray) -> np.ndarray:
    return np.clip(np.floor(v + 0.5), 0, 255).astype(np.uint8)


def decode(data: bytes) -> np.ndarray:
    return to_bytes(pixels_unrounded(data))


# ---- files from another encoder -----------------------------------------------------------------------------------------------------------
PIL_SIZES = ((1, 1), (17, 33), (23, 37), (37, 53), (48, 64))
PIL_SAMPLINGS = (0, 1, 2, "grey")                    # PIL's `subsampling`: 4:4:4, 4:2:2, 4:2:0
PIL_VARIANTS = {"q30": dict(quality=30), "q95_optimize": dict(quality=95, optimize=True),
                "q95_restart3": dict(quality=95, restart_marker_blocks=3)}


def pil_file(Image, frame, sampling, **kw) -> bytes:
    import io
    b = io.BytesIO()
    if sampling == "grey":
        Image.fromarray(frame[..., 1]).save(b, "JPEG", **kw)
    else:
        Image.fromarray(frame).save(b, "JPEG", subsampling=sampling, **kw)
    return b.getvalue()


def pil_cases(Image) -> dict:
    """name -> one Pillow-made file: every size x sampling x (quality 30; 95 with optimised tables; 95 with restart markers)."""
    return {f"{H}x{W}_{s}_{v}": pil_file(Image, J.smooth_noise(H, W, H + W), s, **kw)
            for H, W in PIL_SIZES for s in PIL_SAMPLINGS for v, kw in PIL_VARIANTS.items()}


def pil_decode(Image, data: bytes) -> np.ndarray:
    import io
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


# ---- resize -----------------------------------------------------------------------------------------------------------------------------
def taps(n_in: int, n_out: int):
    """[(first index, fp64 weights)] per output sample: antialiased triangle filter."""
    scale = n_in / n_out
    s = max(scale, 1.0)
    out = []
    for o in range(n_out):
        c = (o + 0.5) * scale
        lo, hi = max(int(c - s + 0.5), 0), min(int(c + s + 0.5), n_in)
        w = np.array([max(0.0, 1.0 - abs((i + 0.5 - c) / s)) for i in range(lo, hi)], dtype=np.float64)
        out.append((lo, w / w.sum()))
    return out


def matrix(n_in: int, n_out: int, rounded: bool = True) -> np.ndarray:
    """[n_out, n_in] fp64; `rounded`: the weights rounded to fp32 as the kernel receives them."""
    M = np.zeros((n_out, n_in))
    for o, (lo, w) in enumerate(taps(n_in, n_out)):
        M[o, lo:lo + len(w)] = w.astype(np.float32).astype(np.float64) if rounded else w
    return M


def resize_unrounded(x: np.ndarray, Hd: int, Wd: int, rounded: bool = True) -> np.ndarray:
    """x [..., Hs, Ws, C] -> fp64 [..., Hd, Wd, C], vertical then horizontal."""
    x = x.astype(np.float64)
    v = np.einsum("oh,...hwc->...owc", matrix(x.shape[-3], Hd, rounded), x)
    return np.einsum("pw,...owc->...opc", matrix(x.shape[-2], Wd, rounded), v)


def cover_window(Hs, Ws, Hd, Wd):
    """(y0, x0, Hc, Wc): the centred window of the target's aspect."""
    if Ws * Hd >= Wd * Hs:
        Wc = min(Ws, max(1, int(np.floor(Hs * Wd / Hd + 0.5))))
        return 0, (Ws - Wc) // 2, Hs, Wc
    Hc = min(Hs, max(1, int(np.floor(Ws * Hd / Wd + 0.5))))
    return (Hs - Hc) // 2, 0, Hc, Ws


def band_check(got: np.ndarray, want: np.ndarray):
    """The pixel rule of the GPU tests: |got - rounded| <= 1 everywhere, equal wherever `want` is more than 2^-8 from a half-integer.
    Returns (max abs difference, mismatches outside the band, share of samples inside the band)."""
    ref = to_bytes(want).astype(np.int64)
    diff = np.abs(got.astype(np.int64) - ref)
    frac = want - np.floor(want)
    inside = (np.abs(frac - 0.5) <= 2.0 ** -8) & (want > -1) & (want < 256)
    return int(diff.max()), int(((diff != 0) & ~inside).sum()), float(inside.mean())
