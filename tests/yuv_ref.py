"""Planar YUV in numpy int64: a restatement of the rules of DESIGN.md section 5c, "Planar YUV and Y4M", written from that text and not
from csrc/yuv.h.  BT.601 in 2^16 fixed point; rnd(x) = floor(x + 1/2) on the exact rational value (fractions); shifts are floors."""
from fractions import Fraction as Fr

import numpy as np

KR, KG, KB = Fr(299, 1000), Fr(587, 1000), Fr(114, 1000)
ONE = 1 << 16
LAYOUTS = ("420jpeg", "420mpeg2", "420paldv", "422", "444", "mono")
# (vertical, horizontal) siting of a layout's chroma
SITING = {"420jpeg": ("centre", "centre"), "420mpeg2": ("centre", "cosited"), "420paldv": ("cosited", "cosited"),
          "422": ("none", "cosited"), "444": ("none", "none")}


def rnd(x) -> int:
    x = Fr(x)
    return (2 * x.numerator + x.denominator) // (2 * x.denominator)


def scales(range_):
    """(sy, sc, yoff, (ylo, yhi), (clo, chi))"""
    if range_ == "full":
        return Fr(1), Fr(1), 0, (0, 255), (0, 255)
    assert range_ == "limited"
    return Fr(219, 255), Fr(224, 255), 16, (16, 235), (16, 240)


def forward_coefficients(range_):
    sy, sc = scales(range_)[:2]
    a_r, a_b = rnd(KR * sy * ONE), rnd(KB * sy * ONE)
    a = (a_r, rnd(sy * ONE) - a_r - a_b, a_b)
    b_r, b_g = -rnd(KR / (2 * (1 - KB)) * sc * ONE), -rnd(KG / (2 * (1 - KB)) * sc * ONE)
    b = (b_r, b_g, -(b_r + b_g))
    c_g, c_b = -rnd(KG / (2 * (1 - KR)) * sc * ONE), -rnd(KB / (2 * (1 - KR)) * sc * ONE)
    c = (-(c_g + c_b), c_g, c_b)
    return a, b, c


def inverse_coefficients(range_):
    """(cy, crv, cbu, cgu, cgv)"""
    sy, sc = scales(range_)[:2]
    return (rnd(ONE / sy), rnd(2 * (1 - KR) / sc * ONE), rnd(2 * (1 - KB) / sc * ONE), rnd(KB * 2 * (1 - KB) / KG / sc * ONE),
            rnd(KR * 2 * (1 - KR) / KG / sc * ONE))


def chroma_shape(layout, H, W):
    if layout == "mono":
        return 0, 0
    v, h = SITING[layout]
    return (H if v == "none" else (H + 1) // 2), (W if h == "none" else (W + 1) // 2)


def yuv420_bytes(H, W):
    return H * W + 2 * ((H + 1) // 2) * ((W + 1) // 2)


def luma(rgb, range_):
    """rgb [..., 3] -> Y [...] (int64)."""
    a = forward_coefficients(range_)[0]
    _, _, yoff, (lo, hi), _ = scales(range_)
    v = rgb.astype(np.int64)
    return np.clip(yoff + ((a[0] * v[..., 0] + a[1] * v[..., 1] + a[2] * v[..., 2] + (1 << 15)) >> 16), lo, hi)


def chroma_of_sums(S, range_):
    """S [..., 3]: channel sums over 2 x 2 pixels -> (Cb, Cr)."""
    _, b, c = forward_coefficients(range_)
    lo, hi = scales(range_)[4]
    S = S.astype(np.int64)
    cb = 128 + ((b[0] * S[..., 0] + b[1] * S[..., 1] + b[2] * S[..., 2] + (1 << 17)) >> 18)
    cr = 128 + ((c[0] * S[..., 0] + c[1] * S[..., 1] + c[2] * S[..., 2] + (1 << 17)) >> 18)
    return np.clip(cb, lo, hi), np.clip(cr, lo, hi)


def rgb_to_planes(frames, range_="limited"):
    """uint8 [T, H, W, 3] -> (y [T, H, W], cb [T, Hc, Wc], cr [T, Hc, Wc]) uint8; a missing last row or column is replicated."""
    T, H, W, _ = frames.shape
    v = frames.astype(np.int64)
    y = luma(v, range_)
    if H % 2:
        v = np.concatenate([v, v[:, -1:]], 1)
    if W % 2:
        v = np.concatenate([v, v[:, :, -1:]], 2)
    S = v[:, 0::2, 0::2] + v[:, 0::2, 1::2] + v[:, 1::2, 0::2] + v[:, 1::2, 1::2]
    cb, cr = chroma_of_sums(S, range_)
    return y.astype(np.uint8), cb.astype(np.uint8), cr.astype(np.uint8)


def rgb_to_i420(frames, range_="limited"):
    """uint8 [T, H, W, 3] -> uint8 [T, yuv420_bytes(H, W)]."""
    y, cb, cr = rgb_to_planes(frames, range_)
    T = frames.shape[0]
    return np.concatenate([y.reshape(T, -1), cb.reshape(T, -1), cr.reshape(T, -1)], 1)


def i420_planes(buf, H, W):
    hc, wc = (H + 1) // 2, (W + 1) // 2
    lead = buf.shape[:-1]
    return (buf[..., :H * W].reshape(*lead, H, W), buf[..., H * W:H * W + hc * wc].reshape(*lead, hc, wc),
            buf[..., H * W + hc * wc:].reshape(*lead, hc, wc))


def axis(mode, length, n):
    """Per luma position o < length: (near, far, weight of far in quarters) over n chroma samples; far clamped to the plane."""
    o = np.arange(length)
    if mode == "none":
        return o, o, np.zeros(length, np.int64)
    near = o >> 1
    if mode == "centre":
        far, wf = np.where(o & 1, near + 1, near - 1), np.ones(length, np.int64)
    else:
        assert mode == "cosited"
        far, wf = near + 1, np.where(o & 1, 2, 0).astype(np.int64)
    return near, np.clip(far, 0, n - 1), wf


def upsample16(plane, layout, H, W):
    """[T, Hc, Wc] -> [T, H, W] in units of 1/16."""
    p = plane.astype(np.int64)
    v, h = SITING[layout]
    ny, fy, wy = axis(v, H, p.shape[1])
    nx, fx, wx = axis(h, W, p.shape[2])
    wy, wx = wy[None, :, None], wx[None, None, :]
    g = lambda r, c: p[:, r][:, :, c]                                     # noqa: E731
    return (4 - wy) * (4 - wx) * g(ny, nx) + (4 - wy) * wx * g(ny, fx) + wy * (4 - wx) * g(fy, nx) + wy * wx * g(fy, fx)


def rgb_of_16(y, u16, v16, range_):
    cy, crv, cbu, cgu, cgv = inverse_coefficients(range_)
    yoff = scales(range_)[2]
    yy = 16 * cy * (y.astype(np.int64) - yoff)
    u, v = u16 - 2048, v16 - 2048
    r = np.clip((yy + crv * v + (1 << 19)) >> 20, 0, 255)
    g = np.clip((yy - cgu * u - cgv * v + (1 << 19)) >> 20, 0, 255)
    b = np.clip((yy + cbu * u + (1 << 19)) >> 20, 0, 255)
    return np.stack([r, g, b], -1).astype(np.uint8)


def planes_to_rgb(y, cb, cr, layout="420jpeg", range_="limited"):
    """y [T, H, W], cb / cr [T, Hc, Wc] (None for mono) -> uint8 [T, H, W, 3]."""
    T, H, W = y.shape
    if layout == "mono":
        u16 = v16 = np.full((T, H, W), 2048, np.int64)
    else:
        assert cb.shape[1:] == chroma_shape(layout, H, W) == cr.shape[1:]
        u16, v16 = upsample16(cb, layout, H, W), upsample16(cr, layout, H, W)
    return rgb_of_16(y, u16, v16, range_)


def psnr(a, b):
    d = a.astype(np.float64) - b.astype(np.float64)
    mse = float((d * d).mean())
    return float("inf") if mse == 0 else 10.0 * np.log10(255.0 * 255.0 / mse)
