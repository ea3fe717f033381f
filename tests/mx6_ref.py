"""Host restatement of the MXFP6 scheme of the block linears (include/longlive_hip.h ll_quantize_mx6 / ll_gemm_mx6):

  * a row is quantised along K in blocks of 32; amax = max |x| over the block's bf16 values, amax = m 2^p with m in [0.5, 1)
    (frexp); e = p - 3 + (m > 0.9375), the smallest integer with amax <= 7.5 2^e, clamped to [-127, 127]; the stored byte is e + 127
    (E8M0), an all-zero block stores 127 and codes 0;
  * codes = OCP FP6 E2M3 of x 2^-e (sign bit 5, exponent bits 4-3 with bias 1, mantissa bits 2-0; subnormals 0.125 m), round to
    nearest with ties to the even code; never saturating under the scale rule (|x 2^-e| <= 7.5);
  * packed storage: K % 256 == 0, 3K/4 bytes per row in 192-byte super-blocks of 256 k; the 32-k block j of a super-block sits at
    byte 48 (j % 4) + 24 (j // 4), code i of the block in bits 6i .. 6i + 5 of its little-endian 192-bit word;
  * y = epilogue(sum_k (cx 2^ex)(cw 2^ew) + bias) in fp32, written as bf16 by the bf16 GEMM's epilogues.

The rounding here is a nearest-value search over the 32 magnitudes in float64, independent of the kernels' integer bit arithmetic.
tests/quant_ref.py puts the oracle's six per-token block linears on this scheme (mode "mxfp6")."""
from typing import Tuple

import numpy as np
import torch
from torch import Tensor

BLOCK = 32
SUPER = 256
MAXV = 7.5


def _magnitudes() -> np.ndarray:
    """The 32 non-negative E2M3 values by code (bits 4-0)."""
    v = np.zeros(32)
    for c in range(32):
        ex, mt = c >> 3, c & 7
        v[c] = mt / 8.0 if ex == 0 else (1.0 + mt / 8.0) * 2.0 ** (ex - 1)
    return v


MAG = _magnitudes()


def decode(codes) -> np.ndarray:
    """float64 values of 6-bit codes (any shape, integer array)."""
    c = np.asarray(codes, dtype=np.int64)
    return np.where(c & 0x20, -1.0, 1.0) * MAG[c & 0x1F]


def encode(v) -> np.ndarray:
    """6-bit codes (uint8) of float64 values |v| <= 7.5: nearest E2M3 value, ties to the even code; the sign bit follows v's."""
    v = np.asarray(v, dtype=np.float64)
    a = np.abs(v)
    assert (a <= MAXV).all(), a.max()
    hi = np.clip(np.searchsorted(MAG, a, side="left"), 0, 31)            # first magnitude >= a
    lo = np.clip(hi - 1, 0, 31)
    dl, dh = a - MAG[lo], MAG[hi] - a
    pick_hi = (dh < dl) | ((dh == dl) & (hi % 2 == 0))
    c = np.where(a == MAG[hi], hi, np.where(pick_hi, hi, lo))
    return (c | np.where(np.signbit(v), 0x20, 0)).astype(np.uint8)


def scale_exp(amax: Tensor) -> Tensor:
    """Block exponent e (int32) of float32 block maxima (>= 0)."""
    m, p = torch.frexp(amax.float())
    e = p - 3 + (m > 0.9375).to(torch.int32)
    return torch.where(amax > 0, e, torch.zeros_like(e)).clamp(-127, 127)


def quantize_codes(x: Tensor) -> Tuple[np.ndarray, Tensor]:
    """bf16 [..., K] -> (6-bit codes uint8 [rows, K] unpacked, uint8 E8M0 scales [rows, K / 32])."""
    K = x.shape[-1]
    assert K % BLOCK == 0
    xf = x.to(torch.bfloat16).float().reshape(-1, K // BLOCK, BLOCK)
    e = scale_exp(xf.abs().amax(-1))
    v = xf.double().numpy() * np.ldexp(1.0, -e.numpy().astype(np.int64))[..., None]
    return encode(v).reshape(-1, K), (e + 127).to(torch.uint8)


def pack(codes: np.ndarray) -> np.ndarray:
    """6-bit codes [rows, K] (K % 256 == 0) -> packed bytes [rows, 3K/4]."""
    rows, K = codes.shape
    assert K % SUPER == 0
    c = np.asarray(codes, dtype=np.uint8).reshape(rows, K // SUPER, 8, 32)           # (row, super-block, block, code)
    bits = ((c[..., None] >> np.arange(6, dtype=np.uint8)) & 1).reshape(rows, K // SUPER, 8, 192)
    blocks = np.packbits(bits, axis=-1, bitorder="little")                              # (..., 8 blocks, 24 bytes)
    blocks = blocks.reshape(rows, K // SUPER, 2, 4, 24).transpose(0, 1, 3, 2, 4)        # block 4 s + g -> slot 2 g + s
    return np.ascontiguousarray(blocks).reshape(rows, K // 4 * 3)


def unpack(packed: np.ndarray) -> np.ndarray:
    """packed bytes [rows, 3K/4] -> 6-bit codes [rows, K]."""
    p = np.asarray(packed, dtype=np.uint8)
    rows, nb = p.shape
    assert nb % 192 == 0
    ns = nb // 192
    blocks = p.reshape(rows, ns, 4, 2, 24).transpose(0, 1, 3, 2, 4).reshape(rows, ns, 8, 24)
    bits = np.unpackbits(blocks, axis=-1, bitorder="little").reshape(rows, ns, 8, 32, 6)
    codes = (bits * (1 << np.arange(6, dtype=np.uint8))).sum(-1).astype(np.uint8)
    return codes.reshape(rows, ns * SUPER)


def quantize(x: Tensor) -> Tuple[Tensor, Tensor]:
    """bf16 [..., K] -> (packed uint8 [..., 3K/4], uint8 scales [rows, K / 32]), the library's layout."""
    codes, s = quantize_codes(x)
    K = x.shape[-1]
    return torch.from_numpy(pack(codes)).reshape(*x.shape[:-1], K // 4 * 3), s


def dequantize(packed: Tensor, scales: Tensor) -> Tensor:
    """float64 [rows, K] = code * 2^(byte - 127)."""
    p = packed.cpu().reshape(-1, packed.shape[-1]).numpy()
    c = torch.from_numpy(decode(unpack(p)))
    K = c.shape[-1]
    s = torch.pow(2.0, scales.cpu().double() - 127).reshape(c.shape[0], K // BLOCK, 1)
    return (c.reshape(-1, K // BLOCK, BLOCK) * s).reshape(-1, K)


def mx6_matmul(x: Tensor, w_deq: Tensor) -> Tensor:
    """fp64 sum of the dequantised products: x bf16 [..., K] quantised here, w_deq [N, K] fp64."""
    return dequantize(*quantize(x.reshape(-1, x.shape[-1]))) @ w_deq.t()
