"""Host restatement of the W4A6 scheme of the block linears (include/longlive_hip.h ll_quantize_mx4 / ll_gemm_mx4w6):

  * weights are quantised along K in blocks of 32; amax = max |x| over the block's bf16 values, amax = m 2^p with m in [0.5, 1)
    (frexp); e = p - 3 + (m > 0.75), the smallest integer with amax <= 6 2^e, clamped to [-127, 127]; the stored byte is e + 127
    (E8M0), an all-zero block stores 127 and codes 0;
  * codes = OCP FP4 E2M1 of x 2^-e (sign bit 3, exponent bits 2-1 with bias 1, mantissa bit 0; the subnormal 0.5), round to nearest
    with ties to the even code; never saturating under the scale rule (|x 2^-e| <= 6);
  * packed storage: K % 256 == 0, K/2 bytes per row in 128-byte super-blocks of 256 k; the 32-k block j of a super-block sits at
    byte 32 (j % 4) + 16 (j // 4), code i of the block in bits 4i .. 4i + 3 of its little-endian 128-bit word;
  * activations are MXFP6 (tests/mx6_ref.py); y = epilogue(sum_k (cx 2^ex)(cw 2^ew) + bias) in fp32, written as bf16 by the bf16
    GEMM's epilogues.

The rounding here is a nearest-value search over the 8 magnitudes in float64, independent of the kernels' integer bit arithmetic.
tests/quant_ref.py puts the oracle's six per-token block linears on this scheme: mode "mxfp4_a6" (these weights, MXFP6 activations)
and mode "mxfp4_a4" (this scheme on both sides)."""
from typing import Tuple

import numpy as np
import torch
from torch import Tensor

BLOCK = 32
SUPER = 256
MAXV = 6.0
MAG = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])          # the 8 non-negative E2M1 values by code (bits 2-0)


def decode(codes) -> np.ndarray:
    """float64 values of 4-bit codes (any shape, integer array)."""
    c = np.asarray(codes, dtype=np.int64)
    return np.where(c & 0x8, -1.0, 1.0) * MAG[c & 0x7]


def encode(v) -> np.ndarray:
    """4-bit codes (uint8) of float64 values |v| <= 6: nearest E2M1 value, ties to the even code; the sign bit follows v's."""
    v = np.asarray(v, dtype=np.float64)
    a = np.abs(v)
    assert (a <= MAXV).all(), a.max()
    hi = np.clip(np.searchsorted(MAG, a, side="left"), 0, 7)             # first magnitude >= a
    lo = np.clip(hi - 1, 0, 7)
    dl, dh = a - MAG[lo], MAG[hi] - a
    pick_hi = (dh < dl) | ((dh == dl) & (hi % 2 == 0))
    c = np.where(a == MAG[hi], hi, np.where(pick_hi, hi, lo))
    return (c | np.where(np.signbit(v), 0x8, 0)).astype(np.uint8)


def scale_exp(amax: Tensor) -> Tensor:
    """Block exponent e (int32) of float32 block maxima (>= 0)."""
    m, p = torch.frexp(amax.float())
    e = p - 3 + (m > 0.75).to(torch.int32)
    return torch.where(amax > 0, e, torch.zeros_like(e)).clamp(-127, 127)


def quantize_codes(x: Tensor) -> Tuple[np.ndarray, Tensor]:
    """bf16 [..., K] -> (4-bit codes uint8 [rows, K] unpacked, uint8 E8M0 scales [rows, K / 32])."""
    K = x.shape[-1]
    assert K % BLOCK == 0
    xf = x.to(torch.bfloat16).float().reshape(-1, K // BLOCK, BLOCK)
    e = scale_exp(xf.abs().amax(-1))
    v = xf.double().numpy() * np.ldexp(1.0, -e.numpy().astype(np.int64))[..., None]
    return encode(v).reshape(-1, K), (e + 127).to(torch.uint8)


def pack(codes: np.ndarray) -> np.ndarray:
    """4-bit codes [rows, K] (K % 256 == 0) -> packed bytes [rows, K/2]."""
    rows, K = codes.shape
    assert K % SUPER == 0
    c = np.asarray(codes, dtype=np.uint8).reshape(rows, K // SUPER, 8, 16, 2)         # (row, super-block, block, byte, nibble)
    blocks = c[..., 0] | (c[..., 1] << 4)                                             # (..., 8 blocks, 16 bytes)
    blocks = blocks.reshape(rows, K // SUPER, 2, 4, 16).transpose(0, 1, 3, 2, 4)      # block 4 s + g -> slot 2 g + s
    return np.ascontiguousarray(blocks).reshape(rows, K // 2)


def unpack(packed: np.ndarray) -> np.ndarray:
    """packed bytes [rows, K/2] -> 4-bit codes [rows, K]."""
    p = np.asarray(packed, dtype=np.uint8)
    rows, nb = p.shape
    assert nb % 128 == 0
    ns = nb // 128
    blocks = p.reshape(rows, ns, 4, 2, 16).transpose(0, 1, 3, 2, 4).reshape(rows, ns, 8, 16)
    codes = np.stack([blocks & 0xF, blocks >> 4], axis=-1)
    return codes.reshape(rows, ns * SUPER).astype(np.uint8)


def quantize(x: Tensor) -> Tuple[Tensor, Tensor]:
    """bf16 [..., K] -> (packed uint8 [..., K/2], uint8 scales [rows, K / 32]), the library's layout."""
    codes, s = quantize_codes(x)
    K = x.shape[-1]
    return torch.from_numpy(pack(codes)).reshape(*x.shape[:-1], K // 2), s


def dequantize(packed: Tensor, scales: Tensor) -> Tensor:
    """float64 [rows, K] = code * 2^(byte - 127)."""
    p = packed.cpu().reshape(-1, packed.shape[-1]).numpy()
    c = torch.from_numpy(decode(unpack(p)))
    K = c.shape[-1]
    s = torch.pow(2.0, scales.cpu().double() - 127).reshape(c.shape[0], K // BLOCK, 1)
    return (c.reshape(-1, K // BLOCK, BLOCK) * s).reshape(-1, K)
