"""Host restatement of the MXFP8 scheme of the block linears (include/longlive_hip.h ll_quantize_mx / ll_gemm_mx):

  * a row is quantised along K in blocks of 32; amax = max |x| over the block's bf16 values, amax = m 2^p with m in [0.5, 1)
    (frexp); e = p - 9 + (m > 0.875), the smallest integer with amax <= 448 2^e, clamped to [-127, 127]; the stored byte is e + 127
    (E8M0), an all-zero block stores 127 and codes 0;
  * codes = e4m3fn(RNE(x 2^-e)), OCP e4m3fn, subnormals kept, saturating at +-448 (reached only under the clamp);
  * y = epilogue(sum_k (cx 2^ex)(cw 2^ew) + bias) in fp32, written as bf16 by the bf16 GEMM's epilogues.

tests/quant_ref.py puts the oracle's six per-token block linears on this scheme (mode "mxfp8")."""
from typing import Tuple

import torch
from torch import Tensor

FP8 = torch.float8_e4m3fn
BLOCK = 32


def scale_exp(amax: Tensor) -> Tensor:
    """Block exponent e (int32) of float32 block maxima (>= 0)."""
    m, p = torch.frexp(amax.float())
    e = p - 9 + (m > 0.875).to(torch.int32)
    return torch.where(amax > 0, e, torch.zeros_like(e)).clamp(-127, 127)


def quantize(x: Tensor) -> Tuple[Tensor, Tensor]:
    """bf16 [..., K] -> (e4m3fn codes [..., K], uint8 E8M0 scales [rows, K / 32])."""
    K = x.shape[-1]
    assert K % BLOCK == 0
    xf = x.to(torch.bfloat16).float().reshape(-1, K // BLOCK, BLOCK)
    e = scale_exp(xf.abs().amax(-1))
    mul = torch.pow(2.0, -e.double()).float()                  # exact powers of two (2^-127 .. 2^127)
    codes = (xf * mul.unsqueeze(-1)).to(FP8).reshape(x.shape)
    return codes, (e + 127).to(torch.uint8)


def dequantize(codes: Tensor, scales: Tensor) -> Tensor:
    """float64 [rows, K] = code * 2^(byte - 127)."""
    K = codes.shape[-1]
    c = codes.reshape(-1, K // BLOCK, BLOCK).cpu().double()
    s = torch.pow(2.0, scales.cpu().double() - 127).reshape(c.shape[0], K // BLOCK, 1)
    return (c * s).reshape(-1, K)


def mx_matmul(x: Tensor, w_deq: Tensor) -> Tensor:
    """fp64 sum of the dequantised products: x bf16 [..., K] quantised here, w_deq [N, K] fp64."""
    return dequantize(*quantize(x.reshape(-1, x.shape[-1]))) @ w_deq.t()
