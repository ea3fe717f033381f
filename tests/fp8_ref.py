"""Host restatement of the FP8 rowwise scheme of the block linears (include/longlive_hip.h ll_quantize_rows_f8 / ll_gemm_f8):

  * rows are tokens for activations and output channels ([N, K] rows) for weights; amax = max |x| over the row's bf16 values (fp32);
  * sc = amax / 448 in fp32 (1 for an all-zero row), inv = 1 / sc in fp32;
  * code = e4m3fn(RNE(clamp(x * inv, -448, 448))), OCP e4m3fn, subnormals kept; codes uint8 [rows, K], scales fp32 [rows];
  * y = bf16(acc * (sx[m] * sw[n]) + bias) with acc = sum_k dec(xq[m, k]) dec(wq[n, k]) (fp32), then the epilogue's tail -- the
    rounding points of the oracle's int8 linears (oracle/ref_model.py RefModel.lin).

tests/quant_ref.py puts the oracle's six per-token block linears on this scheme (mode "fp8_rowwise")."""
from typing import Tuple

import numpy as np
import torch
from torch import Tensor

FP8 = torch.float8_e4m3fn
MAX = 448.0


def quantize(x: Tensor) -> Tuple[Tensor, Tensor]:
    """bf16 [..., K] -> (e4m3fn codes as uint8 [..., K], fp32 scales [rows])."""
    K = x.shape[-1]
    xf = x.to(torch.bfloat16).float().reshape(-1, K)
    amax = xf.abs().amax(-1)
    sc = torch.where(amax > 0, amax / MAX, torch.ones_like(amax))
    inv = 1.0 / sc
    codes = (xf * inv.unsqueeze(-1)).clamp(-MAX, MAX).to(FP8).view(torch.uint8)
    return codes.reshape(x.shape), sc


def e4m3_rne(v: np.ndarray) -> np.ndarray:
    """Independent integer form of the code of fp32 values already clamped to [-448, 448]: the fp32 mantissa rounded to 3 bits
    (ties to even) in the normal range (>= 2^-6), multiples of 2^-9 below it.  Checks torch's conversion in the host tests."""
    v = np.asarray(v, dtype=np.float32)
    b = v.view(np.uint32)
    sign = ((b >> 24) & 0x80).astype(np.uint32)
    ab = b & np.uint32(0x7FFFFFFF)
    a = np.abs(v)
    r = (ab.astype(np.uint64) + 0x7FFFF + ((ab >> 20) & 1)) >> 20
    normal = (r - ((127 - 7) << 3)).astype(np.int64)
    sub = np.rint(a.astype(np.float64) * 512.0).astype(np.int64)
    c = np.where(a >= 2.0 ** -6, normal, sub)
    return (sign | c.astype(np.uint32)).astype(np.uint8)


def decode(codes: Tensor) -> Tensor:
    """float64 values of uint8 e4m3fn codes."""
    return codes.cpu().view(FP8).double()


def dequantize(codes: Tensor, scales: Tensor) -> Tensor:
    """float64 [rows, K] = dec(code) * scale."""
    K = codes.shape[-1]
    return decode(codes).reshape(-1, K) * scales.cpu().double().reshape(-1, 1)


def f8_linear(x: Tensor, wq: Tensor, sw: Tensor, bias: Tensor) -> Tensor:
    """bf16 [rows, N] = bf16(acc * (sx sw) + bias), x bf16 [rows, K] quantised here, (wq, sw) the packed weight."""
    xq, sx = quantize(x)
    acc = (decode(xq) @ decode(wq).t()).float()          # products of two e4m3 values are exact; the fp32 sum is the kernel's to ~1 ulp
    y = acc * (sx.float().unsqueeze(1) * sw.float().unsqueeze(0)) + bias.float()
    return y.to(torch.bfloat16)
