"""Host restatement of the W4A4 mode of the block linears (include/longlive_hip.h ll_gemm_mx4): activations and weights both in
tests/mx4_ref.py's scheme (per-32 E8M0 blocks with e = p - 3 + (m > 0.75), E2M1 codes rounded to nearest even, never saturating, -0
kept, packed 4 bits each in 128-byte super-blocks of 256 k); y = epilogue(sum_k (cx 2^ex)(cw 2^ew) + bias) in fp32, written as bf16 by
the bf16 GEMM's epilogues.  tests/quant_ref.py's mode "mxfp4_a4" passes the activations of the six block linears through
mx4_ref.quantize / dequantize instead of MXFP6."""
from torch import Tensor

import mx4_ref


def mx4_matmul(x: Tensor, w_deq: Tensor) -> Tensor:
    """fp64 sum of the dequantised products: x bf16 [..., K] quantised here as MXFP4, w_deq [N, K] fp64."""
    return mx4_ref.dequantize(*mx4_ref.quantize(x.reshape(-1, x.shape[-1]))) @ w_deq.t()
