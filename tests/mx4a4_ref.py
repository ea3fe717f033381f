"""Host restatement of the W4A4 mode of the block linears (include/longlive_hip.h ll_gemm_mx4): activations and weights both in
tests/mx4_ref.py's scheme (per-32 E8M0 blocks with e = p - 3 + (m > 0.75), E2M1 codes rounded to nearest even, never saturating, -0
kept, packed 4 bits each in 128-byte super-blocks of 256 k); y = epilogue(sum_k (cx 2^ex)(cw 2^ew) + bias) in fp32, written as bf16 by
the bf16 GEMM's epilogues.  Mx4a4RefModel is Mx4a6RefModel with the activations of the six block linears passed through
mx4_ref.quantize / dequantize instead of MXFP6 (the oracle itself is untouched)."""
from torch import Tensor

import mx4_ref


def mx4_matmul(x: Tensor, w_deq: Tensor) -> Tensor:
    """fp64 sum of the dequantised products: x bf16 [..., K] quantised here as MXFP4, w_deq [N, K] fp64."""
    return mx4_ref.dequantize(*mx4_ref.quantize(x.reshape(-1, x.shape[-1]))) @ w_deq.t()


class Mx4a4RefModel(mx4_ref.Mx4a6RefModel):
    """Mx4a6RefModel whose six per-token block linears also take E2M1-dequantised activations."""

    def lin(self, x: Tensor, name: str) -> Tensor:
        if not (name.startswith("blocks.") and name.endswith(self._W8A8)):
            return super().lin(x, name)
        assert name not in self.lora
        if name not in self._wmx6:
            self._wmx6[name] = mx4_ref.dequantize(*mx4_ref.quantize(self.sd[name + ".weight"]))
        acc = mx4_matmul(x.to(self.dtype), self._wmx6[name]).float()
        y = acc + self.sd[name + ".bias"].float()
        return y.to(self.dtype).reshape(*x.shape[:-1], -1)
