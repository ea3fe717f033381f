"""The host oracle of the quantised block linears: the oracle's RefModel with the six per-token block linears (self_attn q/k/v/o,
cross_attn q/o, ffn.0, ffn.2) on one mode of longlive_amd.model._QUANT_MODES (the oracle itself is untouched).  A mode is a pair of
scheme modules, one for the activations and one for the weights; the schemes themselves are restated in tests/mx_ref.py (MXFP8),
tests/fp8_ref.py (FP8 rowwise), tests/mx6_ref.py (MXFP6) and tests/mx4_ref.py (MXFP4 E2M1).

  * block-scaled modes: y = bf16(float(dequant(quant(x)) @ dequant(quant(w))^T in fp64) + bias in fp32);
  * fp8_rowwise: fp8_ref.f8_linear, the rounding points of the oracle's int8 linears;
  * int8 is the oracle's own RefModel(quant="int8"); make_ref returns the right model for every mode."""
from typing import Optional

from torch import Tensor

import fp8_ref
import mx4_ref
import mx6_ref
import mx_ref
from oracle import ref_model as RM

# mode -> (activation scheme, weight scheme)
SCHEMES = {
    "mxfp8": (mx_ref, mx_ref),
    "fp8_rowwise": (fp8_ref, fp8_ref),
    "mxfp6": (mx6_ref, mx6_ref),
    "mxfp4_a6": (mx6_ref, mx4_ref),
    "mxfp4_a4": (mx4_ref, mx4_ref),
}


class QuantRefModel(RM.RefModel):
    """RefModel whose six per-token block linears run `mode`.  (mode=None keeps the oracle's bf16 linears: what a subclass that
    changes something else, tests/mx_attn_ref.py's attention, is without quantised linears.)"""

    def __init__(self, *a, mode: Optional[str], **kw):
        super().__init__(*a, **kw)
        self.mode = mode
        self.act, self.wgt = SCHEMES[mode] if mode is not None else (None, None)
        self._w = {}                 # name -> dequantised weight (fp64), or the (codes, scales) pack of fp8_rowwise

    def lin(self, x: Tensor, name: str) -> Tensor:
        if self.mode is None or not (name.startswith("blocks.") and name.endswith(self._W8A8)):
            return super().lin(x, name)
        assert name not in self.lora
        x2d = x.to(self.dtype).reshape(-1, x.shape[-1])
        bias = self.sd[name + ".bias"]
        if name not in self._w:
            pack = self.wgt.quantize(self.sd[name + ".weight"])
            self._w[name] = pack if self.mode == "fp8_rowwise" else self.wgt.dequantize(*pack)
        if self.mode == "fp8_rowwise":
            y = fp8_ref.f8_linear(x2d, *self._w[name], bias)
        else:
            y = (self.act.dequantize(*self.act.quantize(x2d)) @ self._w[name].t()).float() + bias.float()
        return y.to(self.dtype).reshape(*x.shape[:-1], -1)


def make_ref(mode: Optional[str], cfg: RM.RefConfig, sd, **kw) -> RM.RefModel:
    """The host model of any mode of _QUANT_MODES: None (bf16) and "int8" are the oracle's own."""
    if mode in (None, "int8"):
        return RM.RefModel(cfg, sd, quant=mode, **kw)
    return QuantRefModel(cfg, sd, mode=mode, **kw)
