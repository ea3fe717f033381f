"""What the model-level tests (tests/test_quant_model_gpu.py) assert for each quantised mode of the block linears: plain data, one
row per mode of longlive_amd.model._QUANT_MODES.  The numbers were measured on one MI355X and are recorded in DESIGN.md; a
model-level bound is about twice its measured distance unless the row says why not."""
from dataclasses import dataclass
from typing import Dict, Optional, Tuple


@dataclass(frozen=True)
class Band:
    """rel-L2 < rel and, where the row gives one, cosine > cos or 1 - cosine < one_minus_cos."""
    rel: float
    cos: Optional[float] = None
    one_minus_cos: Optional[float] = None

    def holds(self, r, c):
        return (r < self.rel and (self.cos is None or c > self.cos)
                and (self.one_minus_cos is None or 1 - c < self.one_minus_cos))


@dataclass(frozen=True)
class Toy:
    """The toy model beside MX self-attention: worst x0 rel-L2 to the oracle with this mode's linears < bound, and smaller than to
    the oracle with `other` linears (a mode, or None for bf16 linears)."""
    bound: float
    other: Optional[str]


@dataclass(frozen=True)
class Row:
    neighbour: Optional[str]                 # the mode the full-depth runs are held against (None: our bf16 path)
    seed: int                                # hash seed of the block test's inputs
    block: Band                              # one real-shape block against the mode's own oracle
    steady: Band                             # 30 layers, steady state, against the reference's bf16 golden
    config2: Band                            # config 2 free-running, per block, against the reference's bf16 latents
    measured: Optional[Dict[str, float]] = None
    block_exclude: Tuple[Optional[str], ...] = ()   # oracles the block bound must exclude: the own oracle sits further from each
    block_closer_than: Tuple[Optional[str], ...] = ()   # oracles the block's output must sit further from than from its own
    block_packs_of: Optional[str] = None     # the mode whose weight packs this mode's must equal bit for bit
    near: Optional[Band] = None              # steady state: within this band of the neighbour's run
    apart: Optional[float] = None            # steady state and every config 2 block: rel-L2 to the neighbour's run above this
    growth_inclusive: bool = False           # config 2, last block vs 1.25x the first: <= (True) or < (False)
    toy: Optional[Toy] = None


# int8 and mxfp8 keep absolute bounds: the bf16 block test's rel-L2 < 6e-3 / cosine > 0.9999 (int8 measured 3.0e-3; the same block
# int8 vs bf16: 3.9e-3), 30 layers within 6e-2 / 0.998 of our bf16 path and 7e-2 / 0.997 of the reference's bf16 golden, config 2 per
# block within that one-forward bound (DESIGN.md sections 2 and 5b.1).  mxfp8's block must also sit closer to the MX restatement than
# to the bf16 oracle, so that the pass band excludes "did not quantise".
_ABS = dict(block=Band(6e-3, cos=0.9999), steady=Band(7e-2, cos=0.997), near=Band(6e-2, cos=0.998), config2=Band(7e-2, cos=0.997))

# measured on one MI355X; the model-level bounds are about twice these.  The block's is 1.8x: twice would reach the
# fp8_rowwise oracle's own 9.0e-3 distance to the bf16 oracle, and the band must exclude that oracle.
_F8 = dict(block=4.7e-3, steady_ref=4.9e-2, config2=3.4e-2, toy_attn=2.3e-3)
# measured on one MI355X; the model-level bounds are about twice these.  The block's is 1.23x: twice would reach the
# mxfp6 oracle's own 6.75e-3 distance to the MXFP8 oracle, and the band must exclude that oracle.
_MX6 = dict(block=4.9e-3, steady_ref=4.9e-2, config2=3.7e-2, toy_attn=2.2e-3)
# measured on one MI355X; the model-level bounds are about twice these.  The 30-layer steady state's cosine to the
# reference is 0.98826: 1 - cos ~ rel-L2^2 / 2 grows with the square of W4A6's ~3x MXFP6 distance, so its bound is 0.98, not 0.99.
_A6 = dict(block=4.93e-3, steady_ref=0.154, config2=0.135, toy_attn=2.12e-3)
# measured on one MI355X; the model-level bounds are about twice these (rel-L2, and 1 - cos).  The block bound is
# 1.7x its measured distance: the mxfp4_a4 oracle itself sits 3.06e-2 from the mxfp4_a6 oracle (3.86e-2 from the bf16 oracle), and the
# bound must stay below both.
_A4 = dict(block=1.50e-2, steady_ref=0.203, steady_cos=0.97952, config2=0.155, config2_cos=0.98793, toy_attn=3.23e-3)

MODES = {
    "int8": Row(neighbour=None, seed=71, **_ABS),
    "mxfp8": Row(neighbour=None, seed=71, block_closer_than=(None,), **_ABS),
    "fp8_rowwise": Row(
        neighbour="int8", seed=71, measured=_F8, block=Band(8.5e-3), block_exclude=(None, "int8"),
        steady=Band(2 * _F8["steady_ref"], cos=0.995), config2=Band(2 * _F8["config2"], cos=0.995), apart=1e-3,
        toy=Toy(2 * _F8["toy_attn"], other=None)),
    "mxfp6": Row(
        neighbour="mxfp8", seed=71, measured=_MX6, block=Band(6.0e-3), block_exclude=(None, "mxfp8"),
        steady=Band(2 * _MX6["steady_ref"], cos=0.99), config2=Band(2 * _MX6["config2"], cos=0.99), apart=1e-3,
        toy=Toy(2 * _MX6["toy_attn"], other=None)),
    "mxfp4_a6": Row(
        neighbour="mxfp6", seed=73, measured=_A6, block=Band(1.0e-2), block_exclude=(None, "mxfp6"),
        steady=Band(2 * _A6["steady_ref"], cos=0.98), config2=Band(2 * _A6["config2"], cos=0.99), apart=1e-2,
        growth_inclusive=True, toy=Toy(2 * _A6["toy_attn"], other="mxfp6")),
    "mxfp4_a4": Row(
        neighbour="mxfp4_a6", seed=73, measured=_A4, block=Band(2.5e-2), block_exclude=(None, "mxfp4_a6"), block_packs_of="mxfp4_a6",
        steady=Band(2 * _A4["steady_ref"], one_minus_cos=2 * (1 - _A4["steady_cos"])),
        config2=Band(2 * _A4["config2"], one_minus_cos=2 * (1 - _A4["config2_cos"])), apart=1e-2,
        growth_inclusive=True, toy=Toy(2 * _A4["toy_attn"], other="mxfp4_a6")),
}
