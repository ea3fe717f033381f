"""tests/quant_ref.py's QuantRefModel on the host: for every mode its block linears equal the formula written out here from the
scheme modules, every other linear is the oracle's own, and mxfp4_a4's activations go through the E2M1 scheme."""
import pytest
import torch

import fp8_ref
import mx4_ref
import mx4a4_ref
import mx6_ref
import mx_ref
from oracle import ref_model as RM
from quant_ref import SCHEMES, QuantRefModel, make_ref

bf = torch.bfloat16
LIN, OTHER = "blocks.0.ffn.0", "blocks.0.cross_attn.k"        # one of the six per-token linears, and one outside them


def _model(mode, rows=4, N=16, K=256):
    g = torch.Generator().manual_seed(7)
    sd = {}
    for name in (LIN, OTHER):
        sd[name + ".weight"] = (K ** -0.5 * torch.randn(N, K, generator=g)).to(bf)
        sd[name + ".bias"] = (0.1 * torch.randn(N, generator=g)).to(bf)
    x = torch.randn(2, rows // 2, K, generator=g).to(bf)
    cfg = RM.RefConfig(dim=K, ffn_dim=K, num_heads=2, num_layers=1, local_attn_size=3, sink_size=1)
    return make_ref(mode, cfg, sd), sd, x


def _deq(scheme, t):
    return scheme.dequantize(*scheme.quantize(t))


@pytest.mark.parametrize("mode", list(SCHEMES))
def test_block_linears_equal_the_formula_and_other_linears_are_the_oracles(mode):
    ref, sd, x = _model(mode)
    assert isinstance(ref, QuantRefModel)
    w, b, x2d = sd[LIN + ".weight"], sd[LIN + ".bias"], x.reshape(-1, x.shape[-1])
    if mode == "fp8_rowwise":
        (xq, sx), (wq, sw) = fp8_ref.quantize(x2d), fp8_ref.quantize(w)
        acc = (fp8_ref.decode(xq) @ fp8_ref.decode(wq).t()).float()
        want = (acc * (sx.unsqueeze(1) * sw.unsqueeze(0)) + b.float()).to(bf)
    else:
        act, wgt = {"mxfp8": (mx_ref, mx_ref), "mxfp6": (mx6_ref, mx6_ref), "mxfp4_a6": (mx6_ref, mx4_ref),
                    "mxfp4_a4": (mx4_ref, mx4_ref)}[mode]
        want = ((_deq(act, x2d) @ _deq(wgt, w).t()).float() + b.float()).to(bf)
    got = ref.lin(x, LIN)
    assert got.dtype == bf and got.shape == (2, 2, 16)
    assert torch.equal(got.reshape(4, 16), want)
    assert torch.equal(ref.lin(x, LIN), got)                    # the cached weight pack gives the same bits
    plain = RM.RefModel(ref.cfg, sd)
    assert not torch.equal(got, plain.lin(x, LIN))
    assert torch.equal(ref.lin(x, OTHER), plain.lin(x, OTHER))


def test_make_ref_gives_the_oracles_own_models_for_bf16_and_int8():
    for mode in (None, "int8"):
        ref, sd, x = _model(mode)
        assert type(ref) is RM.RefModel and ref.quant == mode
        assert torch.equal(ref.lin(x, LIN), RM.RefModel(ref.cfg, sd, quant=mode).lin(x, LIN))


def test_mxfp4_a4_quantises_the_activations_as_mxfp4():
    """The activations of the mxfp4_a4 linears go through the E2M1 scheme: the product equals the one of the dequantised MXFP4
    activations, and differs from the MXFP6 activations' (tests/mx6_ref.py, the mxfp4_a6 mode) on Gaussian data."""
    ref, sd, x = _model("mxfp4_a4", rows=16, N=8, K=512)
    x2d, b = x.reshape(-1, 512), sd[LIN + ".bias"]
    w = _deq(mx4_ref, sd[LIN + ".weight"])
    xd = _deq(mx4_ref, x2d)
    got = ref.lin(x, LIN).reshape(16, 8)
    assert torch.equal(got, ((xd @ w.t()).float() + b.float()).to(bf))
    assert torch.equal(mx4a4_ref.mx4_matmul(x2d, w), xd @ w.t())
    assert set(torch.unique(xd.abs() / torch.pow(2.0, mx4_ref.quantize(x2d)[1].double() - 127).repeat_interleave(32, 1)).tolist()) <= \
        {0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0}
    assert not torch.allclose(xd @ w.t(), mx6_ref.mx6_matmul(x2d, w))
    assert not torch.equal(got, make_ref("mxfp4_a6", ref.cfg, sd).lin(x, LIN).reshape(16, 8))
