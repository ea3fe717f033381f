"""MXFP8 mode, host side: the scale rule of the scheme at its edges (tests/mx_ref.py), argument validation of every new entry
point before anything is launched (the library loads without a GPU), the plan string, and the switches that reach the mode."""
import pytest
import torch

import mx_ref
from longlive_amd import _lib

bf = torch.bfloat16


def _block(vals):
    x = torch.zeros(1, 32, dtype=bf)
    x[0, : len(vals)] = torch.tensor(vals, dtype=torch.float64).to(bf)
    return x


@pytest.mark.parametrize("e", [-20, -1, 0, 1, 7, 30])
def test_scale_rule_at_448_times_a_power_of_two(e):
    q, s = mx_ref.quantize(_block([448.0 * 2.0 ** e, 1.0 * 2.0 ** e]))
    assert int(s[0, 0]) == e + 127
    assert q.view(torch.uint8)[0, 0] == 0x7E                  # 448 exactly, not saturated past it
    # the next bf16 above 448 2^e needs the next exponent
    nxt = torch.tensor([448.0 * 2.0 ** e], dtype=bf).view(torch.int16) + 1
    q, s = mx_ref.quantize(_block([float(nxt.view(bf).float())]))
    assert int(s[0, 0]) == e + 128
    assert q.float()[0, 0] <= 448


def test_scale_rule_zero_block_subnormals_and_negative_maxima():
    q, s = mx_ref.quantize(torch.zeros(2, 64, dtype=bf))
    assert (s == 127).all() and (q.view(torch.uint8) == 0).all()
    # bf16 subnormals: the exponent clamps at -127 (2^-133 2^127 = 2^-6, the smallest e4m3 normal; 3 2^-133 -> 1.5 2^-5)
    q, s = mx_ref.quantize(_block([2.0 ** -133, 3 * 2.0 ** -133, -(2.0 ** -133)]))
    assert int(s[0, 0]) == 0
    assert q.view(torch.uint8)[0, :3].tolist() == [0x08, 0x14, 0x88]
    # e4m3 subnormal codes are kept, not flushed: 2^-8 and 3 2^-10 beside 448 (e = 0) are 2 and 1.5 steps of 2^-9 (RNE -> 2)
    q, s = mx_ref.quantize(_block([448.0, 2.0 ** -8, 3 * 2.0 ** -10, -(2.0 ** -9)]))
    assert int(s[0, 0]) == 127 and q.view(torch.uint8)[0, :4].tolist() == [0x7E, 0x02, 0x02, 0x81]
    # the maximum magnitude is negative: same exponent as its positive twin, negative code
    q, s = mx_ref.quantize(_block([-448.0 * 8, 3.0]))
    assert int(s[0, 0]) == 127 + 3 and q.view(torch.uint8)[0, 0] == 0xFE
    # codes are RNE of x 2^-e: 17 * 2^-e with e = p - 9 ... 17 = 1.0001b x 2^4 rounds to 16 (tie to even) in e4m3
    q, s = mx_ref.quantize(_block([17.0, 448.0]))
    assert int(s[0, 0]) == 127 and float(q.float()[0, 0]) == 16.0


def test_dequantize_round_trip_is_within_half_an_e4m3_step():
    x = (torch.randn(64, 256, generator=torch.Generator().manual_seed(0)) * 3).to(bf)
    d = mx_ref.dequantize(*mx_ref.quantize(x))
    amax = x.float().reshape(64, 8, 32).abs().amax(-1, keepdim=True).double()
    err = (d.reshape(64, 8, 32) - x.double().reshape(64, 8, 32)).abs()
    assert (err <= amax * 2.0 ** -4 + 1e-30).all()


# every new entry point refuses bad arguments with a message, before any launch (pointer 1 = "some non-NULL pointer")
@pytest.mark.parametrize("call,needle", [
    (lambda L: L.ll_quantize_mx(1, 1, 1, 8, 40, 40, None), "multiple of 32"),
    (lambda L: L.ll_quantize_mx(1, 0, 1, 8, 64, 64, None), "codes and scales are required"),
    (lambda L: L.ll_quantize_mx(1, 1, 1, 8, 64, 32, None), "ldx=32"),
    (lambda L: L.ll_gemm_mx(1, 1, 1, 1, 1, 1, 0, 0, 64, 256, 96, 256, 0, 0, 0, 0, 0, 0, 0, 0, None), "positive multiple of 128"),
    (lambda L: L.ll_gemm_mx(1, 0, 1, 1, 1, 1, 0, 0, 64, 256, 128, 256, 0, 0, 0, 0, 0, 0, 0, 0, None), "codes and scales of both operands"),
    (lambda L: L.ll_gemm_mx(1, 1, 1, 1, 0, 1, 0, 0, 64, 256, 128, 256, 0, 0, 0, 0, 0, 0, 0, 0, None), "bias is required"),
    (lambda L: L.ll_gemm_mx(1, 1, 1, 1, 1, 1, 1, 1, 64, 256, 128, 256, 1, 0, 0, 0, 0, 0, 0, 0, None), "exactly one of out"),
    (lambda L: L.ll_gemm_mx(1, 1, 1, 1, 1, 0, 1, 0, 64, 256, 128, 256, 1, 0, 0, 0, 0, 0, 0, 0, None), "both codes and scales"),
    (lambda L: L.ll_gemm_mx(1, 1, 1, 1, 1, 0, 1, 1, 64, 256, 128, 256, 0, 0, 0, 0, 0, 0, 0, 0, None), "GELU epilogue only"),
    (lambda L: L.ll_gemm_mx(1, 1, 1, 1, 1, 0, 1, 1, 64, 264, 128, 264, 1, 0, 0, 0, 0, 0, 0, 0, None), "multiple of 32"),
    (lambda L: L.ll_gemm_mx(1, 1, 1, 1, 1, 1, 0, 0, 64, 256, 128, 256, 2, 0, 0, 0, 0, 0, 0, 0, None), "needs res and e"),
    (lambda L: L.ll_gemm_mx(1, 1, 1, 1, 1, 1, 0, 0, 64, 256, 128, 256, 3, 0, 0, 0, 0, 0, 0, 0, None), "needs res"),
    (lambda L: L.ll_gemm_mx(1, 1, 1, 1, 1, 1, 0, 0, 64, 256, 128, 256, 7, 0, 0, 0, 0, 0, 0, 0, None), "unknown epilogue"),
    (lambda L: L.ll_gemm_mx_qkv(1, 1, 1, 1, 1, 1, 64, 768, 128, 768, 0, 1, 64, 128, 0, 0, 64, None), "cache_v is required"),
    (lambda L: L.ll_gemm_mx_qkv(1, 1, 1, 1, 1, 1, 64, 768, 128, 768, 1, 2, 64, 128, 0, 0, 64, None), "is not B=2"),
    (lambda L: L.ll_gemm_mx_qkv(1, 1, 1, 1, 1, 1, 64, 768, 128, 768, 1, 1, 64, 128, 100, 0, 64, None), "outside cache"),
    (lambda L: L.ll_gemm_mx_qkv(1, 1, 1, 1, 1, 1, 64, 768, 136, 768, 1, 1, 64, 128, 0, 0, 64, None), "positive multiple of 128"),
    (lambda L: L.ll_ln_modulate_mx(1, 1, 1, 1, 0, 6, 0, 1, 1, 9, 48, 3, 1e-6, None), "multiple of 32"),
    (lambda L: L.ll_ln_modulate_mx(1, 0, 1, 1, 0, 6, 0, 1, 1, 9, 64, 3, 1e-6, None), "codes and scales are required"),
    (lambda L: L.ll_ln_modulate_mx(1, 1, 1, 1, 0, 6, 0, 7, 1, 9, 64, 3, 1e-6, None), "bad mod index"),
    (lambda L: L.ll_ln_modulate_mx(1, 1, 1, 1, 0, 6, 0, 1, 1, 10, 64, 3, 1e-6, None), "not divisible"),
    (lambda L: L.ll_ln_modulate_tab_mx(1, 1, 1, 0, 6, 0, 1, 1, 9, 64, 3, 1e-6, None), "x and tab are required"),
    (lambda L: L.ll_ln_modulate_tab_mx(1, 1, 1, 1, 6, 9, 1, 1, 9, 64, 3, 1e-6, None), "bad mod index"),
    (lambda L: L.ll_layernorm_affine_mx(1, 1, 1, 1, 1, 9, 2080, 1e-6, None), "<= 2048"),
    (lambda L: L.ll_layernorm_affine_mx(1, 0, 1, 1, 1, 9, 64, 1e-6, None), "x, w and b are required"),
])
def test_invalid_arguments_are_rejected_before_launch(call, needle):
    lib = _lib.load()
    rc = call(lib)
    assert rc == -1, rc
    msg = lib.ll_last_error().decode()
    assert needle in msg, msg


def test_plan_strings():
    from longlive_amd import ops
    assert ops.gemm_plan_mx(4680, 8960, 1536) == "gemm_mx_kernel tile 256x128, 1330 workgroups, groups of 4 m-tiles"
    assert ops.gemm_plan_mx(4680, 1536, 8960) == "gemm_mx_kernel tile 256x128, 228 workgroups, groups of 4 m-tiles"
    assert ops.gemm_plan_mx(4680, 4608, 1536).startswith("gemm_mx_kernel tile 256x128, 684 workgroups")


def test_set_quant_and_cli_key():
    from longlive_amd import cli, synth
    from longlive_amd.model import CausalWanModelHIP
    m = CausalWanModelHIP(synth.toy_config(), device="cpu")
    assert m.set_quant("mxfp8").quant == "mxfp8"
    assert m.set_quant(None).quant is None
    with pytest.raises(ValueError):
        m.set_quant("fp8")
    assert [cli.quant_mode(v) for v in (None, "none", "int8", "mxfp8", "MXFP8")] == [None, None, "int8", "mxfp8", "mxfp8"]
    with pytest.raises(ValueError):
        cli.quant_mode("fp8")
