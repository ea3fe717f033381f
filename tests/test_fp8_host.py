"""FP8 rowwise mode, host side: the scheme at its edges (tests/fp8_ref.py) and its agreement with an independent integer rounding,
argument validation of every new entry point before anything is launched (the library loads without a GPU), the plan strings at the
production shapes, the switches that reach the mode and the re-pack after an in-place weight update."""
import numpy as np
import pytest
import torch

import fp8_ref
from longlive_amd import _lib

bf = torch.bfloat16


@pytest.fixture(autouse=True)
def _scheme_is_the_librarys():
    """tests/fp8_ref.py restates ll_quantize_rows_f8 / ll_gemm_f8: its edges are pinned only where the library declares them."""
    import os
    header = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "longlive_hip.h")).read()
    assert "int ll_quantize_rows_f8(" in header and hasattr(_lib.load(), "ll_quantize_rows_f8")


def _row(vals, K=32):
    x = torch.zeros(1, K, dtype=bf)
    x[0, : len(vals)] = torch.tensor(vals, dtype=torch.float64).to(bf)
    return x


def test_all_zero_row_has_unit_scale_and_zero_codes():
    q, s = fp8_ref.quantize(torch.zeros(3, 64, dtype=bf))
    assert s.dtype == torch.float32 and (s == 1).all() and (q == 0).all()


@pytest.mark.parametrize("k", [-20, -3, 0, 1, 5, 30])
def test_amax_448_times_a_power_of_two(k):
    a = 448.0 * 2.0 ** k
    q, s = fp8_ref.quantize(_row([a, -a, a / 2, 2.0 ** k]))
    assert float(s[0]) == 2.0 ** k                                    # exact: 448 2^k / 448
    assert q[0, :4].tolist() == [0x7E, 0xFE, 0x76, 0x38]              # 448, -448, 224, 1


def test_rounding_midpoint_goes_to_the_even_code():
    # amax 448 -> sc = 1: 17 = 1.0001b x 2^4 lies halfway between 16 (mantissa 000) and 18 (001): even -> 16;
    # 19 halfway between 18 (001) and 20 (010): even -> 20
    q, s = fp8_ref.quantize(_row([448.0, 17.0, 19.0, -17.0]))
    assert float(s[0]) == 1.0
    assert fp8_ref.decode(q[0, 1:4]).tolist() == [16.0, 20.0, -16.0]


def test_subnormal_codes_appear_beside_a_large_amax():
    # sc = 1: 2^-8 and 3 2^-10 are 2 and 1.5 steps of 2^-9 (RNE -> 2), 2^-10 is half a step (-> 0), 2^-6 the smallest normal
    q, s = fp8_ref.quantize(_row([448.0, 2.0 ** -8, 3 * 2.0 ** -10, -(2.0 ** -9), 2.0 ** -10, 2.0 ** -6]))
    assert q[0, :6].tolist() == [0x7E, 0x02, 0x02, 0x81, 0x00, 0x08]


def test_product_rounding_just_above_448_saturates_instead_of_nan():
    # for some bf16 amax, sc = amax / 448 and inv = 1 / sc round so that amax * inv lands just above 448 in fp32; without the clamp
    # v_cvt_pk_fp8_f32 would write NaN there.  Searched over bf16 values: every such row must code its maximum as 448.
    hits = 0
    for bits in range(0x3F80, 0x4780, 7):                             # bf16 values 1 .. 65536
        amax = torch.tensor([bits], dtype=torch.int16).view(bf)
        a = amax.float()
        sc = a / 448.0
        prod = a * (1.0 / sc)
        if float(prod) > 448.0:
            hits += 1
            q, s = fp8_ref.quantize(_row([float(a)]))
            assert int(q[0, 0]) == 0x7E, (float(a), float(prod))      # 448, not NaN (0x7F)
    assert hits > 0, "no bf16 amax rounds above 448: the edge is not exercised"


def test_negative_zero_keeps_its_sign_bit():
    x = torch.tensor([[448.0, -0.0, 0.0, -(2.0 ** -12)]], dtype=bf)
    q, _ = fp8_ref.quantize(x)
    assert q[0].tolist() == [0x7E, 0x80, 0x00, 0x80]                 # -0 and a negative value below half a step -> -0


def test_restatement_agrees_with_an_independent_integer_rounding():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(256, 512, generator=g) * torch.logspace(-6, 3, 256).unsqueeze(1)
    x[:, :3] *= 100
    x[7] = 0
    x[9, 5:40] = 2.0 ** -20
    x = x.to(bf)
    q, s = fp8_ref.quantize(x)
    inv = 1.0 / s
    v = (x.float() * inv.unsqueeze(1)).clamp(-448, 448)
    assert np.array_equal(fp8_ref.e4m3_rne(v.numpy()), q.numpy())
    # and torch's own conversion of the clamped fp32 product, the definition the restatement uses
    assert torch.equal(v.to(torch.float8_e4m3fn).view(torch.uint8), q)


def test_dequantize_round_trip_is_within_half_an_e4m3_step_of_the_row():
    x = (torch.randn(64, 256, generator=torch.Generator().manual_seed(1)) * 3).to(bf)
    d = fp8_ref.dequantize(*fp8_ref.quantize(x))
    amax = x.float().abs().amax(-1, keepdim=True).double()
    # relative half step 2^-4 in the normal range; below 2^-6 sc the step is 2^-9 sc (half: 2^-10 sc = amax 2^-10 / 448)
    err = (d - x.double()).abs()
    assert (err <= torch.maximum(x.double().abs() * 2.0 ** -4, amax * 2.0 ** -10 / 448) * (1 + 1e-6)).all()


# every new entry point refuses bad arguments with a message, before any launch (pointer 1 = "some non-NULL pointer")
@pytest.mark.parametrize("call,needle", [
    (lambda L: L.ll_quantize_rows_f8(1, 1, 1, 8, 36, 36, None), "multiple of 8"),
    (lambda L: L.ll_quantize_rows_f8(1, 0, 1, 8, 64, 64, None), "x, codes and scales are required"),
    (lambda L: L.ll_quantize_rows_f8(1, 1, 1, 8, 64, 32, None), "ldx=32"),
    (lambda L: L.ll_gemm_f8(1, 1, 1, 1, 1, 1, 64, 256, 96, 256, 0, 0, 0, 0, 0, 0, 0, 0, None), "positive multiple of 128"),
    (lambda L: L.ll_gemm_f8(1, 0, 1, 1, 1, 1, 64, 256, 128, 256, 0, 0, 0, 0, 0, 0, 0, 0, None), "codes and scales of both operands"),
    (lambda L: L.ll_gemm_f8(1, 1, 1, 1, 1, 0, 64, 256, 128, 256, 0, 0, 0, 0, 0, 0, 0, 0, None), "out is required"),
    (lambda L: L.ll_gemm_f8(1, 1, 1, 1, 0, 1, 64, 256, 128, 256, 0, 0, 0, 0, 0, 0, 0, 0, None), "bias is required"),
    (lambda L: L.ll_gemm_f8(1, 1, 1, 1, 1, 1, 64, 256, 128, 252, 0, 0, 0, 0, 0, 0, 0, 0, None), "ldo=252"),
    (lambda L: L.ll_gemm_f8(1, 1, 1, 1, 1, 1, 64, 256, 128, 128, 0, 0, 0, 0, 0, 0, 0, 0, None), "must be >= N"),
    (lambda L: L.ll_gemm_f8(1, 1, 1, 1, 1, 1, 64, 252, 128, 256, 0, 0, 0, 0, 0, 0, 0, 0, None), "N=252"),
    (lambda L: L.ll_gemm_f8(1, 1, 1, 1, 1, 1, 64, 256, 128, 256, 2, 0, 0, 0, 0, 0, 0, 0, None), "needs res and e"),
    (lambda L: L.ll_gemm_f8(1, 1, 1, 1, 1, 1, 64, 256, 128, 256, 3, 0, 0, 0, 0, 0, 0, 0, None), "needs res"),
    (lambda L: L.ll_gemm_f8(1, 1, 1, 1, 1, 1, 64, 256, 128, 256, 7, 0, 0, 0, 0, 0, 0, 0, None), "unknown epilogue"),
    (lambda L: L.ll_gemm_f8_qkv(1, 1, 1, 1, 1, 1, 64, 768, 128, 768, 0, 1, 64, 128, 0, 0, 64, None), "cache_v is required"),
    (lambda L: L.ll_gemm_f8_qkv(1, 1, 1, 1, 1, 1, 64, 768, 128, 768, 1, 2, 64, 128, 0, 0, 64, None), "is not B=2"),
    (lambda L: L.ll_gemm_f8_qkv(1, 1, 1, 1, 1, 1, 64, 768, 128, 768, 1, 1, 64, 128, 100, 0, 64, None), "outside cache"),
    (lambda L: L.ll_gemm_f8_qkv(1, 1, 1, 1, 1, 1, 64, 768, 136, 768, 1, 1, 64, 128, 0, 0, 64, None), "positive multiple of 128"),
    (lambda L: L.ll_gemm_f8_qkv(1, 1, 0, 1, 1, 1, 64, 768, 128, 768, 1, 1, 64, 128, 0, 0, 64, None), "codes and scales of both operands"),
    (lambda L: L.ll_ln_modulate_f8(1, 1, 1, 1, 0, 6, 0, 1, 1, 9, 44, 3, 1e-6, None), "multiple of 8"),
    (lambda L: L.ll_ln_modulate_f8(1, 0, 1, 1, 0, 6, 0, 1, 1, 9, 64, 3, 1e-6, None), "codes and scales are required"),
    (lambda L: L.ll_ln_modulate_f8(1, 1, 1, 1, 0, 6, 0, 7, 1, 9, 64, 3, 1e-6, None), "bad mod index"),
    (lambda L: L.ll_ln_modulate_f8(1, 1, 1, 1, 0, 6, 0, 1, 1, 10, 64, 3, 1e-6, None), "not divisible"),
    (lambda L: L.ll_ln_modulate_tab_f8(1, 1, 1, 0, 6, 0, 1, 1, 9, 64, 3, 1e-6, None), "x and tab are required"),
    (lambda L: L.ll_ln_modulate_tab_f8(1, 1, 0, 1, 6, 0, 1, 1, 9, 64, 3, 1e-6, None), "codes and scales are required"),
    (lambda L: L.ll_ln_modulate_tab_f8(1, 1, 1, 1, 6, 9, 1, 1, 9, 64, 3, 1e-6, None), "bad mod index"),
    (lambda L: L.ll_ln_modulate_tab_f8(1, 1, 1, 1, 6, 0, 1, 1, 9, 2056, 3, 1e-6, None), "<= 2048"),
    (lambda L: L.ll_layernorm_affine_f8(1, 1, 1, 1, 1, 9, 2080, 1e-6, None), "<= 2048"),
    (lambda L: L.ll_layernorm_affine_f8(1, 0, 1, 1, 1, 9, 64, 1e-6, None), "x, w and b are required"),
    (lambda L: L.ll_layernorm_affine_f8(1, 1, 1, 0, 1, 9, 64, 1e-6, None), "codes and scales are required"),
    (lambda L: L.ll_gemm_plan_f8(64, 256, 128, None, 0), "needs an output buffer"),
])
def test_invalid_arguments_are_rejected_before_launch(call, needle):
    lib = _lib.load()
    rc = call(lib)
    assert rc == -1, rc
    msg = lib.ll_last_error().decode()
    assert needle in msg, msg


def test_plan_strings_name_the_fp8_instances_at_the_production_shapes():
    from longlive_amd import ops
    assert ops.gemm_plan_f8(4680, 4608, 1536) == "gemm_kernel_v5<f8> tile 256x192, 456 workgroups, groups of 4 m-tiles"
    assert ops.gemm_plan_f8(4680, 1536, 1536) == "gemm_kernel_v2<f8> tile 256x128, 228 workgroups, groups of 4 m-tiles"
    assert ops.gemm_plan_f8(4680, 8960, 1536) == "gemm_kernel_v5<f8> tile 256x224, 760 workgroups, groups of 4 m-tiles"
    assert ops.gemm_plan_f8(4680, 1536, 8960) == "gemm_kernel_v2<f8> tile 256x128, 228 workgroups, groups of 4 m-tiles"
    # the int8 plan of each shape names the same kernel and tile: FP8 runs on the W8A8 kernels' structure
    import ctypes
    for N, K in ((4608, 1536), (1536, 1536), (8960, 1536), (1536, 8960)):
        buf = ctypes.create_string_buffer(256)
        assert _lib.load().ll_gemm_plan(4680, N, K, 1, buf, 256) == 0
        assert ops.gemm_plan_f8(4680, N, K).replace("<f8>", "<i8>") == buf.value.decode()


def test_forced_256_wide_tiling_is_named_as_the_two_stage_kernel():
    """gemm_variant 3 (256 x 256) is an instance of gemm_kernel_v5: the plan names the device symbol, for every operand kind."""
    import ctypes
    from longlive_amd import ops
    lib = _lib.load()
    try:
        assert lib.ll_set_tuning(b"gemm_variant", 3) == 0
        buf = ctypes.create_string_buffer(256)
        plans = [ops.gemm_plan_f8(4680, 4608, 1536)]
        for int8 in (0, 1):
            assert lib.ll_gemm_plan(4680, 4608, 1536, int8, buf, 256) == 0
            plans.append(buf.value.decode())
        for plan, kind in zip(plans, ("f8", "bf16", "i8")):
            assert plan.startswith(f"gemm_kernel_v5<{kind}>") and "tile 256x256" in plan, plan
    finally:
        assert lib.ll_set_tuning(b"gemm_variant", 0) == 0


def test_set_quant_and_cli_key_accept_fp8_rowwise_and_still_refuse_fp8():
    from longlive_amd import cli, synth
    from longlive_amd.model import CausalWanModelHIP
    m = CausalWanModelHIP(synth.toy_config(), device="cpu")
    assert m.set_quant("fp8_rowwise").quant == "fp8_rowwise"
    assert m.set_quant(None).quant is None
    for bad in ("fp8", "FP8", "fp8-rowwise"):
        with pytest.raises(ValueError):
            m.set_quant(bad)
    assert [cli.quant_mode(v) for v in ("fp8_rowwise", "FP8_ROWWISE", "int8")] == ["fp8_rowwise", "fp8_rowwise", "int8"]
    with pytest.raises(ValueError):
        cli.quant_mode("fp8")


def test_in_place_weight_update_repacks_the_fp8_weights():
    """The packed FP8 copies are keyed on every one of the six quantised weights: an in-place update of any of them (which bf16
    mode does not pack, so its key does not cover them) changes the key, and _pack re-quantises."""
    from longlive_amd import synth
    from longlive_amd.model import CausalWanModelHIP
    m = CausalWanModelHIP(synth.toy_config(), device="cpu")
    blk = m.blocks[0]
    six = [blk.self_attn.q.weight, blk.self_attn.o.weight, blk.cross_attn.q.weight, blk.cross_attn.o.weight,
           blk.ffn[0].weight, blk.ffn[2].weight]
    m.set_quant(None)
    k_bf = m._param_key()
    with torch.no_grad():
        blk.ffn[2].weight.add_(1.0)
    assert m._param_key() == k_bf                                      # bf16 mode packs no FFN weight
    m.set_quant("fp8_rowwise")
    for w in six:
        k0 = m._param_key()
        with torch.no_grad():
            w.mul_(0.5)
        assert m._param_key() != k0
    # _pack compares the key and rebuilds: simulate a stale pack and check it is dropped
    m._packed, m._packed_key = ["stale"], k0
    calls = []
    import longlive_amd.model as MD
    orig = MD.ops.quantize_rows_f8
    MD.ops.quantize_rows_f8 = lambda w: (calls.append(tuple(w.shape)) or (torch.zeros(w.shape, dtype=torch.uint8), torch.ones(w.shape[0])))
    try:
        P = m._pack()
    finally:
        MD.ops.quantize_rows_f8 = orig
    assert P != ["stale"] and len(calls) == 6 * len(m.blocks)
    assert set(P[0]) >= {"q_qkv", "s_qkv", "q_o", "s_o", "q_cq", "s_cq", "q_co", "s_co", "q_f1", "s_f1", "q_f2", "s_f2"}
