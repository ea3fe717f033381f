"""MXFP6 mode, host side: the scheme at its edges (tests/mx6_ref.py) -- the scale rule, every code, round-to-nearest-even ties, the
packed layout -- argument validation of every new entry point before anything is launched (the library loads without a GPU), the
plan strings, and the switches that reach the mode."""
import numpy as np
import pytest
import torch

import mx6_ref
from longlive_amd import _lib

bf = torch.bfloat16


@pytest.fixture(autouse=True)
def _scheme_is_the_librarys():
    """tests/mx6_ref.py restates ll_quantize_mx6 / ll_gemm_mx6: its edges are pinned only where the library declares them."""
    import os
    header = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "longlive_hip.h")).read()
    assert "int ll_quantize_mx6(" in header and hasattr(_lib.load(), "ll_quantize_mx6")


def _block(vals):
    x = torch.zeros(1, 256, dtype=bf)
    x[0, : len(vals)] = torch.tensor(vals, dtype=torch.float64).to(bf)
    return x


# ---- scale rule -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("e", [-20, -1, 0, 3, 40])
def test_scale_rule_at_and_just_above_7_5_times_a_power_of_two(e):
    at = 7.5 * 2.0 ** e
    above = float(torch.tensor(at).to(bf).view(torch.int16).add(1).view(bf).float())       # the next bf16 above 7.5 2^e
    assert above > at
    _, s = mx6_ref.quantize_codes(_block([at]))
    assert int(s[0, 0]) - 127 == e                                      # amax == 7.5 2^e: e itself (7.5 is representable)
    _, s = mx6_ref.quantize_codes(_block([above]))
    assert int(s[0, 0]) - 127 == e + 1


def test_scale_rule_at_m_0_9375_and_its_neighbours():
    # amax = m 2^p: m = 0.9375 is 7.5 2^(p-3) (e = p - 3); the next bf16 above it needs e = p - 2; 0.9375 - one bf16 step stays at p - 3
    p = 4
    for m, want in ((0.9375, p - 3), (0.9375 + 2 ** -8, p - 2), (0.9375 - 2 ** -8, p - 3), (0.5, p - 3)):
        amax = torch.tensor([m * 2.0 ** p])
        assert int(mx6_ref.scale_exp(amax)[0]) == want, m


def test_zero_block_bf16_subnormals_and_the_clamp():
    codes, s = mx6_ref.quantize_codes(torch.zeros(2, 256, dtype=bf))
    assert (s == 127).all() and (codes == 0).all()
    tiny = 2.0 ** -133                                                   # the smallest bf16 subnormal: e would be -136, clamped to -127
    codes, s = mx6_ref.quantize_codes(_block([tiny, -3 * tiny]))
    assert int(s[0, 0]) == 0                                             # e = -127
    assert int(codes[0, 0]) == 0 and int(codes[0, 1]) == 0x20           # 2^-6 and -3 2^-6 round to (signed) zero
    big = float(torch.tensor(3.0e38).to(bf))                             # near the bf16 maximum: e = 126 + ..., never above 127
    _, s = mx6_ref.quantize_codes(_block([big]))
    assert 127 < int(s[0, 0]) <= 254
    assert int(mx6_ref.scale_exp(torch.tensor([3.0e38]))[0]) <= 127
    assert int(mx6_ref.scale_exp(torch.tensor([1e-45]))[0]) == -127


# ---- codes ------------------------------------------------------------------------------------------------------------------------
def test_all_64_codes_round_trip():
    codes = np.arange(64, dtype=np.uint8)
    vals = mx6_ref.decode(codes)
    assert vals[31] == 7.5 and vals[1] == 0.125 and vals[8] == 1.0 and vals[16] == 2.0 and vals[24] == 4.0
    back = mx6_ref.encode(vals)
    assert (back == codes).all()
    # and through the scale: a block of every magnitude at e = 0 (amax 7.5) keeps every code
    x = torch.from_numpy(np.concatenate([vals[:32], vals[32:]] * 4)).to(bf).view(1, 256)
    got, s = mx6_ref.quantize_codes(x)
    assert (s == 127).all() and (got[0] == np.tile(codes, 4)).all()


@pytest.mark.parametrize("v,want", [(7.25, 7.0), (0.0625, 0.0), (0.1875, 0.25), (1.0625, 1.0), (1.1875, 1.25), (1.9375, 2.0),
                                    (3.875, 4.0), (0.9375, 1.0), (5.25, 5.0), (5.75, 6.0), (-7.25, -7.0)])
def test_ties_go_to_the_even_code(v, want):
    c = mx6_ref.encode(np.array([v]))
    assert mx6_ref.decode(c)[0] == want and (int(c[0]) & 1) == 0


def test_restatement_agrees_with_an_independent_integer_rounding():
    """RNE on the 2^-3 grid of each binade, computed with integers, for every bf16 value in [-7.5, 7.5]."""
    h = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(bf).float().double().numpy()
    v = h[np.isfinite(h) & (np.abs(h) <= 7.5)]
    a = np.abs(v)
    step = np.where(a < 1, 0.125, 2.0 ** (np.floor(np.log2(np.maximum(a, 1))) - 3))
    q = a / step
    r = np.floor(q)
    frac = q - r
    r = np.where((frac > 0.5) | ((frac == 0.5) & (r % 2 == 1)), r + 1, r)
    want = np.copysign(r * step, v)
    got = mx6_ref.decode(mx6_ref.encode(v))
    assert np.array_equal(np.abs(got), np.abs(want)) and np.array_equal(np.signbit(got), np.signbit(v))


# ---- packed layout -------------------------------------------------------------------------------------------------------------------
def test_pack_and_unpack_round_trip_and_the_documented_layout():
    rng = np.random.default_rng(0)
    codes = rng.integers(0, 64, (5, 512), dtype=np.uint8)
    p = mx6_ref.pack(codes)
    assert p.shape == (5, 384) and (mx6_ref.unpack(p) == codes).all()
    # 32-k block j of a super-block at byte 48 (j % 4) + 24 (j // 4); code i of the block in bits 6i .. 6i + 5 (little-endian)
    for sb in range(2):
        for j in range(8):
            word = int.from_bytes(bytes(p[3, sb * 192 + 48 * (j % 4) + 24 * (j // 4):][:24]), "little")
            for i in range(32):
                assert (word >> (6 * i)) & 63 == codes[3, sb * 256 + 32 * j + i]
    x = torch.randn(7, 1536).to(bf)
    q, s = mx6_ref.quantize(x)
    assert q.dtype == torch.uint8 and q.shape == (7, 1152) and s.shape == (7, 48)
    d = mx6_ref.dequantize(q, s)
    blk = x.double().reshape(7, 48, 32)
    step = torch.pow(2.0, s.double() - 127).unsqueeze(-1) * 0.25       # half of the coarsest step (0.5 in [4, 7.5]) of each block
    assert ((d.reshape(7, 48, 32) - blk).abs() <= step).all()


# ---- validation ------------------------------------------------------------------------------------------------------------------------
# every new entry point refuses bad arguments with a message, before any launch (pointer 1 = "some non-NULL pointer")
@pytest.mark.parametrize("call,needle", [
    (lambda L: L.ll_quantize_mx6(1, 1, 1, 8, 128, 128, None), "K=128 must be a positive multiple of 256"),
    (lambda L: L.ll_quantize_mx6(1, 0, 1, 8, 256, 256, None), "x, codes and scales are required"),
    (lambda L: L.ll_quantize_mx6(1, 1, 1, 8, 256, 252, None), "ldx=252"),
    (lambda L: L.ll_quantize_mx6(1, 1, 1, -1, 256, 256, None), "rows=-1"),
    (lambda L: L.ll_gemm_mx6(1, 1, 1, 1, 1, 1, 0, 0, 64, 256, 384, 256, 0, 0, 0, 0, 0, 0, 0, 0, None), "positive multiple of 256"),
    (lambda L: L.ll_gemm_mx6(1, 0, 1, 1, 1, 1, 0, 0, 64, 256, 256, 256, 0, 0, 0, 0, 0, 0, 0, 0, None), "codes and scales of both operands"),
    (lambda L: L.ll_gemm_mx6(1, 1, 1, 1, 0, 1, 0, 0, 64, 256, 256, 256, 0, 0, 0, 0, 0, 0, 0, 0, None), "bias is required"),
    (lambda L: L.ll_gemm_mx6(1, 1, 1, 1, 1, 1, 0, 0, 64, 252, 256, 256, 0, 0, 0, 0, 0, 0, 0, 0, None), "N=252"),
    (lambda L: L.ll_gemm_mx6(1, 1, 1, 1, 1, 1, 0, 0, 64, 256, 256, 128, 0, 0, 0, 0, 0, 0, 0, 0, None), "ldo=128"),
    (lambda L: L.ll_gemm_mx6(1, 1, 1, 1, 1, 1, 0, 0, -1, 256, 256, 256, 0, 0, 0, 0, 0, 0, 0, 0, None), "M=-1"),
    (lambda L: L.ll_gemm_mx6(1, 1, 1, 1, 1, 1, 0, 0, 64, 256, 256, 256, 7, 0, 0, 0, 0, 0, 0, 0, None), "unknown epilogue"),
    (lambda L: L.ll_gemm_mx6(1, 1, 1, 1, 1, 1, 0, 0, 64, 256, 256, 256, 2, 0, 0, 0, 0, 0, 0, 0, None), "needs res and e"),
    (lambda L: L.ll_gemm_mx6(1, 1, 1, 1, 1, 1, 0, 0, 64, 256, 256, 256, 2, 1, 1, 0, 6, 0, 64, 24, None), "do not tile"),
    (lambda L: L.ll_gemm_mx6(1, 1, 1, 1, 1, 1, 0, 0, 64, 256, 256, 256, 2, 1, 1, 0, 6, 6, 64, 16, None), "gate_idx 6"),
    (lambda L: L.ll_gemm_mx6(1, 1, 1, 1, 1, 1, 0, 0, 64, 256, 256, 256, 3, 0, 0, 0, 0, 0, 0, 0, None), "needs res"),
    (lambda L: L.ll_gemm_mx6(1, 1, 1, 1, 1, 1, 1, 0, 64, 256, 256, 256, 1, 0, 0, 0, 0, 0, 0, 0, None), "needs both codes and scales"),
    (lambda L: L.ll_gemm_mx6(1, 1, 1, 1, 1, 1, 1, 1, 64, 256, 256, 256, 1, 0, 0, 0, 0, 0, 0, 0, None), "exactly one of out"),
    (lambda L: L.ll_gemm_mx6(1, 1, 1, 1, 1, 0, 0, 0, 64, 256, 256, 256, 1, 0, 0, 0, 0, 0, 0, 0, None), "exactly one of out"),
    (lambda L: L.ll_gemm_mx6(1, 1, 1, 1, 1, 0, 1, 1, 64, 256, 256, 256, 0, 0, 0, 0, 0, 0, 0, 0, None), "GELU epilogue only"),
    (lambda L: L.ll_gemm_mx6(1, 1, 1, 1, 1, 0, 1, 1, 64, 384, 256, 384, 1, 0, 0, 0, 0, 0, 0, 0, None), "N=384 a multiple of 256"),
    (lambda L: L.ll_gemm_mx6_qkv(1, 1, 1, 1, 1, 1, 64, 768, 256, 768, 0, 1, 64, 128, 0, 0, 64, None), "cache_v is required"),
    (lambda L: L.ll_gemm_mx6_qkv(1, 1, 1, 1, 1, 0, 64, 768, 256, 768, 1, 1, 64, 128, 0, 0, 64, None), "out is required"),
    (lambda L: L.ll_gemm_mx6_qkv(1, 1, 1, 1, 1, 1, 64, 760, 256, 760, 1, 1, 64, 128, 0, 0, 64, None), "N=760 must be 3 C"),
    (lambda L: L.ll_gemm_mx6_qkv(1, 1, 1, 1, 1, 1, 64, 768, 256, 768, 1, 2, 64, 128, 0, 0, 64, None), "is not B=2"),
    (lambda L: L.ll_gemm_mx6_qkv(1, 1, 1, 1, 1, 1, 64, 768, 256, 768, 1, 1, 64, 128, 0, 10, 64, None), "write window outside"),
    (lambda L: L.ll_gemm_mx6_qkv(1, 1, 1, 1, 1, 1, 64, 768, 256, 768, 1, 1, 64, 128, 100, 0, 64, None), "outside cache"),
    (lambda L: L.ll_gemm_mx6_qkv(1, 1, 1, 1, 1, 1, 64, 768, 128, 768, 1, 1, 64, 128, 0, 0, 64, None), "positive multiple of 256"),
    (lambda L: L.ll_gemm_mx6_qkv(1, 1, 0, 1, 1, 1, 64, 768, 256, 768, 1, 1, 64, 128, 0, 0, 64, None), "codes and scales of both operands"),
    (lambda L: L.ll_ln_modulate_mx6(1, 1, 1, 1, 0, 6, 0, 1, 1, 9, 160, 3, 1e-6, None), "C=160 must be a multiple of 256"),
    (lambda L: L.ll_ln_modulate_mx6(1, 0, 1, 1, 0, 6, 0, 1, 1, 9, 256, 3, 1e-6, None), "codes and scales are required"),
    (lambda L: L.ll_ln_modulate_mx6(0, 1, 1, 1, 0, 6, 0, 1, 1, 9, 256, 3, 1e-6, None), "x and e are required"),
    (lambda L: L.ll_ln_modulate_mx6(1, 1, 1, 1, 0, 6, 0, 7, 1, 9, 256, 3, 1e-6, None), "bad mod index"),
    (lambda L: L.ll_ln_modulate_mx6(1, 1, 1, 1, 0, 6, 0, 1, 1, 10, 256, 3, 1e-6, None), "not divisible"),
    (lambda L: L.ll_ln_modulate_tab_mx6(1, 1, 1, 0, 6, 0, 1, 1, 9, 256, 3, 1e-6, None), "x and tab are required"),
    (lambda L: L.ll_ln_modulate_tab_mx6(1, 1, 0, 1, 6, 0, 1, 1, 9, 256, 3, 1e-6, None), "codes and scales are required"),
    (lambda L: L.ll_ln_modulate_tab_mx6(1, 1, 1, 1, 6, 9, 1, 1, 9, 256, 3, 1e-6, None), "bad mod index"),
    (lambda L: L.ll_ln_modulate_tab_mx6(1, 1, 1, 1, 6, 0, 1, 1, 10, 256, 3, 1e-6, None), "not divisible"),
    (lambda L: L.ll_ln_modulate_tab_mx6(1, 1, 1, 1, 6, 0, 1, 1, 9, 2304, 3, 1e-6, None), "<= 2048"),
    (lambda L: L.ll_layernorm_affine_mx6(1, 1, 1, 1, 1, 9, 2304, 1e-6, None), "<= 2048"),
    (lambda L: L.ll_layernorm_affine_mx6(1, 0, 1, 1, 1, 9, 256, 1e-6, None), "x, w and b are required"),
    (lambda L: L.ll_layernorm_affine_mx6(1, 1, 1, 0, 1, 9, 256, 1e-6, None), "codes and scales are required"),
    (lambda L: L.ll_gemm_plan_mx6(64, 256, 256, None, 0), "needs an output buffer"),
])
def test_invalid_arguments_are_rejected_before_launch(call, needle):
    lib = _lib.load()
    rc = call(lib)
    assert rc == -1, rc
    msg = lib.ll_last_error().decode()
    assert needle in msg, msg


def test_plan_strings():
    from longlive_amd import ops
    assert ops.gemm_plan_mx6(4680, 4608, 1536) == "gemm_mx6_kernel tile 256x128, 256 k per stage, 684 workgroups, groups of 4 m-tiles"
    assert ops.gemm_plan_mx6(4680, 1536, 8960) == "gemm_mx6_kernel tile 256x128, 256 k per stage, 228 workgroups, groups of 4 m-tiles"
    assert ops.gemm_plan_mx6(9360, 8960, 1536) == "gemm_mx6_kernel tile 256x128, 256 k per stage, 2590 workgroups, groups of 4 m-tiles"


# ---- switches -------------------------------------------------------------------------------------------------------------------------
def test_set_quant_and_cli_key_accept_mxfp6_and_refuse_the_other_fp6_fp4_names():
    from longlive_amd import cli, synth
    from longlive_amd.model import CausalWanModelHIP
    m = CausalWanModelHIP(synth.toy_config(), device="cpu")
    assert m.set_quant("mxfp6").quant == "mxfp6"
    assert m.set_quant(None).quant is None
    for bad in ("fp6", "mxfp4", "mxfp6_e3m2", "MXFP6", "mx6"):
        with pytest.raises(ValueError):
            m.set_quant(bad)
    assert [cli.quant_mode(v) for v in ("mxfp6", "MXFP6", " mxfp6 ")] == ["mxfp6"] * 3
    for bad in ("fp6", "mxfp4", "mxfp6_e3m2"):
        with pytest.raises(ValueError):
            cli.quant_mode(bad)


def test_set_quant_mxfp6_needs_256_wide_linears():
    from longlive_amd import synth
    from longlive_amd.model import CausalWanModelHIP
    cfg = synth.toy_config()
    cfg.dim, cfg.ffn_dim = 384, 768                       # multiples of 128, not of 256
    m = CausalWanModelHIP.__new__(CausalWanModelHIP)
    m.cfg = cfg
    with pytest.raises(ValueError, match="multiples of 256"):
        CausalWanModelHIP.set_quant(m, "mxfp6")


def test_param_key_covers_the_six_packed_weights():
    """The packed MXFP6 copies are keyed on every one of the six quantised weights: an in-place update of any of them changes the key,
    and _pack re-quantises all six per block."""
    from longlive_amd import synth
    from longlive_amd.model import CausalWanModelHIP
    m = CausalWanModelHIP(synth.toy_config(), device="cpu")
    blk = m.blocks[0]
    six = [blk.self_attn.q.weight, blk.self_attn.o.weight, blk.cross_attn.q.weight, blk.cross_attn.o.weight,
           blk.ffn[0].weight, blk.ffn[2].weight]
    m.set_quant("mxfp6")
    for w in six:
        k0 = m._param_key()
        with torch.no_grad():
            w.mul_(0.5)
        assert m._param_key() != k0
    m._packed, m._packed_key = ["stale"], k0
    calls = []
    import longlive_amd.model as MD
    orig = MD.ops.quantize_mx6
    MD.ops.quantize_mx6 = lambda w: (calls.append(tuple(w.shape)) or (torch.zeros(w.shape[0], w.shape[1] // 4 * 3, dtype=torch.uint8),
                                                                      torch.zeros(w.shape[0], w.shape[1] // 32, dtype=torch.uint8)))
    try:
        P = m._pack()
    finally:
        MD.ops.quantize_mx6 = orig
    assert P != ["stale"] and len(calls) == 6 * len(m.blocks)
    assert set(P[0]) >= {"q_qkv", "s_qkv", "q_o", "s_o", "q_cq", "s_cq", "q_co", "s_co", "q_f1", "s_f1", "q_f2", "s_f2"}
