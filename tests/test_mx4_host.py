"""W4A6 mode (MXFP4 E2M1 weights over MXFP6 activations), host side: the E2M1 scheme at its edges (tests/mx4_ref.py) -- the scale
rule, every code, round-to-nearest-even ties, the packed layout -- argument validation of every new entry point before anything is
launched (the library loads without a GPU), the plan strings, the ABI version, and the switches that reach the mode."""
import os

import numpy as np
import pytest
import torch

import mx4_ref
from longlive_amd import _lib

bf = torch.bfloat16


def _block(vals):
    x = torch.zeros(1, 256, dtype=bf)
    x[0, : len(vals)] = torch.tensor(vals, dtype=torch.float64).to(bf)
    return x


def test_abi_version_and_the_new_entry_points_are_the_headers():
    header = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "longlive_hip.h")).read()
    assert f"#define LL_ABI_VERSION {_lib.ABI_VERSION}" in header and _lib.ABI_VERSION == 111
    lib = _lib.load()
    assert lib.ll_version() == 111
    for fn in ("ll_quantize_mx4", "ll_gemm_mx4w6", "ll_gemm_mx4w6_qkv", "ll_gemm_plan_mx4w6"):
        assert f"int {fn}(" in header and hasattr(lib, fn) and fn in _lib.SIGNATURES, fn


# ---- scale rule -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("e", [-20, -1, 0, 3, 40])
def test_scale_rule_at_and_just_above_6_times_a_power_of_two(e):
    at = 6.0 * 2.0 ** e
    above = float(torch.tensor(at).to(bf).view(torch.int16).add(1).view(bf).float())       # the next bf16 above 6 2^e
    assert above > at
    codes, s = mx4_ref.quantize_codes(_block([at]))
    assert int(s[0, 0]) - 127 == e and int(codes[0, 0]) == 7              # amax == 6 2^e: e itself (6 is representable)
    _, s = mx4_ref.quantize_codes(_block([above]))
    assert int(s[0, 0]) - 127 == e + 1


def test_scale_rule_at_m_0_75_and_its_bf16_neighbours():
    # amax = m 2^p: m = 0.75 is 6 2^(p-3) (e = p - 3); the next bf16 above it needs e = p - 2; one bf16 step below stays at p - 3
    p = 4
    for m, want in ((0.75, p - 3), (0.75 + 2 ** -8, p - 2), (0.75 - 2 ** -8, p - 3), (0.5, p - 3), (0.99609375, p - 2)):
        assert float(torch.tensor(m).to(bf)) == m
        amax = torch.tensor([m * 2.0 ** p])
        assert int(mx4_ref.scale_exp(amax)[0]) == want, m


def test_zero_block_bf16_subnormals_and_the_clamp():
    codes, s = mx4_ref.quantize_codes(torch.zeros(2, 256, dtype=bf))
    assert (s == 127).all() and (codes == 0).all()
    tiny = 2.0 ** -133                                                   # the smallest bf16 subnormal: e would be -135, clamped to -127
    codes, s = mx4_ref.quantize_codes(_block([tiny, -3 * tiny]))
    assert int(s[0, 0]) == 0                                             # e = -127
    assert int(codes[0, 0]) == 0 and int(codes[0, 1]) == 0x8             # 2^-6 and -3 2^-6 round to (signed) zero
    big = float(torch.tensor(3.0e38).to(bf))                             # near the bf16 maximum: never above 127
    _, s = mx4_ref.quantize_codes(_block([big]))
    assert 127 < int(s[0, 0]) <= 254
    assert int(mx4_ref.scale_exp(torch.tensor([3.0e38]))[0]) <= 127
    assert int(mx4_ref.scale_exp(torch.tensor([1e-45]))[0]) == -127


# ---- codes ------------------------------------------------------------------------------------------------------------------------
def test_all_16_codes_round_trip():
    codes = np.arange(16, dtype=np.uint8)
    vals = mx4_ref.decode(codes)
    assert list(vals[:8]) == [0, 0.5, 1, 1.5, 2, 3, 4, 6] and list(vals[8:]) == [-0.0, -0.5, -1, -1.5, -2, -3, -4, -6]
    assert np.signbit(vals[8])
    assert (mx4_ref.encode(vals) == codes).all()
    # and through the scale: a block of every value at e = 0 (amax 6) keeps every code
    x = torch.from_numpy(np.tile(vals, 16)).to(bf).view(1, 256)
    got, s = mx4_ref.quantize_codes(x)
    assert (s == 127).all() and (got[0] == np.tile(codes, 16)).all()


@pytest.mark.parametrize("v,want", [(0.25, 0.0), (0.75, 1.0), (1.25, 1.0), (1.75, 2.0), (2.5, 2.0), (3.5, 4.0), (5.0, 4.0),
                                    (-0.25, -0.0), (-5.0, -4.0)])
def test_ties_go_to_the_even_code(v, want):
    c = mx4_ref.encode(np.array([v]))
    got = mx4_ref.decode(c)[0]
    assert got == want and np.signbit(got) == np.signbit(want) and (int(c[0]) & 1) == 0


def test_restatement_agrees_with_an_independent_integer_rounding():
    """RNE on the 2^-1 grid of each binade, computed with integers, for every bf16 value in [-6, 6]."""
    h = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(bf).float().double().numpy()
    v = h[np.isfinite(h) & (np.abs(h) <= 6)]
    a = np.abs(v)
    step = np.where(a < 1, 0.5, 2.0 ** (np.floor(np.log2(np.maximum(a, 1))) - 1))
    q = a / step
    r = np.floor(q)
    frac = q - r
    r = np.where((frac > 0.5) | ((frac == 0.5) & (r % 2 == 1)), r + 1, r)
    want = np.copysign(r * step, v)
    got = mx4_ref.decode(mx4_ref.encode(v))
    assert np.array_equal(np.abs(got), np.abs(want)) and np.array_equal(np.signbit(got), np.signbit(v))


# ---- packed layout -------------------------------------------------------------------------------------------------------------------
def test_pack_and_unpack_round_trip_and_the_documented_layout():
    rng = np.random.default_rng(0)
    codes = rng.integers(0, 16, (5, 512), dtype=np.uint8)
    p = mx4_ref.pack(codes)
    assert p.shape == (5, 256) and (mx4_ref.unpack(p) == codes).all()
    # 32-k block j of a super-block at byte 32 (j % 4) + 16 (j // 4); code i of the block in bits 4i .. 4i + 3 (little-endian)
    for sb in range(2):
        for j in range(8):
            word = int.from_bytes(bytes(p[3, sb * 128 + 32 * (j % 4) + 16 * (j // 4):][:16]), "little")
            for i in range(32):
                assert (word >> (4 * i)) & 15 == codes[3, sb * 256 + 32 * j + i]
    # lane group g's fragments of both MFMA K-steps (blocks g and g + 4) are the 32 contiguous bytes at 32 g
    for g in range(4):
        frag = bytes(p[1, 32 * g: 32 * g + 32])
        lo, hi = int.from_bytes(frag[:16], "little"), int.from_bytes(frag[16:], "little")
        assert [(lo >> (4 * i)) & 15 for i in range(32)] == list(codes[1, 32 * g: 32 * g + 32])          # K-step 0: block g
        assert [(hi >> (4 * i)) & 15 for i in range(32)] == list(codes[1, 128 + 32 * g: 160 + 32 * g])   # K-step 1: block g + 4
    x = torch.randn(7, 1536).to(bf)
    q, s = mx4_ref.quantize(x)
    assert q.dtype == torch.uint8 and q.shape == (7, 768) and s.shape == (7, 48)
    d = mx4_ref.dequantize(q, s)
    blk = x.double().reshape(7, 48, 32)
    step = torch.pow(2.0, s.double() - 127).unsqueeze(-1) * 1.0        # half of the coarsest step (2 in [4, 6]) of each block
    assert ((d.reshape(7, 48, 32) - blk).abs() <= step).all()


def test_every_e2m1_value_is_an_e2m3_value():
    """The GPU tests re-encode E2M1 weights as E2M3 under the same scale bytes (ll_gemm_mx6 as an independent implementation)."""
    import mx6_ref
    vals = mx4_ref.decode(np.arange(16))
    assert np.array_equal(mx6_ref.decode(mx6_ref.encode(vals)), vals)


# ---- validation ------------------------------------------------------------------------------------------------------------------------
# every new entry point refuses bad arguments with a message, before any launch (pointer 1 = "some non-NULL pointer")
@pytest.mark.parametrize("call,needle", [
    (lambda L: L.ll_quantize_mx4(1, 1, 1, 8, 128, 128, None), "K=128 must be a positive multiple of 256"),
    (lambda L: L.ll_quantize_mx4(1, 0, 1, 8, 256, 256, None), "x, codes and scales are required"),
    (lambda L: L.ll_quantize_mx4(1, 1, 1, 8, 256, 252, None), "ldx=252"),
    (lambda L: L.ll_quantize_mx4(1, 1, 1, -1, 256, 256, None), "rows=-1"),
    (lambda L: L.ll_gemm_mx4w6(1, 1, 1, 1, 1, 1, 0, 0, 64, 256, 384, 256, 0, 0, 0, 0, 0, 0, 0, 0, None), "positive multiple of 256"),
    (lambda L: L.ll_gemm_mx4w6(1, 0, 1, 1, 1, 1, 0, 0, 64, 256, 256, 256, 0, 0, 0, 0, 0, 0, 0, 0, None), "codes and scales of both operands"),
    (lambda L: L.ll_gemm_mx4w6(1, 1, 1, 1, 0, 1, 0, 0, 64, 256, 256, 256, 0, 0, 0, 0, 0, 0, 0, 0, None), "bias is required"),
    (lambda L: L.ll_gemm_mx4w6(1, 1, 1, 1, 1, 1, 0, 0, 64, 252, 256, 256, 0, 0, 0, 0, 0, 0, 0, 0, None), "N=252"),
    (lambda L: L.ll_gemm_mx4w6(1, 1, 1, 1, 1, 1, 0, 0, 64, 256, 256, 128, 0, 0, 0, 0, 0, 0, 0, 0, None), "ldo=128"),
    (lambda L: L.ll_gemm_mx4w6(1, 1, 1, 1, 1, 1, 0, 0, -1, 256, 256, 256, 0, 0, 0, 0, 0, 0, 0, 0, None), "M=-1"),
    (lambda L: L.ll_gemm_mx4w6(1, 1, 1, 1, 1, 1, 0, 0, 64, 256, 256, 256, 7, 0, 0, 0, 0, 0, 0, 0, None), "unknown epilogue"),
    (lambda L: L.ll_gemm_mx4w6(1, 1, 1, 1, 1, 1, 0, 0, 64, 256, 256, 256, 2, 0, 0, 0, 0, 0, 0, 0, None), "needs res and e"),
    (lambda L: L.ll_gemm_mx4w6(1, 1, 1, 1, 1, 1, 0, 0, 64, 256, 256, 256, 2, 1, 1, 0, 6, 0, 64, 24, None), "do not tile"),
    (lambda L: L.ll_gemm_mx4w6(1, 1, 1, 1, 1, 1, 0, 0, 64, 256, 256, 256, 2, 1, 1, 0, 6, 6, 64, 16, None), "gate_idx 6"),
    (lambda L: L.ll_gemm_mx4w6(1, 1, 1, 1, 1, 1, 0, 0, 64, 256, 256, 256, 3, 0, 0, 0, 0, 0, 0, 0, None), "needs res"),
    (lambda L: L.ll_gemm_mx4w6(1, 1, 1, 1, 1, 1, 1, 0, 64, 256, 256, 256, 1, 0, 0, 0, 0, 0, 0, 0, None), "needs both codes and scales"),
    (lambda L: L.ll_gemm_mx4w6(1, 1, 1, 1, 1, 1, 1, 1, 64, 256, 256, 256, 1, 0, 0, 0, 0, 0, 0, 0, None), "exactly one of out"),
    (lambda L: L.ll_gemm_mx4w6(1, 1, 1, 1, 1, 0, 0, 0, 64, 256, 256, 256, 1, 0, 0, 0, 0, 0, 0, 0, None), "exactly one of out"),
    (lambda L: L.ll_gemm_mx4w6(1, 1, 1, 1, 1, 0, 1, 1, 64, 256, 256, 256, 0, 0, 0, 0, 0, 0, 0, 0, None), "GELU epilogue only"),
    (lambda L: L.ll_gemm_mx4w6(1, 1, 1, 1, 1, 0, 1, 1, 64, 384, 256, 384, 1, 0, 0, 0, 0, 0, 0, 0, None), "N=384 a multiple of 256"),
    (lambda L: L.ll_gemm_mx4w6_qkv(1, 1, 1, 1, 1, 1, 64, 768, 256, 768, 0, 1, 64, 128, 0, 0, 64, None), "cache_v is required"),
    (lambda L: L.ll_gemm_mx4w6_qkv(1, 1, 1, 1, 1, 0, 64, 768, 256, 768, 1, 1, 64, 128, 0, 0, 64, None), "out is required"),
    (lambda L: L.ll_gemm_mx4w6_qkv(1, 1, 1, 1, 1, 1, 64, 760, 256, 760, 1, 1, 64, 128, 0, 0, 64, None), "N=760 must be 3 C"),
    (lambda L: L.ll_gemm_mx4w6_qkv(1, 1, 1, 1, 1, 1, 64, 768, 256, 768, 1, 2, 64, 128, 0, 0, 64, None), "is not B=2"),
    (lambda L: L.ll_gemm_mx4w6_qkv(1, 1, 1, 1, 1, 1, 64, 768, 256, 768, 1, 1, 64, 128, 0, 10, 64, None), "write window outside"),
    (lambda L: L.ll_gemm_mx4w6_qkv(1, 1, 1, 1, 1, 1, 64, 768, 256, 768, 1, 1, 64, 128, 100, 0, 64, None), "outside cache"),
    (lambda L: L.ll_gemm_mx4w6_qkv(1, 1, 1, 1, 1, 1, 64, 768, 128, 768, 1, 1, 64, 128, 0, 0, 64, None), "positive multiple of 256"),
    (lambda L: L.ll_gemm_mx4w6_qkv(1, 1, 0, 1, 1, 1, 64, 768, 256, 768, 1, 1, 64, 128, 0, 0, 64, None),
     "codes and scales of both operands"),
    (lambda L: L.ll_gemm_plan_mx4w6(64, 256, 256, None, 0), "needs an output buffer"),
])
def test_invalid_arguments_are_rejected_before_launch(call, needle):
    lib = _lib.load()
    rc = call(lib)
    assert rc == -1, rc
    msg = lib.ll_last_error().decode()
    assert needle in msg, msg
    assert "mx4" in msg, msg


def test_plan_strings():
    from longlive_amd import ops
    assert ops.gemm_plan_mx4w6(4680, 4608, 1536) == "gemm_mx4w6_kernel tile 256x128, 256 k per stage, 684 workgroups, groups of 4 m-tiles"
    assert ops.gemm_plan_mx4w6(4680, 1536, 8960) == "gemm_mx4w6_kernel tile 256x128, 256 k per stage, 228 workgroups, groups of 4 m-tiles"
    assert ops.gemm_plan_mx4w6(9360, 8960, 1536) == "gemm_mx4w6_kernel tile 256x128, 256 k per stage, 2590 workgroups, groups of 4 m-tiles"


# ---- switches -------------------------------------------------------------------------------------------------------------------------
def test_set_quant_and_cli_key_accept_mxfp4_a6_and_still_refuse_mxfp4():
    from longlive_amd import cli, synth
    from longlive_amd.model import CausalWanModelHIP
    m = CausalWanModelHIP(synth.toy_config(), device="cpu")
    assert m.set_quant("mxfp4_a6").quant == "mxfp4_a6"
    assert m.set_quant(None).quant is None
    for bad in ("mxfp4", "fp4", "MXFP4_A6", "mxfp4a6", "w4a6"):
        with pytest.raises(ValueError):
            m.set_quant(bad)
    assert [cli.quant_mode(v) for v in ("mxfp4_a6", "MXFP4_A6", " mxfp4_a6 ")] == ["mxfp4_a6"] * 3
    for bad in ("mxfp4", "fp4", "w4a6"):
        with pytest.raises(ValueError):
            cli.quant_mode(bad)


def test_set_quant_mxfp4_a6_needs_256_wide_linears():
    from longlive_amd import synth
    from longlive_amd.model import CausalWanModelHIP
    cfg = synth.toy_config()
    cfg.dim, cfg.ffn_dim = 384, 768                       # multiples of 128, not of 256
    m = CausalWanModelHIP.__new__(CausalWanModelHIP)
    m.cfg = cfg
    with pytest.raises(ValueError, match="multiples of 256"):
        CausalWanModelHIP.set_quant(m, "mxfp4_a6")


def test_param_key_covers_the_six_packed_weights():
    """The packed E2M1 copies are keyed on every one of the six quantised weights: an in-place update of any of them changes the key,
    and _pack re-quantises all six per block with quantize_mx4 (never the MXFP6 quantiser)."""
    from longlive_amd import synth
    from longlive_amd.model import CausalWanModelHIP
    m = CausalWanModelHIP(synth.toy_config(), device="cpu")
    blk = m.blocks[0]
    six = [blk.self_attn.q.weight, blk.self_attn.o.weight, blk.cross_attn.q.weight, blk.cross_attn.o.weight,
           blk.ffn[0].weight, blk.ffn[2].weight]
    m.set_quant("mxfp4_a6")
    for w in six:
        k0 = m._param_key()
        with torch.no_grad():
            w.mul_(0.5)
        assert m._param_key() != k0
    m._packed, m._packed_key = ["stale"], k0
    calls = []
    import longlive_amd.model as MD
    orig4, orig6 = MD.ops.quantize_mx4, MD.ops.quantize_mx6
    MD.ops.quantize_mx4 = lambda w: (calls.append(tuple(w.shape)) or (torch.zeros(w.shape[0], w.shape[1] // 2, dtype=torch.uint8),
                                                                      torch.zeros(w.shape[0], w.shape[1] // 32, dtype=torch.uint8)))
    MD.ops.quantize_mx6 = lambda w: pytest.fail("weights packed as MXFP6 in mxfp4_a6 mode")
    try:
        P = m._pack()
    finally:
        MD.ops.quantize_mx4, MD.ops.quantize_mx6 = orig4, orig6
    assert P != ["stale"] and len(calls) == 6 * len(m.blocks)
    assert set(P[0]) >= {"q_qkv", "s_qkv", "q_o", "s_o", "q_cq", "s_cq", "q_co", "s_co", "q_f1", "s_f1", "q_f2", "s_f2"}
    assert P[0]["q_f1"].shape[-1] == blk.ffn[0].weight.shape[1] // 2
