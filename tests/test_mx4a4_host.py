"""W4A4 mode (MXFP4 E2M1 weights and activations), host side: the new entry points in the header and the bindings under the unchanged
ABI version, argument validation of every new entry point before anything is launched (the library loads without a GPU), the plan
strings and the switches that reach the mode.  (The restatement's activation path is pinned in tests/test_quant_ref_host.py.)"""
import os

import pytest
import torch

from longlive_amd import _lib

bf = torch.bfloat16
NEW = ("ll_gemm_mx4", "ll_gemm_mx4_qkv", "ll_ln_modulate_mx4", "ll_ln_modulate_tab_mx4", "ll_layernorm_affine_mx4", "ll_gemm_plan_mx4")


def test_new_entry_points_are_declared_bound_and_keep_abi_111():
    header = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "longlive_hip.h")).read()
    assert "#define LL_ABI_VERSION 111" in header and _lib.ABI_VERSION == 111
    lib = _lib.load()
    assert lib.ll_version() == 111
    for fn in NEW:
        assert f"int {fn}(" in header and hasattr(lib, fn) and fn in _lib.SIGNATURES, fn


# ---- validation ------------------------------------------------------------------------------------------------------------------------
# every new entry point refuses bad arguments with a message, before any launch (pointer 1 = "some non-NULL pointer")
@pytest.mark.parametrize("call,needle", [
    (lambda L: L.ll_gemm_mx4(1, 1, 1, 1, 1, 1, 0, 0, 64, 256, 384, 256, 0, 0, 0, 0, 0, 0, 0, 0, None), "positive multiple of 256"),
    (lambda L: L.ll_gemm_mx4(1, 0, 1, 1, 1, 1, 0, 0, 64, 256, 256, 256, 0, 0, 0, 0, 0, 0, 0, 0, None), "codes and scales of both operands"),
    (lambda L: L.ll_gemm_mx4(0, 1, 1, 1, 1, 1, 0, 0, 64, 256, 256, 256, 0, 0, 0, 0, 0, 0, 0, 0, None), "codes and scales of both operands"),
    (lambda L: L.ll_gemm_mx4(1, 1, 1, 1, 0, 1, 0, 0, 64, 256, 256, 256, 0, 0, 0, 0, 0, 0, 0, 0, None), "bias is required"),
    (lambda L: L.ll_gemm_mx4(1, 1, 1, 1, 1, 1, 0, 0, 64, 252, 256, 256, 0, 0, 0, 0, 0, 0, 0, 0, None), "N=252"),
    (lambda L: L.ll_gemm_mx4(1, 1, 1, 1, 1, 1, 0, 0, 64, 256, 256, 128, 0, 0, 0, 0, 0, 0, 0, 0, None), "ldo=128"),
    (lambda L: L.ll_gemm_mx4(1, 1, 1, 1, 1, 1, 0, 0, -1, 256, 256, 256, 0, 0, 0, 0, 0, 0, 0, 0, None), "M=-1"),
    (lambda L: L.ll_gemm_mx4(1, 1, 1, 1, 1, 1, 0, 0, 64, 256, 256, 256, 7, 0, 0, 0, 0, 0, 0, 0, None), "unknown epilogue"),
    (lambda L: L.ll_gemm_mx4(1, 1, 1, 1, 1, 1, 0, 0, 64, 256, 256, 256, 2, 0, 0, 0, 0, 0, 0, 0, None), "needs res and e"),
    (lambda L: L.ll_gemm_mx4(1, 1, 1, 1, 1, 1, 0, 0, 64, 256, 256, 256, 2, 1, 1, 0, 6, 0, 64, 24, None), "do not tile"),
    (lambda L: L.ll_gemm_mx4(1, 1, 1, 1, 1, 1, 0, 0, 64, 256, 256, 256, 2, 1, 1, 0, 6, 6, 64, 16, None), "gate_idx 6"),
    (lambda L: L.ll_gemm_mx4(1, 1, 1, 1, 1, 1, 0, 0, 64, 256, 256, 256, 3, 0, 0, 0, 0, 0, 0, 0, None), "needs res"),
    (lambda L: L.ll_gemm_mx4(1, 1, 1, 1, 1, 1, 1, 0, 64, 256, 256, 256, 1, 0, 0, 0, 0, 0, 0, 0, None), "needs both codes and scales"),
    (lambda L: L.ll_gemm_mx4(1, 1, 1, 1, 1, 1, 1, 1, 64, 256, 256, 256, 1, 0, 0, 0, 0, 0, 0, 0, None), "exactly one of out"),
    (lambda L: L.ll_gemm_mx4(1, 1, 1, 1, 1, 0, 0, 0, 64, 256, 256, 256, 1, 0, 0, 0, 0, 0, 0, 0, None), "exactly one of out"),
    (lambda L: L.ll_gemm_mx4(1, 1, 1, 1, 1, 0, 1, 1, 64, 256, 256, 256, 0, 0, 0, 0, 0, 0, 0, 0, None), "GELU epilogue only"),
    (lambda L: L.ll_gemm_mx4(1, 1, 1, 1, 1, 0, 1, 1, 64, 384, 256, 384, 1, 0, 0, 0, 0, 0, 0, 0, None), "N=384 a multiple of 256"),
    (lambda L: L.ll_gemm_mx4_qkv(1, 1, 1, 1, 1, 1, 64, 768, 256, 768, 0, 1, 64, 128, 0, 0, 64, None), "cache_v is required"),
    (lambda L: L.ll_gemm_mx4_qkv(1, 1, 1, 1, 1, 0, 64, 768, 256, 768, 1, 1, 64, 128, 0, 0, 64, None), "out is required"),
    (lambda L: L.ll_gemm_mx4_qkv(1, 1, 1, 1, 1, 1, 64, 760, 256, 760, 1, 1, 64, 128, 0, 0, 64, None), "N=760 must be 3 C"),
    (lambda L: L.ll_gemm_mx4_qkv(1, 1, 1, 1, 1, 1, 64, 768, 256, 768, 1, 2, 64, 128, 0, 0, 64, None), "is not B=2"),
    (lambda L: L.ll_gemm_mx4_qkv(1, 1, 1, 1, 1, 1, 64, 768, 256, 768, 1, 1, 64, 128, 0, 10, 64, None), "write window outside"),
    (lambda L: L.ll_gemm_mx4_qkv(1, 1, 1, 1, 1, 1, 64, 768, 256, 768, 1, 1, 64, 128, 100, 0, 64, None), "outside cache"),
    (lambda L: L.ll_gemm_mx4_qkv(1, 1, 1, 1, 1, 1, 64, 768, 128, 768, 1, 1, 64, 128, 0, 0, 64, None), "positive multiple of 256"),
    (lambda L: L.ll_gemm_mx4_qkv(1, 1, 0, 1, 1, 1, 64, 768, 256, 768, 1, 1, 64, 128, 0, 0, 64, None),
     "codes and scales of both operands"),
    (lambda L: L.ll_ln_modulate_mx4(1, 1, 1, 1, 0, 6, 0, 1, 1, 3, 1200, 3, 1e-6, None), "C=1200 must be a multiple of 256"),
    (lambda L: L.ll_ln_modulate_mx4(1, 0, 1, 1, 0, 6, 0, 1, 1, 3, 1536, 3, 1e-6, None), "codes and scales are required"),
    (lambda L: L.ll_ln_modulate_mx4(0, 1, 1, 1, 0, 6, 0, 1, 1, 3, 1536, 3, 1e-6, None), "x and e are required"),
    (lambda L: L.ll_ln_modulate_mx4(1, 1, 1, 1, 0, 6, 0, 1, 1, 4, 1536, 3, 1e-6, None), "L=4 not divisible by F=3"),
    (lambda L: L.ll_ln_modulate_mx4(1, 1, 1, 1, 0, 6, 0, 6, 1, 3, 1536, 3, 1e-6, None), "bad mod index"),
    (lambda L: L.ll_ln_modulate_tab_mx4(1, 1, 1, 1, 6, 0, 1, 1, 3, 2304, 3, 1e-6, None), "C=2304"),
    (lambda L: L.ll_ln_modulate_tab_mx4(1, 1, 0, 1, 6, 0, 1, 1, 3, 1536, 3, 1e-6, None), "codes and scales are required"),
    (lambda L: L.ll_ln_modulate_tab_mx4(1, 1, 1, 0, 6, 0, 1, 1, 3, 1536, 3, 1e-6, None), "x and tab are required"),
    (lambda L: L.ll_ln_modulate_tab_mx4(1, 1, 1, 1, 6, 0, 1, 1, 3, 1536, 0, 1e-6, None), "not divisible by F=0"),
    (lambda L: L.ll_ln_modulate_tab_mx4(1, 1, 1, 1, 6, -1, 1, 1, 3, 1536, 3, 1e-6, None), "bad mod index"),
    (lambda L: L.ll_layernorm_affine_mx4(1, 1, 1, 1, 1, 8, 1000, 1e-6, None), "C=1000"),
    (lambda L: L.ll_layernorm_affine_mx4(1, 0, 1, 1, 1, 8, 1536, 1e-6, None), "x, w and b are required"),
    (lambda L: L.ll_layernorm_affine_mx4(1, 1, 1, 1, 0, 8, 1536, 1e-6, None), "codes and scales are required"),
    (lambda L: L.ll_gemm_plan_mx4(64, 256, 256, None, 0), "needs an output buffer"),
])
def test_invalid_arguments_are_rejected_before_launch(call, needle):
    lib = _lib.load()
    rc = call(lib)
    assert rc == -1, rc
    msg = lib.ll_last_error().decode()
    assert needle in msg, msg
    assert "mx4" in msg and "mx4w6" not in msg, msg


def test_plan_strings():
    from longlive_amd import ops
    assert ops.gemm_plan_mx4(4680, 4608, 1536) == "gemm_mx4_kernel tile 256x128, 256 k per stage, 684 workgroups, groups of 4 m-tiles"
    assert ops.gemm_plan_mx4(4680, 1536, 8960) == "gemm_mx4_kernel tile 256x128, 256 k per stage, 228 workgroups, groups of 4 m-tiles"
    assert ops.gemm_plan_mx4(9360, 8960, 1536) == "gemm_mx4_kernel tile 256x128, 256 k per stage, 2590 workgroups, groups of 4 m-tiles"
    assert ops.gemm_plan_mx4(1, 128, 256) == "gemm_mx4_kernel tile 256x128, 256 k per stage, 1 workgroups, groups of 4 m-tiles"


# ---- switches -------------------------------------------------------------------------------------------------------------------------
def test_set_quant_and_cli_key_accept_mxfp4_a4_and_still_refuse_mxfp4():
    from longlive_amd import cli, synth
    from longlive_amd.model import CausalWanModelHIP
    m = CausalWanModelHIP(synth.toy_config(), device="cpu")
    assert m.set_quant("mxfp4_a4").quant == "mxfp4_a4"
    assert m.set_quant(None).quant is None
    for bad in ("mxfp4", "fp4", "w4a4", "mxfp4a4", "mxfp4_a"):
        with pytest.raises(ValueError):
            m.set_quant(bad)
    assert [cli.quant_mode(v) for v in ("mxfp4_a4", "MXFP4_A4", " mxfp4_a4 ", "\tMxFp4_A4\n")] == ["mxfp4_a4"] * 4
    assert "mxfp4_a4" in cli.QUANT_MODES
    for bad in ("mxfp4", "fp4", "w4a4", "mxfp4a4"):
        with pytest.raises(ValueError):
            cli.quant_mode(bad)


def test_set_quant_mxfp4_a4_needs_256_wide_linears():
    from longlive_amd import synth
    from longlive_amd.model import CausalWanModelHIP
    cfg = synth.toy_config()
    cfg.dim, cfg.ffn_dim = 384, 768                       # multiples of 128, not of 256
    m = CausalWanModelHIP.__new__(CausalWanModelHIP)
    m.cfg = cfg
    with pytest.raises(ValueError, match="multiples of 256"):
        CausalWanModelHIP.set_quant(m, "mxfp4_a4")


def test_weight_packs_use_the_mxfp4_quantiser():
    """mxfp4_a4 keys its packs on the six quantised weights and packs them with quantize_mx4 (the W4A6 mode's weight packs)."""
    from longlive_amd import synth
    from longlive_amd.model import CausalWanModelHIP
    m = CausalWanModelHIP(synth.toy_config(), device="cpu")
    blk = m.blocks[0]
    m.set_quant("mxfp4_a4")
    k0 = m._param_key()
    with torch.no_grad():
        blk.ffn[2].weight.mul_(0.5)
    assert m._param_key() != k0
    calls = []
    import longlive_amd.model as MD
    orig4, orig6 = MD.ops.quantize_mx4, MD.ops.quantize_mx6
    MD.ops.quantize_mx4 = lambda w: (calls.append(tuple(w.shape)) or (torch.zeros(w.shape[0], w.shape[1] // 2, dtype=torch.uint8),
                                                                      torch.zeros(w.shape[0], w.shape[1] // 32, dtype=torch.uint8)))
    MD.ops.quantize_mx6 = lambda w: pytest.fail("weights packed as MXFP6 in mxfp4_a4 mode")
    try:
        P = m._pack()
    finally:
        MD.ops.quantize_mx4, MD.ops.quantize_mx6 = orig4, orig6
    assert len(calls) == 6 * len(m.blocks)
    assert P[0]["q_f2"].shape[-1] == blk.ffn[2].weight.shape[1] // 2
