"""The 16x16x32 MFMA form of the generated bf16 GEMM kernels (tuning key gemm_asm_mfma16, one bit per kernel) on the GPU: each kernel
with its own bit forced on against the same call with the bit forced off (the 32x32x16 form: same products, another order of the fp32
sum inside an MFMA), run twice, against fp64, and named by the plan; the persistent forms bit for bit against the classic ones; the
fused QKV projection with its V redirect; the projection that leaves row sums of squares for the attention kernel's Q prologue."""
import ctypes as C
import math

import pytest
import torch

from longlive_amd import synth
from util import assert_bf16_close, bf, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
BITS = {"128_bias": 1, "128_res": 2, "128_gate_res": 4, "128_bias_ssq": 8, "192_bias_p": 16, "192_bias": 32, "224_gelu_p": 64, "224_gelu": 128,
        "256_bias": 256}
ALL = 511


@pytest.fixture(scope="module")
def ops():
    from longlive_amd import ops as o
    return o


def hn(name, shape, scale=1.0, device=DEV):
    return (synth.hash_normal(77, name, shape, device=device) * scale).to(bf)


def _set(key, value):
    from longlive_amd import _lib
    _lib.check(_lib.load().ll_set_tuning(key.encode(), int(value)), "ll_set_tuning")


def _plan(ops, M, N, K, code, plain=1):
    from longlive_amd import _lib
    buf = C.create_string_buffer(320)
    _lib.check(_lib.load().ll_gemm_plan_epi(M, N, K, 0, code, plain, buf, 320), "plan")
    return buf.value.decode()


def _case(ops, M, N, K, epi, tag):
    x = hn(tag + "x", (M, K))
    w = (hn(tag + "w", (N, K)) / math.sqrt(K)).to(bf)
    b = hn(tag + "b", (N,), 0.1)
    kw = {}
    code = {"bias": ops.EPI_BIAS, "gelu": ops.EPI_BIAS_GELU, "gate": ops.EPI_BIAS_GATE_RES, "res": ops.EPI_BIAS_RES}[epi]
    if epi in ("gate", "res"):
        kw["res"] = hn(tag + "r", (M, N))
    if epi == "gate":
        F_ = next(f for f in (8, 3, 1) if M % f == 0)            # frame boundaries inside 16-row blocks (328 = 8 x 41, 321 = 3 x 107)
        kw.update(e=hn(tag + "e", (1, F_, 6, N), 0.5), mod=None, gate_idx=5, rows_per_batch=M, frame_len=M // F_)
    return x, w, b, code, kw


# (M, N, K, epilogue, kernel): 256 + 72 rows (wave 1 of the last tile has eight rows, waves 2-3 idle); 8 full tiles + 52 rows at the
# shortest K; 321 = 256 + 65 rows (one valid row in a 16-row block) at 7 K-steps (not a multiple of the 6-step unroll)
CLASSIC = [(328, 128, 256, "bias", "128_bias"), (328, 128, 256, "res", "128_res"), (328, 128, 256, "gate", "128_gate_res"),
           (2100, 3584, 256, "gelu", "224_gelu"),
           (321, 1536, 448, "bias", "128_bias"), (321, 1536, 448, "res", "128_res"), (321, 1536, 448, "gate", "128_gate_res"),
           (328, 2304, 256, "bias", "192_bias"), (321, 16384, 448, "bias", "256_bias")]


@pytest.mark.parametrize("M,N,K,epi,kernel", CLASSIC)
def test_mfma16_kernel_against_its_32_shape_form(ops, M, N, K, epi, kernel):
    x, w, b, code, kw = _case(ops, M, N, K, epi, "c")
    name = f"gemm_asm_{kernel}"
    try:
        _set("gemm_asm_mfma16", ALL ^ BITS[kernel])              # this kernel's bit alone off: its 32-shape form
        plan = _plan(ops, M, N, K, code)
        assert name + "<" in plan and "_m16" not in plan, plan
        want = ops.gemm(x, w, b, code, **kw)
        _set("gemm_asm_mfma16", BITS[kernel])                    # this kernel's bit alone on
        plan = _plan(ops, M, N, K, code)
        assert name + "_m16<" in plan, plan
        got = ops.gemm(x, w, b, code, **kw)
        again = ops.gemm(x, w, b, code, **kw)
    finally:
        _set("gemm_asm_mfma16", -1)
    assert torch.equal(got, again)
    assert_bf16_close(got, want, 2, 0.97, f"mfma16 {M}x{N}x{K} {epi}", atol=4e-2 if epi in ("gate", "res") else None)
    if epi == "bias":
        ref = (x.double() @ w.double().t() + b.double()).cpu()
        assert rel_l2(got.cpu(), ref) < 4e-3


# more tiles than CUs: 6 x 48 tiles at 224 and at 192; 17 x 16 at 128
@pytest.mark.parametrize("M,N,K,epi,kernel", [(1352, 10752, 256, "gelu", "224_gelu"), (1352, 9216, 256, "bias", "192_bias"),
                                              (4200, 2048, 256, "gate", "128_gate_res")])
def test_mfma16_persistent_form_is_the_classic_form_bit_for_bit(ops, M, N, K, epi, kernel):
    x, w, b, code, kw = _case(ops, M, N, K, epi, "p")
    wn = int(kernel.split("_")[0])
    pbit = BITS.get(kernel + "_p", BITS[kernel])                 # (the 128-wide kernels have one bit for both forms)
    try:
        _set("gemm_asm_mfma16", pbit)
        plan = _plan(ops, M, N, K, code)
        assert f"gemm_asmp_{kernel}_m16<" in plan, plan
        got = ops.gemm(x, w, b, code, **kw)
        again = ops.gemm(x, w, b, code, **kw)
        _set("gemm_asm_mfma16", ALL ^ pbit)
        plan = _plan(ops, M, N, K, code)
        assert f"gemm_asmp_{kernel}<" in plan, plan
        want32 = ops.gemm(x, w, b, code, **kw)
        _set("gemm_asm", 3)                                      # classic form of the same kernel
        _set("gemm_asm_mfma16", BITS[kernel])
        plan = _plan(ops, M, N, K, code)
        assert f"gemm_asm_{kernel}_m16<" in plan, plan
        classic = ops.gemm(x, w, b, code, **kw)
    finally:
        _set("gemm_asm", 35)
        _set("gemm_asm_mfma16", -1)
    assert ((M + 255) // 256) * (N // wn) > 256
    assert torch.equal(got, again) and torch.equal(got, classic), (got.float() - classic.float()).abs().max().item()
    assert_bf16_close(got, want32, 2, 0.97, f"mfma16 persistent {M}x{N}x{K} {epi}", atol=4e-2 if epi == "gate" else None)


@pytest.mark.parametrize("ws,ro,wl", [(100, 37, 200), (5, 250, 78), (40, 0, 9)])
def test_mfma16_qkv_v_redirect(ops, ws, ro, wl):
    """ops.gemm_qkv_v_insert on the 192-wide kernel's 16-shape form: windows that begin and end inside a 16-row block.  The unfused
    projection runs the 128-wide kernel; with both on the 16-shape every element sums its products in the same order, so the q | k
    thirds and the inserted cache rows are the unfused projection's bit for bit; everything outside the window is untouched."""
    L, Cc, K, S = 328, 384, 256, 400
    x = hn("qx", (1, L, K))
    w = (hn("qw", (3 * Cc, K)) / math.sqrt(K)).to(bf)
    b = hn("qb", (3 * Cc,), 0.1)
    cv0 = hn("qc", (1, S, 3, 128))
    try:
        _set("gemm_asm_mfma16", ALL)
        assert "gemm_asm_192_bias_m16<" in _plan(ops, L, 3 * Cc, K, ops.EPI_BIAS, 2)
        assert "gemm_asm_128_bias_m16<" in _plan(ops, L, 3 * Cc, K, ops.EPI_BIAS, 1)
        cv = cv0.clone()
        out = ops.gemm_qkv_v_insert(x, w, b, cv, ws, ro, wl)
        plain = ops.gemm(x, w, b)
        _set("gemm_asm_mfma16", 0)
        cv32 = cv0.clone()
        out32 = ops.gemm_qkv_v_insert(x, w, b, cv32, ws, ro, wl)
    finally:
        _set("gemm_asm_mfma16", -1)
    assert torch.equal(out[..., :2 * Cc], plain[..., :2 * Cc])
    assert torch.equal(cv[0, ws:ws + wl].reshape(wl, Cc), plain[0, ro:ro + wl, 2 * Cc:])
    mask = torch.ones(S, dtype=torch.bool); mask[ws:ws + wl] = False
    assert torch.equal(cv[:, mask], cv0[:, mask])
    assert_bf16_close(out[..., :2 * Cc], out32[..., :2 * Cc], 2, 0.97, "mfma16 qkv q|k")
    assert_bf16_close(cv, cv32, 2, 0.97, "mfma16 qkv cache")


def test_mfma16_row_sums_feed_the_attention_prologue(ops):
    """ops.gemm_ssq on gemm_asm_128_bias_ssq_m16 at L = 328 followed by ops.flash_attn_qnorm, against the three-launch form (gemm,
    rmsnorm, flash_attn) at the bound of test_cross_q_rmsnorm_fused_into_projection_and_attention; planes in plane order."""
    B, L, H, K, Sk = 1, 328, 3, 384, 512
    Cc = H * 128
    x, w, b = hn("fx", (B, L, K)), hn("fw", (Cc, K), 1.0 / math.sqrt(K)), hn("fb", (Cc,), 0.1)
    nw = (1.0 + 0.1 * hn("fnw", (Cc,)).float()).to(bf)
    k, v = hn("fk", (B, Sk, H, 128)), hn("fv", (B, Sk, H, 128), 0.7)
    assert ops.gemm_ssq_planes(B * L, Cc, K) == H and ops.flash_attn_qnorm_ok(H, Sk)
    try:
        _set("gemm_asm_mfma16", 0)
        q32, ssq32 = ops.gemm_ssq(x, w, b)
        _set("gemm_asm_mfma16", BITS["128_bias_ssq"] | BITS["128_bias"])
        q3 = ops.gemm(x, w, b)
        qraw, ssq = ops.gemm_ssq(x, w, b)
        qraw2, ssq2 = ops.gemm_ssq(x, w, b)
        qn = ops.rmsnorm(q3.view(B * L, Cc), nw, 1e-6).view(B, L, H, 128)
        want = ops.flash_attn(qn, k, v, [(0, Sk)])
        got = ops.flash_attn_qnorm(qraw.view(B, L, H, 128), ssq, nw, 1e-6, k, v, Sk)
    finally:
        _set("gemm_asm_mfma16", -1)
    assert torch.equal(qraw, qraw2) and torch.equal(ssq, ssq2)
    assert torch.equal(qraw, q3), "the SSQ epilogue must not change the projection's output"
    assert_bf16_close(qraw, q32, 2, 0.97, "mfma16 ssq projection")
    ref_ss = (q3.float().view(B * L, H, 128) ** 2).sum(-1).t()                     # [H, B*L]
    assert ssq.shape == ref_ss.shape and torch.allclose(ssq, ref_ss, rtol=2e-6, atol=0), (ssq - ref_ss).abs().max().item()
    assert torch.allclose(ssq, ssq32, rtol=2e-2)      # every output at most 2 bf16 ulp (2^-7 relative) from the 32-shape's: squares within 2^-6
    assert torch.isfinite(got.float()).all()
    assert (got.float() - want.float()).abs().max().item() < 4e-3, (got.float() - want.float()).abs().max().item()
    assert rel_l2(got.cpu(), want.cpu()) < 2e-3
