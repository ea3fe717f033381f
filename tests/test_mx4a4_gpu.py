"""W4A4 block linears on the MI355X (v_mfma_scale_f32_16x16x128_f8f6f4 with E2M1 on both operands, cbsz = 4 / blgp = 4), pinned to
the scheme's definition (tests/mx4_ref.py, tests/mx4a4_ref.py): the lane map with exact data on both sides, every epilogue and the QKV
cache slots bit for bit against ll_gemm_mx4w6 on the same activations re-encoded as E2M3 under the same scale bytes (every E2M1 value
is an E2M3 value), the MXFP4 outputs of the FFN1 epilogue and the producers against ll_quantize_mx4, random data against the fp64
product of the dequantised operands (a bound ll_gemm_mx4w6 fails).  The mode at model level (its weight packs equal mxfp4_a6's, one
real-shape block against its oracle, the 30-layer steady state, config 2 free-running, the mode beside MX self-attention) is
tests/test_quant_model_gpu.py's "mxfp4_a4" row."""
import pytest
import torch

import mx4_ref
import mx6_ref
from longlive_amd import synth
from quant_exact import codes_and_scales as _codes_and_scales
from quant_exact import epi_ref as _epi_ref
from quant_exact import hard_x_mx as _hard_x
from quant_exact import within_1ulp as _within_1ulp
from util import assert_bf16_close, bf

pytestmark = pytest.mark.gpu
DEV = "cuda"
U8 = torch.uint8


@pytest.fixture(scope="module")
def ops():
    from longlive_amd import ops as O
    return O


def hn(name, shape, scale=1.0):
    return (scale * synth.hash_normal(139, name, shape)).to(bf)


def _exact(rows, K, seed, asym):
    """Small-integer values (-2 .. 2) under a distinct power-of-two scale per (row, K-block): (packed E2M1, scales, values, the same
    values as packed E2M3 under the same scale bytes).  Every fp32 sum of the GEMM is exact."""
    c, ex, v = _codes_and_scales(rows, K, seed, asym)
    q4 = torch.from_numpy(mx4_ref.pack(mx4_ref.encode(c.numpy())))
    q6 = torch.from_numpy(mx6_ref.pack(mx6_ref.encode(c.numpy())))
    return q4, (ex + 127).to(U8), v, q6


def _dev(*ts):
    return tuple(t.to(DEV) for t in ts)


def _same(a, b, what):
    assert torch.equal(a[1].cpu(), b[1].cpu()), what + " scales"
    assert torch.equal(a[0].cpu(), b[0].cpu()), what + " codes"


# ---- 1. operand map -----------------------------------------------------------------------------------------------------------
def test_gemm_mx4_lane_map_with_exact_data(ops):
    """Small integer codes, a distinct power-of-two scale per (row, K-block) on both sides, an asymmetric W, K = 512 (two stages):
    every fp32 sum is exact, so the GEMM must equal the exact product bit for bit; a wrong nibble order, block order, X swizzle or
    scale byte on either side changes it."""
    M, N, K = 300, 256, 512
    xq, sx, xv, _ = _exact(M, K, 5, False)
    wq, sw, wv, _ = _exact(N, K, 6, True)
    want = (xv @ wv.t()).to(bf)
    got = ops.gemm_mx4(_dev(xq, sx), _dev(wq, sw), torch.zeros(N, dtype=bf, device=DEV)).cpu()
    assert torch.equal(got, want), (got.float() - want.float()).abs().max()


# ---- 2. every epilogue against ll_gemm_mx4w6 with exact data ------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", [(4608, 1536), (1536, 1536), (8960, 1536), (1536, 8960)])
def test_every_epilogue_equals_mx4w6_with_exact_data(ops, N, K):
    B, F, fs = 1, 3, 1560
    M = B * F * fs
    xq, sx, xv, x6 = _exact(M, K, N + K, False)
    wq, sw, wv, _ = _exact(N, K, N - K, True)
    x4, x6, w = _dev(xq, sx), _dev(x6, sx), _dev(wq, sw)
    bias = hn(f"b{N}", (N,), 0.1)
    bd = bias.to(DEV)
    v = ops.gemm_mx4(x4, w, bd).cpu()
    assert torch.equal(v, _epi_ref(xv @ wv.t(), bias, 0)), f"bias {N}x{K}"
    assert torch.equal(v, ops.gemm_mx4w6(x6, w, bd).cpu())
    if N != 1536:
        assert torch.equal(ops.gemm_mx4(x4, w, bd, ops.EPI_BIAS_GELU).cpu(), ops.gemm_mx4w6(x6, w, bd, ops.EPI_BIAS_GELU).cpu()), "gelu"
        return
    res = hn("res", (M, N)).to(DEV)
    got = ops.gemm_mx4(x4, w, bd, ops.EPI_BIAS_RES, res=res).cpu()
    assert torch.equal(got, ops.gemm_mx4w6(x6, w, bd, ops.EPI_BIAS_RES, res=res).cpu()), f"res {K}"
    assert torch.equal(got, _epi_ref(v, torch.zeros_like(bias), 3, res.cpu())), f"res {K} host"
    e, mod = hn("e", (B, F, 6, N), 0.5).to(DEV), hn("mod", (6, N), 0.1).to(DEV)
    for md in (mod, None):
        kw = dict(res=res, e=e, mod=md, gate_idx=5, rows_per_batch=F * fs, frame_len=fs)
        got = ops.gemm_mx4(x4, w, bd, ops.EPI_BIAS_GATE_RES, **kw).cpu()
        assert torch.equal(got, ops.gemm_mx4w6(x6, w, bd, ops.EPI_BIAS_GATE_RES, **kw).cpu()), f"gate-res {K} mod={md is not None}"


# ---- 3. MXFP4-output GELU form ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [8960, 4608])
def test_gelu_mxfp4_output_is_the_quantiser_of_the_bf16_form(ops, N):
    """Random operands (every code, ties and all-zero blocks in the GELU output): the codes + scales the FFN1 form writes equal
    ll_quantize_mx4 of the bf16 GELU form's output, at M = 4680 (a partial last m-tile)."""
    M, K = 4680, 1536
    xm = ops.quantize_mx4(_hard_x(M, K, 12).to(DEV))
    wm = ops.quantize_mx4(hn(f"gw{N}", (N, K), K ** -0.5).to(DEV))
    bd = hn(f"gb{N}", (N,), 0.1).to(DEV)
    q = ops.gemm_mx4(xm, wm, bd, ops.EPI_BIAS_GELU, mx_out=True)
    assert q[0].shape == (M, N // 2) and q[1].shape == (M, N // 32)
    _same(q, ops.quantize_mx4(ops.gemm_mx4(xm, wm, bd, ops.EPI_BIAS_GELU)), f"ffn1 mx4 epilogue N={N}")


# ---- 4. batch 2, gate-residual, QKV cache slots --------------------------------------------------------------------------------------
def test_batch2_gate_residual_and_qkv_cache_slots_with_exact_data(ops):
    B, F, fs, C = 2, 3, 520, 1536
    L = F * fs
    M = B * L
    xq, sx, xv, x6 = _exact(M, C, 21, False)
    wq, sw, wv, _ = _exact(3 * C, C, 22, True)
    bias = hn("qb", (3 * C,), 0.1)
    xm, x6m, wm = (xq.view(B, L, -1).to(DEV), sx.to(DEV)), (x6.view(B, L, -1).to(DEV), sx.to(DEV)), _dev(wq, sw)
    full = ops.gemm_mx4(xm, wm, bias.to(DEV))
    assert full.shape == (B, L, 3 * C)
    assert torch.equal(full.view(M, -1).cpu(), _epi_ref(xv @ wv.t(), bias, 0)), "B=2"
    oq, osw, _, _ = _exact(C, C, 23, True)
    bo = hn("ob", (C,), 0.1).to(DEV)
    res, e = hn("ores", (M, C)).to(DEV), hn("oe", (B, F, 6, C), 0.5).to(DEV)
    kw = dict(res=res, e=e, gate_idx=2, rows_per_batch=L, frame_len=fs)
    got = ops.gemm_mx4(xm, _dev(oq, osw), bo, ops.EPI_BIAS_GATE_RES, **kw)
    assert torch.equal(got.cpu(), ops.gemm_mx4w6(x6m, _dev(oq, osw), bo, ops.EPI_BIAS_GATE_RES, **kw).cpu()), "gate-res B=2"
    S, ws, ro, wl = 4 * fs, 2 * fs, fs, 2 * fs
    cache = torch.full((B, S, 12, 128), 7.0, dtype=bf, device=DEV)
    qkv = ops.gemm_mx4_qkv_v_insert(xm, wm, bias.to(DEV), cache, ws, ro, wl, B, L)
    assert torch.equal(qkv[..., : 2 * C], full[..., : 2 * C])
    cv = cache.view(B, S, C)
    assert torch.equal(cv[:, ws: ws + wl], full[:, ro: ro + wl, 2 * C:])
    assert (cv[:, :ws] == 7).all() and (cv[:, ws + wl:] == 7).all()
    cache6 = torch.full_like(cache, 7.0)
    qkv6 = ops.gemm_mx4w6_qkv_v_insert(x6m, wm, bias.to(DEV), cache6, ws, ro, wl, B, L)
    assert torch.equal(qkv6[..., : 2 * C], qkv[..., : 2 * C]) and torch.equal(cache6, cache)


# ---- 5. producers -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 2])
def test_producers_emit_the_quantiser_bytes(ops, B):
    F, fs, C = 3, 1560, 1536
    L = F * fs
    x = _hard_x(B * L, C, 11 + B).view(B, L, C).to(DEV)
    e, mod = hn(f"pe{B}", (B, F, 6, C), 0.5).to(DEV), hn("pm", (6, C), 0.1).to(DEV)
    for md in (mod, None):
        q = ops.ln_modulate_mx4(x, e, md, 3, 4, F, 1e-6)
        assert q[0].shape == (B, L, C // 2) and q[1].shape == (B * L, C // 32)
        _same(q, ops.quantize_mx4(ops.ln_modulate(x, e, md, 3, 4, F, 1e-6)), f"ln_modulate B={B} mod={md is not None}")
    tab = ops.modulation_table_f32(e, mod.view(1, 6, C), 0b010010)[0]
    _same(ops.ln_modulate_tab_mx4(x, tab, 0, 1, F, 1e-6), ops.quantize_mx4(ops.ln_modulate_tab(x, tab, 0, 1, F, 1e-6)),
          f"ln_modulate_tab B={B}")
    w, b = hn("nw", (C,), 0.2).to(DEV), hn("nb", (C,), 0.1).to(DEV)
    _same(ops.layernorm_affine_mx4(x, w, b, 1e-6), ops.quantize_mx4(ops.layernorm_affine(x, w, b, 1e-6)), f"layernorm_affine B={B}")


# ---- 6. random data ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", [(4608, 1536), (1536, 1536), (8960, 1536), (1536, 8960)])
def test_random_data_vs_fp64_and_not_mx4w6(ops, N, K):
    """The bias form at the real shapes against the fp64 product of the dequantised operands (E2M1 x, E2M1 w) at 1 bf16 ulp; the W4A6
    GEMM on the same bf16 activations fails that bound (so E2M1 activations were used)."""
    M = 4680
    x, w, bias = hn(f"x{K}", (M, K)), hn(f"w{N}{K}", (N, K), K ** -0.5), hn(f"b{N}", (N,), 0.1)
    xd, bd = x.to(DEV), bias.to(DEV)
    xm, wm = ops.quantize_mx4(xd), ops.quantize_mx4(w.to(DEV))
    acc = mx4_ref.dequantize(*xm) @ mx4_ref.dequantize(*wm).t()
    want = (acc.float() + bias.float()).to(bf)
    assert_bf16_close(ops.gemm_mx4(xm, wm, bd), want, 1, 0.97, f"mx4 {N}x{K}")
    assert not _within_1ulp(ops.gemm_mx4w6(ops.quantize_mx6(xd), wm, bd), want), "mxfp4_a6 passes the W4A4 bound"
