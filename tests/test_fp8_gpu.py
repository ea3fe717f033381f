"""FP8 rowwise block linears on the MI355X (e4m3fn codes, per-token / per-output-channel fp32 scales, v_mfma_scale_f32_16x16x128_f8f6f4
at unit block scales on the W8A8 kernels' structure), pinned to the scheme's definition (tests/fp8_ref.py): quantiser and producer
bytes, every epilogue and kernel instance with exact data, random data against the fp64 product (a bound the int8 and bf16 GEMMs
fail), outliers against int8.  The mode at model level (one real-shape block against its oracle, the 30-layer steady state, config 2
free-running, the mode beside MX self-attention) is tests/test_quant_model_gpu.py's "fp8_rowwise" row."""
import pytest
import torch

import fp8_ref
from longlive_amd import synth
from quant_exact import epi_tail as _epi_ref
from quant_exact import exact_operands as _exact_operands
from quant_exact import hard_x_f8 as _hard_x
from quant_exact import within_1ulp as _within_1ulp
from util import assert_bf16_close, bf, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
U8 = torch.uint8


@pytest.fixture(scope="module")
def ops():
    from longlive_amd import ops as O
    return O


def hn(name, shape, scale=1.0):
    return (scale * synth.hash_normal(113, name, shape)).to(bf)


def _same(got, ref, what):
    assert torch.equal(got[0].cpu(), ref[0].cpu()), f"{what}: codes"
    assert torch.equal(got[1].cpu().view(torch.int32), ref[1].cpu().view(torch.int32)), f"{what}: scales"


# ---- 1. quantiser -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1536, 8960, 10240])       # 1536 / 8960: the register-resident kernel (NCH 4 / 18); 10240: two-pass
def test_quantize_rows_f8_is_bit_identical_to_the_restatement(ops, K):
    for what, x in (("activations", _hard_x(4680, K, K)), ("weights", hn(f"qw{K}", (1536, K), K ** -0.5))):
        q, s = ops.quantize_rows_f8(x.to(DEV))
        assert q.dtype == U8 and s.dtype == torch.float32 and s.shape == (x.shape[0],)
        _same((q, s), fp8_ref.quantize(x), f"{what} K={K}")
        assert (q.cpu() & 0x7F).ne(0x7F).all(), f"{what}: NaN code"


# ---- 2. producers -------------------------------------------------------------------------------------------------------
def test_producers_emit_the_quantiser_bytes(ops):
    B, F, fs, C = 1, 3, 1560, 1536
    L = F * fs
    x = _hard_x(L, C, 11).view(B, L, C).to(DEV)
    e, mod = hn("pe", (B, F, 6, C), 0.5).to(DEV), hn("pm", (6, C), 0.1).to(DEV)
    for md in (mod, None):
        _same(ops.ln_modulate_f8(x, e, md, 3, 4, F, 1e-6), ops.quantize_rows_f8(ops.ln_modulate(x, e, md, 3, 4, F, 1e-6)),
              f"ln_modulate mod={md is not None}")
    tab = ops.modulation_table_f32(e, mod.view(1, 6, C), 0b010010)[0]
    _same(ops.ln_modulate_tab_f8(x, tab, 0, 1, F, 1e-6), ops.quantize_rows_f8(ops.ln_modulate_tab(x, tab, 0, 1, F, 1e-6)), "ln_modulate_tab")
    w, b = hn("nw", (C,), 0.2).to(DEV), hn("nb", (C,), 0.1).to(DEV)
    _same(ops.layernorm_affine_f8(x, w, b, 1e-6), ops.quantize_rows_f8(ops.layernorm_affine(x, w, b, 1e-6)), "layernorm_affine")


# ---- 3. exact data: every epilogue and every kernel instance ------------------------------------------------------------------
def _plan(ops, M, N, K):
    return ops.gemm_plan_f8(M, N, K).split(",")[0]


def test_every_epilogue_and_instance_with_exact_data(ops):
    """bias / residual / gate-residual against the host bit for bit; GELU bit for bit against ll_gemm_w8a8 on the same integers (the
    int8 kernel computes the same exact sums and shares the epilogue) and within 2 ulp of torch's tanh-GELU.  Production shapes, plus
    the 256x256 instance through the gemm_variant knob."""
    lib = ops._lib.load()
    B, F, fs = 1, 3, 1560
    M = B * F * fs
    seen = set()
    cases = [(4608, 1536, 0), (1536, 1536, 0), (8960, 1536, 0), (1536, 8960, 0), (4608, 1536, 3)]
    try:
        for N, K, variant in cases:
            assert lib.ll_set_tuning(b"gemm_variant", variant) == 0
            seen.add(_plan(ops, M, N, K))
            cx, cw, sx, sw = _exact_operands(M, N, K, N + K)
            xq, wq = cx.to(torch.float8_e4m3fn).view(U8), cw.to(torch.float8_e4m3fn).view(U8)
            x8, w8 = cx.to(torch.int8).to(DEV), cw.to(torch.int8).to(DEV)
            acc = (cx.double() @ cw.double().t()).float()
            assert acc.abs().max() < 2 ** 24
            bias = hn(f"b{N}", (N,), 0.1)
            v_ref = (acc * (sx.unsqueeze(1) * sw.unsqueeze(0)) + bias.float()).to(bf)
            d = [t.to(DEV) for t in (xq, sx, wq, sw)]
            bd = bias.to(DEV)
            v = ops.gemm_f8(*d, bd).cpu()
            assert torch.equal(v, v_ref), f"bias {N}x{K} v{variant}: {(v.float() - v_ref.float()).abs().max()}"
            g = ops.gemm_f8(*d, bd, ops.EPI_BIAS_GELU).cpu()
            g8 = ops.gemm_w8a8(x8, d[1], w8, d[3], bd, ops.EPI_BIAS_GELU).cpu()
            assert torch.equal(g, g8), f"gelu vs int8 kernel {N}x{K}"
            assert_bf16_close(g, _epi_ref(v_ref, 1), 2, 0.97, f"gelu {N}x{K}")
            if N != 1536:
                continue
            res = hn("res", (M, N))
            assert torch.equal(ops.gemm_f8(*d, bd, ops.EPI_BIAS_RES, res=res.to(DEV)).cpu(), _epi_ref(v_ref, 3, res)), f"res {K}"
            e, mod = hn("e", (B, F, 6, N), 0.5), hn("mod", (6, N), 0.1)
            for md in (mod, None):
                got = ops.gemm_f8(*d, bd, ops.EPI_BIAS_GATE_RES, res=res.to(DEV), e=e.to(DEV), mod=None if md is None else md.to(DEV),
                                  gate_idx=5, rows_per_batch=F * fs, frame_len=fs).cpu()
                assert torch.equal(got, _epi_ref(v_ref, 2, res, e, md, 5, fs)), f"gate-res {K} mod={md is not None}"
    finally:
        lib.ll_set_tuning(b"gemm_variant", 0)
    assert seen == {"gemm_kernel_v5<f8> tile 256x192", "gemm_kernel_v2<f8> tile 256x128", "gemm_kernel_v5<f8> tile 256x224",
                    "gemm_kernel_v5<f8> tile 256x256"}, seen


def test_qkv_form_writes_q_k_to_out_and_v_to_the_cache_slots(ops):
    B, F, fs, C = 1, 3, 1560, 1536
    L = F * fs
    cx, cw, sx, sw = _exact_operands(L, 3 * C, C, 7)
    d = [t.to(DEV) for t in (cx.to(torch.float8_e4m3fn).view(U8), sx, cw.to(torch.float8_e4m3fn).view(U8), sw)]
    bias = hn("qb", (3 * C,), 0.1).to(DEV)
    full = ops.gemm_f8(*d, bias).view(B, L, 3 * C)
    S, ws, ro, wl = 12 * fs, 9 * fs, fs, 2 * fs
    cache = torch.full((B, S, 12, 128), 7.0, dtype=bf, device=DEV)
    qkv = ops.gemm_f8_qkv_v_insert((d[0], d[1]), (d[2], d[3]), bias, cache, ws, ro, wl, B, L)
    assert torch.equal(qkv[..., : 2 * C], full[..., : 2 * C])
    cv = cache.view(B, S, C)
    assert torch.equal(cv[:, ws: ws + wl], full[:, ro: ro + wl, 2 * C:])
    assert (cv[:, :ws] == 7).all() and (cv[:, ws + wl:] == 7).all()


# ---- 4. random data ---------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("N,K", [(4608, 1536), (1536, 8960)])
def test_random_data_vs_fp64_and_not_int8_or_bf16(ops, N, K):
    """The bias form against the fp64 product of the dequantised operands at 1 bf16 ulp; ll_gemm_w8a8 and ll_gemm_bf16 on the same bf16
    operands fail that bound (so FP8 arithmetic ran)."""
    M = 4680
    x, w, bias = hn(f"x{K}", (M, K)), hn(f"w{N}{K}", (N, K), K ** -0.5), hn(f"b{N}", (N,), 0.1)
    xd, wd, bd = x.to(DEV), w.to(DEV), bias.to(DEV)
    xq, sx = ops.quantize_rows_f8(xd)
    wq, sw = ops.quantize_rows_f8(wd)
    acc = fp8_ref.decode(xq) @ fp8_ref.decode(wq).t()
    want = (acc.float() * (sx.cpu().unsqueeze(1) * sw.cpu().unsqueeze(0)) + bias.float()).to(bf)
    got = ops.gemm_f8(xq, sx, wq, sw, bd)
    assert_bf16_close(got, want, 1, 0.97, f"f8 {N}x{K}")
    x8, s8 = ops.quantize_rows(xd)
    w8, t8 = ops.quantize_rows(wd)
    assert not _within_1ulp(ops.gemm_w8a8(x8, s8, w8, t8, bd), want), "int8 passes the FP8 bound"
    assert not _within_1ulp(ops.gemm(xd, wd, bd), want), "bf16 passes the FP8 bound"


# ---- 5. outliers ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [4608, 8960])
def test_outlier_channels_fp8_rowwise_vs_int8(ops, N):
    M, K = 4680, 1536
    x = hn("ox", (M, K))
    x[:, [400, 1400]] *= 100
    w = hn(f"ow{N}", (N, K), K ** -0.5)
    exact = x.double() @ w.double().t()
    bias = torch.zeros(N, dtype=bf, device=DEV)
    xd, wd = x.to(DEV), w.to(DEV)
    y_f8 = ops.gemm_f8(*ops.quantize_rows_f8(xd), *ops.quantize_rows_f8(wd), bias).cpu()
    y_i8 = ops.gemm_w8a8(*ops.quantize_rows(xd), *ops.quantize_rows(wd), bias).cpu()
    r_f8, r_i8 = rel_l2(y_f8, exact), rel_l2(y_i8, exact)
    print(f"outliers, N={N}: rel-L2 to the exact product: fp8_rowwise {r_f8:.3e}, int8 {r_i8:.3e} (ratio {r_f8 / r_i8:.3f})")
    assert r_f8 < 0.6 * r_i8, (r_f8, r_i8)
