"""MXFP8 block linears on the MI355X (v_mfma_scale_f32_16x16x128_f8f6f4), pinned to the scheme's definition (tests/mx_ref.py):
quantiser bytes, the operand / scale lane map with exact data, every GEMM epilogue against the fp64 product of the dequantised
operands, the fused producers and the FFN1 MX epilogue bit for bit, outlier robustness against int8.  The mode at model level (one
real-shape block against its oracle, the 30-layer steady state, config 2 free-running) is tests/test_quant_model_gpu.py's "mxfp8" row."""
import pytest
import torch

import mx_ref
from longlive_amd import synth
from quant_exact import epi_ref as _epi_ref
from quant_exact import hard_x_mx as _hard_x
from util import assert_bf16_close, bf, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
U8 = torch.uint8


@pytest.fixture(scope="module")
def ops():
    from longlive_amd import ops as O
    return O


def hn(name, shape, scale=1.0):
    return (scale * synth.hash_normal(97, name, shape)).to(bf)


def _bytes(q):
    return q.view(U8).cpu()


@pytest.mark.parametrize("K", [1536, 8960])
def test_quantize_mx_is_bit_identical_to_the_restatement(ops, K):
    x = _hard_x(4680, K, K)
    q, s = ops.quantize_mx(x.to(DEV))
    rq, rs = mx_ref.quantize(x)
    assert q.dtype == torch.float8_e4m3fn and s.shape == (4680, K // 32)
    assert torch.equal(_bytes(s), rs), "scales"
    assert torch.equal(_bytes(q), rq.view(U8)), "codes"


def test_gemm_lane_map_with_exact_data(ops):
    """Small integer codes, a distinct power-of-two scale per (row, K-block) on both sides, an asymmetric B: every fp32 sum is exact
    (multiples of 2^-6 below 2^17), so the GEMM must equal the exact product bit for bit; a swapped operand map, a transposed
    C-write or a scale byte taken from the wrong lane / byte all change it."""
    M, N, K = 300, 256, 256
    g = torch.Generator().manual_seed(5)
    cx = torch.randint(-2, 3, (M, K), generator=g).float()
    cw = torch.randint(-2, 3, (N, K), generator=g).float()
    cw[:, 0] += torch.arange(N) % 3                       # asymmetric: W is not X's shape / pattern transposed
    r, b = torch.arange(M).view(M, 1), torch.arange(K // 32).view(1, -1)
    ex = ((r * 3 + b * 5) % 7) - 3
    n = torch.arange(N).view(N, 1)
    ew = ((n * 5 + b * 3) % 7) - 3
    xq, wq = cx.to(torch.float8_e4m3fn), cw.to(torch.float8_e4m3fn)
    sx, sw = (ex + 127).to(U8), (ew + 127).to(U8)
    want = (mx_ref.dequantize(xq, sx) @ mx_ref.dequantize(wq, sw).t()).to(bf)
    got = ops.gemm_mx((xq.to(DEV), sx.to(DEV)), (wq.to(DEV), sw.to(DEV)), torch.zeros(N, dtype=bf, device=DEV)).cpu()
    assert torch.equal(got, want), (got.float() - want.float()).abs().max()


@pytest.mark.parametrize("N,K", [(4608, 1536), (1536, 1536), (8960, 1536), (1536, 8960)])
def test_gemm_mx_epilogues_vs_fp64(ops, N, K):
    """The bias form against the fp64 product of the dequantised operands (fp32 accumulation order: <= 1 ulp); every other epilogue
    against the host epilogue applied to that bias output (its rounding points exactly: <= 1 ulp, GELU's sigmoid form <= 2)."""
    B, F, fs = 1, 3, 1560
    M = B * F * fs
    x, w, bias = hn(f"x{K}", (M, K)), hn(f"w{N}{K}", (N, K), K ** -0.5), hn(f"b{N}", (N,), 0.1)
    xm, wm = ops.quantize_mx(x.to(DEV)), ops.quantize_mx(w.to(DEV))
    acc = mx_ref.dequantize(*[t.cpu() for t in xm]) @ mx_ref.dequantize(*[t.cpu() for t in wm]).t()
    bd = bias.to(DEV)
    v = ops.gemm_mx(xm, wm, bd).cpu()
    assert_bf16_close(v, _epi_ref(acc, bias, 0), 1, 0.97, f"mx bias {N}x{K}")
    zero = torch.zeros_like(bias)
    if N != 1536:
        assert_bf16_close(ops.gemm_mx(xm, wm, bd, ops.EPI_BIAS_GELU), _epi_ref(v, zero, 1), 2, 0.97, f"mx gelu {N}x{K}")
        return
    res = hn("res", (M, N))
    assert_bf16_close(ops.gemm_mx(xm, wm, bd, ops.EPI_BIAS_RES, res=res.to(DEV)), _epi_ref(v, zero, 3, res), 1, 0.99, "mx res")
    e, mod = hn("e", (B, F, 6, N), 0.5), hn("mod", (6, N), 0.1)
    for md in (mod, None):
        got = ops.gemm_mx(xm, wm, bd, ops.EPI_BIAS_GATE_RES, res=res.to(DEV), e=e.to(DEV), mod=None if md is None else md.to(DEV),
                          gate_idx=5, rows_per_batch=F * fs, frame_len=fs)
        assert_bf16_close(got, _epi_ref(v, zero, 2, res, e, md, 5, fs), 1, 0.99, f"mx gate-res mod={md is not None}")


def test_gemm_mx_batch2_and_qkv_cache_slots(ops):
    B, F, fs, C = 2, 3, 520, 1536
    L = F * fs
    M = B * L
    x, w, bias = hn("qx", (B, L, C)), hn("qw", (3 * C, C), C ** -0.5), hn("qb", (3 * C,), 0.1)
    xm, wm = ops.quantize_mx(x.to(DEV)), ops.quantize_mx(w.to(DEV))
    acc = mx_ref.dequantize(*[t.cpu() for t in xm]) @ mx_ref.dequantize(*[t.cpu() for t in wm]).t()
    full = ops.gemm_mx(xm, wm, bias.to(DEV))
    assert_bf16_close(full.view(M, -1), _epi_ref(acc, bias, 0), 1, 0.97, "mx B=2")
    # gate-residual with two batches: per-batch, per-frame gates
    wo, bo = hn("ow", (C, C), C ** -0.5), hn("ob", (C,), 0.1)
    wom = ops.quantize_mx(wo.to(DEV))
    vo = ops.gemm_mx(xm, wom, bo.to(DEV)).view(M, C).cpu()
    res, e = hn("ores", (M, C)), hn("oe", (B, F, 6, C), 0.5)
    got = ops.gemm_mx(xm, wom, bo.to(DEV), ops.EPI_BIAS_GATE_RES, res=res.to(DEV), e=e.to(DEV), gate_idx=2, rows_per_batch=L, frame_len=fs)
    assert_bf16_close(got.view(M, C), _epi_ref(vo, torch.zeros_like(bo), 2, res, e, None, 2, fs), 1, 0.99, "mx gate-res B=2")
    # fused V insert: q / k thirds and the written cache slots equal the unfused projection's
    S, ws, ro, wl = 4 * fs, 2 * fs, fs, 2 * fs
    cache = torch.full((B, S, 12, 128), 7.0, dtype=bf, device=DEV)
    qkv = ops.gemm_mx_qkv_v_insert(xm, wm, bias.to(DEV), cache, ws, ro, wl, B, L)
    assert torch.equal(qkv[..., : 2 * C], full[..., : 2 * C])
    cv = cache.view(B, S, C)
    assert torch.equal(cv[:, ws: ws + wl], full[:, ro: ro + wl, 2 * C:])
    assert (cv[:, :ws] == 7).all() and (cv[:, ws + wl:] == 7).all()


def test_producers_and_ffn1_epilogue_emit_the_quantiser_bytes(ops):
    B, F, fs, C, Nf = 1, 3, 1560, 1536, 8960
    L = F * fs
    x = _hard_x(L, C, 11).view(B, L, C).to(DEV)
    e, mod = hn("pe", (B, F, 6, C), 0.5).to(DEV), hn("pm", (6, C), 0.1).to(DEV)

    def same(got, ref, what):
        assert torch.equal(_bytes(got[0]), _bytes(ref[0])) and torch.equal(_bytes(got[1]), _bytes(ref[1])), what

    for md in (mod, None):
        same(ops.ln_modulate_mx(x, e, md, 3, 4, F, 1e-6), ops.quantize_mx(ops.ln_modulate(x, e, md, 3, 4, F, 1e-6)), f"ln_modulate mod={md is not None}")
    tab = ops.modulation_table_f32(e, mod.view(1, 6, C), 0b010010)[0]
    same(ops.ln_modulate_tab_mx(x, tab, 3, 4, F, 1e-6), ops.quantize_mx(ops.ln_modulate_tab(x, tab, 3, 4, F, 1e-6)), "ln_modulate_tab")
    w, b = hn("nw", (C,), 0.2).to(DEV), hn("nb", (C,), 0.1).to(DEV)
    same(ops.layernorm_affine_mx(x, w, b, 1e-6), ops.quantize_mx(ops.layernorm_affine(x, w, b, 1e-6)), "layernorm_affine")
    # FFN1 + GELU with MX output
    xm = ops.quantize_mx(x)
    w1, b1 = ops.quantize_mx(hn("f1w", (Nf, C), C ** -0.5).to(DEV)), hn("f1b", (Nf,), 0.1).to(DEV)
    same(ops.gemm_mx(xm, w1, b1, ops.EPI_BIAS_GELU, mx_out=True), ops.quantize_mx(ops.gemm_mx(xm, w1, b1, ops.EPI_BIAS_GELU)), "ffn1 mx epilogue")


@pytest.mark.parametrize("N", [4608, 8960])
def test_outlier_channels_mx_vs_int8(ops, N):
    """Two x100 channels flatten a whole token under a per-token int8 scale; per-32 blocks confine them to their block.  (MXFP8's own
    error here, ~3.7e-2, is e4m3's 3-bit mantissa on both operands; with four such channels the outliers carry most of the output's
    norm and the int8 distance falls to 6.8e-2: ratio 0.55, recorded in DESIGN.md section 5b.1.)"""
    M, K = 4680, 1536
    x = hn("ox", (M, K))
    x[:, [400, 1400]] *= 100
    w = hn(f"ow{N}", (N, K), K ** -0.5)
    exact = x.double() @ w.double().t()
    bias = torch.zeros(N, dtype=bf, device=DEV)
    xd, wd = x.to(DEV), w.to(DEV)
    y_mx = ops.gemm_mx(ops.quantize_mx(xd), ops.quantize_mx(wd), bias).cpu()
    xq, sx = ops.quantize_rows(xd)
    wq, sw = ops.quantize_rows(wd)
    y_i8 = ops.gemm_w8a8(xq, sx, wq, sw, bias).cpu()
    r_mx, r_i8 = rel_l2(y_mx, exact), rel_l2(y_i8, exact)
    print(f"outliers, N={N}: rel-L2 to the exact product: mxfp8 {r_mx:.3e}, int8 {r_i8:.3e} (ratio {r_mx / r_i8:.3f})")
    assert r_mx <= 0.5 * r_i8, (r_mx, r_i8)
