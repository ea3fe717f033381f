"""MXFP6 block linears on the MI355X (v_mfma_scale_f32_16x16x128_f8f6f4 with E2M3 operands), pinned to the scheme's definition
(tests/mx6_ref.py): the operand / scale lane map with exact data, quantiser bytes, the fused producers and the FFN1 MXFP6 epilogue
bit for bit, every epilogue and the QKV cache slots with exact data, random data against the fp64 product of the dequantised operands
(a bound the MXFP8 and bf16 GEMMs fail), outliers against int8.  The mode at model level (one real-shape block against its oracle,
the 30-layer steady state, config 2 free-running, the mode beside MX self-attention) is tests/test_quant_model_gpu.py's "mxfp6" row."""
import pytest
import torch

import mx6_ref
import mx_ref
from longlive_amd import synth
from quant_exact import epi_ref as _epi_ref
from quant_exact import hard_x_mx as _hard_x
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
    return (scale * synth.hash_normal(131, name, shape)).to(bf)


def _same(got, ref, what):
    assert torch.equal(got[0].cpu(), ref[0].cpu()), f"{what}: codes"
    assert torch.equal(got[1].cpu(), ref[1].cpu()), f"{what}: scales"


def _exact(rows, K, seed, asym=False):
    """Small-integer E2M3 codes (exact values -2 .. 2) and a distinct power-of-two scale per (row, K-block): (packed, scales,
    codes as float).  Every fp32 sum of the GEMM is then exact."""
    g = torch.Generator().manual_seed(seed)
    c = torch.randint(-2, 3, (rows, K), generator=g).double()
    if asym:
        c[:, 0] = (torch.arange(rows) % 3).double()                     # W is not X's pattern transposed
    r, b = torch.arange(rows).view(rows, 1), torch.arange(K // 32).view(1, -1)
    ex = ((r * (5 if asym else 3) + b * (3 if asym else 5)) % 7) - 3
    codes = mx6_ref.encode(c.numpy())
    packed = torch.from_numpy(mx6_ref.pack(codes))
    return packed, (ex + 127).to(U8), c * torch.pow(2.0, ex.double()).repeat_interleave(32, 1)


# ---- 1. operand map -----------------------------------------------------------------------------------------------------------
def test_gemm_mx6_lane_map_with_exact_data(ops):
    """Small integer codes, a distinct power-of-two scale per (row, K-block) on both sides, an asymmetric B, K = 512 (two stages):
    every fp32 sum is exact, so the GEMM must equal the exact product bit for bit; a wrong k order inside a lane's 192 bits, a wrong
    chunk order, a swapped operand map, a transposed C-write or a scale byte taken from the wrong lane / byte all change it."""
    M, N, K = 300, 256, 512
    xq, sx, xv = _exact(M, K, 5)
    wq, sw, wv = _exact(N, K, 6, asym=True)
    want = (xv @ wv.t()).to(bf)
    got = ops.gemm_mx6((xq.to(DEV), sx.to(DEV)), (wq.to(DEV), sw.to(DEV)), torch.zeros(N, dtype=bf, device=DEV)).cpu()
    assert torch.equal(got, want), (got.float() - want.float()).abs().max()


# ---- 2. quantiser ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1536, 8960, 10240])
def test_quantize_mx6_is_bit_identical_to_the_restatement(ops, K):
    x = _hard_x(4680, K, K)
    q, s = ops.quantize_mx6(x.to(DEV))
    rq, rs = mx6_ref.quantize(x)
    assert q.dtype == U8 and q.shape == (4680, K // 4 * 3) and s.shape == (4680, K // 32)
    assert torch.equal(s.cpu(), rs), "scales"
    assert torch.equal(q.cpu(), rq), "codes"


# ---- 3. producers and the FFN1 epilogue -------------------------------------------------------------------------------------------
def test_producers_and_ffn1_epilogue_emit_the_quantiser_bytes(ops):
    B, F, fs, C, Nf = 1, 3, 1560, 1536, 8960
    L = F * fs
    x = _hard_x(L, C, 11).view(B, L, C).to(DEV)
    e, mod = hn("pe", (B, F, 6, C), 0.5).to(DEV), hn("pm", (6, C), 0.1).to(DEV)
    for md in (mod, None):
        _same(ops.ln_modulate_mx6(x, e, md, 3, 4, F, 1e-6), ops.quantize_mx6(ops.ln_modulate(x, e, md, 3, 4, F, 1e-6)),
              f"ln_modulate mod={md is not None}")
    tab = ops.modulation_table_f32(e, mod.view(1, 6, C), 0b010010)[0]
    _same(ops.ln_modulate_tab_mx6(x, tab, 3, 4, F, 1e-6), ops.quantize_mx6(ops.ln_modulate_tab(x, tab, 3, 4, F, 1e-6)), "ln_modulate_tab")
    w, b = hn("nw", (C,), 0.2).to(DEV), hn("nb", (C,), 0.1).to(DEV)
    _same(ops.layernorm_affine_mx6(x, w, b, 1e-6), ops.quantize_mx6(ops.layernorm_affine(x, w, b, 1e-6)), "layernorm_affine")
    xm = ops.quantize_mx6(x)
    w1, b1 = ops.quantize_mx6(hn("f1w", (Nf, C), C ** -0.5).to(DEV)), hn("f1b", (Nf,), 0.1).to(DEV)
    _same(ops.gemm_mx6(xm, w1, b1, ops.EPI_BIAS_GELU, mx_out=True), ops.quantize_mx6(ops.gemm_mx6(xm, w1, b1, ops.EPI_BIAS_GELU)),
          "ffn1 mx6 epilogue")


# ---- 4. every epilogue with exact data ------------------------------------------------------------------------------------------------
def _as_mx8(v):
    """The same exact operand values as MXFP8 (e4m3 holds -2 .. 2 too): codes and scales for ll_gemm_mx."""
    return mx_ref.quantize(v.to(bf))


@pytest.mark.parametrize("N,K", [(4608, 1536), (1536, 1536), (8960, 1536), (1536, 8960)])
def test_every_epilogue_with_exact_data(ops, N, K):
    """Exact sums: the bias form equals the host bit for bit, and every epilogue equals ll_gemm_mx on the same values bit for bit (the
    two kernels compute the same exact fp32 sums and share the epilogues), the residual and gate forms also the host's rounding points."""
    B, F, fs = 1, 3, 1560
    M = B * F * fs
    xq, sx, xv = _exact(M, K, N + K)
    wq, sw, wv = _exact(N, K, N - K, asym=True)
    assert (xv.abs() <= 2 ** 3 * 2).all()
    acc = xv @ wv.t()
    bias = hn(f"b{N}", (N,), 0.1)
    d6 = ((xq.to(DEV), sx.to(DEV)), (wq.to(DEV), sw.to(DEV)))
    d8 = tuple(tuple(t.to(DEV) for t in _as_mx8(v)) for v in (xv, wv))
    bd = bias.to(DEV)
    v = ops.gemm_mx6(*d6, bd).cpu()
    assert torch.equal(v, _epi_ref(acc, bias, 0)), f"bias {N}x{K}"
    assert torch.equal(v, ops.gemm_mx(*d8, bd).cpu())
    zero = torch.zeros_like(bias)
    if N != 1536:
        g = ops.gemm_mx6(*d6, bd, ops.EPI_BIAS_GELU).cpu()
        assert torch.equal(g, ops.gemm_mx(*d8, bd, ops.EPI_BIAS_GELU).cpu()), f"gelu {N}x{K}"
        assert_bf16_close(g, _epi_ref(v, zero, 1), 2, 0.97, f"gelu {N}x{K}")
        return
    res = hn("res", (M, N))
    got = ops.gemm_mx6(*d6, bd, ops.EPI_BIAS_RES, res=res.to(DEV)).cpu()
    assert torch.equal(got, _epi_ref(v, zero, 3, res)), f"res {K}"
    e, mod = hn("e", (B, F, 6, N), 0.5), hn("mod", (6, N), 0.1)
    for md in (mod, None):
        kw = dict(res=res.to(DEV), e=e.to(DEV), mod=None if md is None else md.to(DEV), gate_idx=5, rows_per_batch=F * fs, frame_len=fs)
        got = ops.gemm_mx6(*d6, bd, ops.EPI_BIAS_GATE_RES, **kw).cpu()
        assert torch.equal(got, ops.gemm_mx(*d8, bd, ops.EPI_BIAS_GATE_RES, **kw).cpu()), f"gate-res {K} mod={md is not None}"
        assert_bf16_close(got, _epi_ref(v, zero, 2, res, e, md, 5, fs), 1, 0.99, f"gate-res {K} mod={md is not None}")


def test_batch2_gate_residual_and_qkv_cache_slots_with_exact_data(ops):
    B, F, fs, C = 2, 3, 520, 1536
    L = F * fs
    M = B * L
    xq, sx, xv = _exact(M, C, 21)
    wq, sw, wv = _exact(3 * C, C, 22, asym=True)
    bias = hn("qb", (3 * C,), 0.1)
    xm, wm = (xq.view(B, L, -1).to(DEV), sx.to(DEV)), (wq.to(DEV), sw.to(DEV))
    full = ops.gemm_mx6(xm, wm, bias.to(DEV))
    assert torch.equal(full.view(M, -1).cpu(), _epi_ref(xv @ wv.t(), bias, 0)), "B=2"
    # gate-residual with two batches: per-batch, per-frame gates
    oq, osw, ov = _exact(C, C, 23, asym=True)
    bo = hn("ob", (C,), 0.1)
    vo = _epi_ref(xv @ ov.t(), bo, 0)
    res, e = hn("ores", (M, C)), hn("oe", (B, F, 6, C), 0.5)
    got = ops.gemm_mx6(xm, (oq.to(DEV), osw.to(DEV)), bo.to(DEV), ops.EPI_BIAS_GATE_RES, res=res.to(DEV), e=e.to(DEV), gate_idx=2,
                       rows_per_batch=L, frame_len=fs)
    assert_bf16_close(got.view(M, C), _epi_ref(vo, torch.zeros_like(bo), 2, res, e, None, 2, fs), 1, 0.99, "gate-res B=2")
    # fused V insert: q / k thirds and the written cache slots equal the unfused projection's
    S, ws, ro, wl = 4 * fs, 2 * fs, fs, 2 * fs
    cache = torch.full((B, S, 12, 128), 7.0, dtype=bf, device=DEV)
    qkv = ops.gemm_mx6_qkv_v_insert(xm, wm, bias.to(DEV), cache, ws, ro, wl, B, L)
    assert torch.equal(qkv[..., : 2 * C], full[..., : 2 * C])
    cv = cache.view(B, S, C)
    assert torch.equal(cv[:, ws: ws + wl], full[:, ro: ro + wl, 2 * C:])
    assert (cv[:, :ws] == 7).all() and (cv[:, ws + wl:] == 7).all()


# ---- 5. random data ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", [(4608, 1536), (1536, 8960)])
def test_random_data_vs_fp64_and_not_mxfp8_or_bf16(ops, N, K):
    """The bias form against the fp64 product of the MXFP6-dequantised operands at 1 bf16 ulp; ll_gemm_mx and ll_gemm_bf16 on the same
    bf16 operands fail that bound (so E2M3 arithmetic ran)."""
    M = 4680
    x, w, bias = hn(f"x{K}", (M, K)), hn(f"w{N}{K}", (N, K), K ** -0.5), hn(f"b{N}", (N,), 0.1)
    xd, wd, bd = x.to(DEV), w.to(DEV), bias.to(DEV)
    xm, wm = ops.quantize_mx6(xd), ops.quantize_mx6(wd)
    acc = mx6_ref.dequantize(*xm) @ mx6_ref.dequantize(*wm).t()
    want = (acc.float() + bias.float()).to(bf)
    assert_bf16_close(ops.gemm_mx6(xm, wm, bd), want, 1, 0.97, f"mx6 {N}x{K}")
    assert not _within_1ulp(ops.gemm_mx(ops.quantize_mx(xd), ops.quantize_mx(wd), bd), want), "mxfp8 passes the MXFP6 bound"
    assert not _within_1ulp(ops.gemm(xd, wd, bd), want), "bf16 passes the MXFP6 bound"


# ---- 6. outliers ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [4608, 8960])
def test_outlier_channels_mxfp6_vs_int8(ops, N):
    M, K = 4680, 1536
    x = hn("ox", (M, K))
    x[:, [400, 1400]] *= 100
    w = hn(f"ow{N}", (N, K), K ** -0.5)
    exact = x.double() @ w.double().t()
    bias = torch.zeros(N, dtype=bf, device=DEV)
    xd, wd = x.to(DEV), w.to(DEV)
    y6 = ops.gemm_mx6(ops.quantize_mx6(xd), ops.quantize_mx6(wd), bias).cpu()
    xq, sx = ops.quantize_rows(xd)
    wq, sw = ops.quantize_rows(wd)
    y8 = ops.gemm_w8a8(xq, sx, wq, sw, bias).cpu()
    r6, r8 = rel_l2(y6, exact), rel_l2(y8, exact)
    print(f"outliers, N={N}: rel-L2 to the exact product: mxfp6 {r6:.3e}, int8 {r8:.3e} (ratio {r6 / r8:.3f})")
    assert r6 < r8, (r6, r8)
