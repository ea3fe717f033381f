"""W4A6 block linears on the MI355X (v_mfma_scale_f32_16x16x128_f8f6f4 with E2M1 weights and E2M3 activations, cbsz = 4 / blgp = 2),
pinned to the scheme's definition (tests/mx4_ref.py): the FP4 operand / scale lane map with exact data, quantiser bytes, every epilogue
and the QKV cache slots bit for bit against ll_gemm_mx6 on the same values re-encoded as E2M3 (every E2M1 value is an E2M3 value),
random data against the fp64 product of the dequantised operands (a bound the MXFP6 GEMM fails).  The mode at model level (one
real-shape block against its oracle, the 30-layer steady state and config 2 free-running apart from the same runs in mxfp6, the mode
beside MX self-attention) is tests/test_quant_model_gpu.py's "mxfp4_a6" row."""
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
    return (scale * synth.hash_normal(137, name, shape)).to(bf)


def _exact_x(rows, K, seed):
    """MXFP6 activations: (packed E2M3, scales, values).  Every fp32 sum of the GEMM is exact."""
    c, ex, v = _codes_and_scales(rows, K, seed, False)
    return torch.from_numpy(mx6_ref.pack(mx6_ref.encode(c.numpy()))), (ex + 127).to(U8), v


def _exact_w(rows, K, seed):
    """MXFP4 weights: (packed E2M1, scales, values, the same values as packed E2M3 under the same scale bytes)."""
    c, ex, v = _codes_and_scales(rows, K, seed, True)
    w4 = torch.from_numpy(mx4_ref.pack(mx4_ref.encode(c.numpy())))
    w6 = torch.from_numpy(mx6_ref.pack(mx6_ref.encode(c.numpy())))
    return w4, (ex + 127).to(U8), v, w6


def _dev(*ts):
    return tuple(t.to(DEV) for t in ts)


# ---- 1. operand map -----------------------------------------------------------------------------------------------------------
def test_gemm_mx4w6_lane_map_with_exact_data(ops):
    """Small integer codes, a distinct power-of-two scale per (row, K-block) on both sides, an asymmetric W, K = 512 (two stages):
    every fp32 sum is exact, so the GEMM must equal the exact product bit for bit; a wrong nibble order inside a lane's 128 bits, a
    wrong block order, a swapped operand side or a scale byte taken from the wrong lane / byte all change it."""
    M, N, K = 300, 256, 512
    xq, sx, xv = _exact_x(M, K, 5)
    wq, sw, wv, _ = _exact_w(N, K, 6)
    want = (xv @ wv.t()).to(bf)
    got = ops.gemm_mx4w6(_dev(xq, sx), _dev(wq, sw), torch.zeros(N, dtype=bf, device=DEV)).cpu()
    assert torch.equal(got, want), (got.float() - want.float()).abs().max()


# ---- 2. quantiser ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1536, 8960, 10240])
def test_quantize_mx4_is_bit_identical_to_the_restatement(ops, K):
    """Outlier channels, all-zero blocks, tiny blocks next to a large value and bf16-subnormal blocks (tests/quant_exact.py hard_x_mx),
    plus -0 and exact ties."""
    x = _hard_x(4680, K, K)
    x[3, 128:160] = -0.0
    x[5, 160:192] = torch.tensor([6.0, 0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0] * 4)
    q, s = ops.quantize_mx4(x.to(DEV))
    rq, rs = mx4_ref.quantize(x)
    assert q.dtype == U8 and q.shape == (4680, K // 2) and s.shape == (4680, K // 32)
    assert torch.equal(s.cpu(), rs), "scales"
    assert torch.equal(q.cpu(), rq), "codes"


# ---- 3. every epilogue against ll_gemm_mx6 with exact data -------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", [(4608, 1536), (1536, 1536), (8960, 1536), (1536, 8960)])
def test_every_epilogue_equals_mx6_with_exact_data(ops, N, K):
    """The weights re-encoded as E2M3 under the same scale bytes make ll_gemm_mx6 an independent implementation of the same exact
    fp32 sums: every epilogue must equal it bit for bit, the MXFP6 output bytes of the FFN1 form included; the bias form also equals
    the host."""
    B, F, fs = 1, 3, 1560
    M = B * F * fs
    xq, sx, xv = _exact_x(M, K, N + K)
    wq, sw, wv, w6 = _exact_w(N, K, N - K)
    x, w4, w6 = _dev(xq, sx), _dev(wq, sw), _dev(w6, sw)
    bias = hn(f"b{N}", (N,), 0.1)
    bd = bias.to(DEV)
    v = ops.gemm_mx4w6(x, w4, bd).cpu()
    assert torch.equal(v, _epi_ref(xv @ wv.t(), bias, 0)), f"bias {N}x{K}"
    assert torch.equal(v, ops.gemm_mx6(x, w6, bd).cpu())
    if N != 1536:
        assert torch.equal(ops.gemm_mx4w6(x, w4, bd, ops.EPI_BIAS_GELU).cpu(), ops.gemm_mx6(x, w6, bd, ops.EPI_BIAS_GELU).cpu()), "gelu"
        if N % 256 == 0:
            g4, g6 = ops.gemm_mx4w6(x, w4, bd, ops.EPI_BIAS_GELU, mx_out=True), ops.gemm_mx6(x, w6, bd, ops.EPI_BIAS_GELU, mx_out=True)
            assert torch.equal(g4[0].cpu(), g6[0].cpu()) and torch.equal(g4[1].cpu(), g6[1].cpu()), "gelu mxfp6 output"
        return
    res = hn("res", (M, N)).to(DEV)
    got = ops.gemm_mx4w6(x, w4, bd, ops.EPI_BIAS_RES, res=res).cpu()
    assert torch.equal(got, ops.gemm_mx6(x, w6, bd, ops.EPI_BIAS_RES, res=res).cpu()), f"res {K}"
    assert torch.equal(got, _epi_ref(v, torch.zeros_like(bias), 3, res.cpu())), f"res {K} host"
    e, mod = hn("e", (B, F, 6, N), 0.5).to(DEV), hn("mod", (6, N), 0.1).to(DEV)
    for md in (mod, None):
        kw = dict(res=res, e=e, mod=md, gate_idx=5, rows_per_batch=F * fs, frame_len=fs)
        got = ops.gemm_mx4w6(x, w4, bd, ops.EPI_BIAS_GATE_RES, **kw).cpu()
        assert torch.equal(got, ops.gemm_mx6(x, w6, bd, ops.EPI_BIAS_GATE_RES, **kw).cpu()), f"gate-res {K} mod={md is not None}"


def test_batch2_gate_residual_and_qkv_cache_slots_with_exact_data(ops):
    B, F, fs, C = 2, 3, 520, 1536
    L = F * fs
    M = B * L
    xq, sx, xv = _exact_x(M, C, 21)
    wq, sw, wv, w6 = _exact_w(3 * C, C, 22)
    bias = hn("qb", (3 * C,), 0.1)
    xm, wm = (xq.view(B, L, -1).to(DEV), sx.to(DEV)), _dev(wq, sw)
    full = ops.gemm_mx4w6(xm, wm, bias.to(DEV))
    assert torch.equal(full.view(M, -1).cpu(), _epi_ref(xv @ wv.t(), bias, 0)), "B=2"
    # gate-residual with two batches: per-batch, per-frame gates, against ll_gemm_mx6
    oq, osw, _, o6 = _exact_w(C, C, 23)
    bo = hn("ob", (C,), 0.1).to(DEV)
    res, e = hn("ores", (M, C)).to(DEV), hn("oe", (B, F, 6, C), 0.5).to(DEV)
    kw = dict(res=res, e=e, gate_idx=2, rows_per_batch=L, frame_len=fs)
    got = ops.gemm_mx4w6(xm, _dev(oq, osw), bo, ops.EPI_BIAS_GATE_RES, **kw)
    assert torch.equal(got.cpu(), ops.gemm_mx6(xm, _dev(o6, osw), bo, ops.EPI_BIAS_GATE_RES, **kw).cpu()), "gate-res B=2"
    # fused V insert: q / k thirds and the written cache slots equal the unfused projection's (and ll_gemm_mx6_qkv's)
    S, ws, ro, wl = 4 * fs, 2 * fs, fs, 2 * fs
    cache = torch.full((B, S, 12, 128), 7.0, dtype=bf, device=DEV)
    qkv = ops.gemm_mx4w6_qkv_v_insert(xm, wm, bias.to(DEV), cache, ws, ro, wl, B, L)
    assert torch.equal(qkv[..., : 2 * C], full[..., : 2 * C])
    cv = cache.view(B, S, C)
    assert torch.equal(cv[:, ws: ws + wl], full[:, ro: ro + wl, 2 * C:])
    assert (cv[:, :ws] == 7).all() and (cv[:, ws + wl:] == 7).all()
    cache6 = torch.full_like(cache, 7.0)
    qkv6 = ops.gemm_mx6_qkv_v_insert(xm, _dev(w6, sw), bias.to(DEV), cache6, ws, ro, wl, B, L)
    assert torch.equal(qkv6[..., : 2 * C], qkv[..., : 2 * C]) and torch.equal(cache6, cache)


# ---- 4. random data ---------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("N,K", [(4608, 1536), (1536, 1536), (8960, 1536), (1536, 8960)])
def test_random_data_vs_fp64_and_not_mxfp6(ops, N, K):
    """The bias form at the real shapes against the fp64 product of the dequantised operands (MXFP6 x, E2M1 w) at 1 bf16 ulp; the
    MXFP6 GEMM on the same bf16 operands fails that bound (so E2M1 weights were used)."""
    M = 4680
    x, w, bias = hn(f"x{K}", (M, K)), hn(f"w{N}{K}", (N, K), K ** -0.5), hn(f"b{N}", (N,), 0.1)
    xd, wd, bd = x.to(DEV), w.to(DEV), bias.to(DEV)
    xm, wm = ops.quantize_mx6(xd), ops.quantize_mx4(wd)
    acc = mx6_ref.dequantize(*xm) @ mx4_ref.dequantize(*wm).t()
    want = (acc.float() + bias.float()).to(bf)
    assert_bf16_close(ops.gemm_mx4w6(xm, wm, bd), want, 1, 0.97, f"mx4w6 {N}x{K}")
    assert not _within_1ulp(ops.gemm_mx6(xm, ops.quantize_mx6(wd), bd), want), "mxfp6 passes the W4A6 bound"
