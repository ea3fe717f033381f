"""MXFP8 block linears on the MI355X (v_mfma_scale_f32_16x16x128_f8f6f4), pinned to the scheme's definition (tests/mx_ref.py):
quantiser bytes, the operand / scale lane map with exact data, every GEMM epilogue against the fp64 product of the dequantised
operands, the fused producers and the FFN1 MX epilogue bit for bit, outlier robustness against int8, one real-shape block against
the MX oracle, a 30-layer steady-state forward and config 2 free-running against the reference's bf16 goldens."""
import pytest
import torch

import mx_ref
from conftest import load_golden
from longlive_amd import synth
from quant_exact import hard_x_mx as _hard_x
from test_shipped_sizes_gpu import _config2_run, _have, _kv_fill, _new_caches, real30  # noqa: F401  (real30: module fixture)
from util import assert_bf16_close, bf, cosine, rel_l2

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


def _epi_ref(acc, bias, epi, res=None, e=None, mod=None, gate_idx=0, fs=1):
    """The bf16 epilogues' rounding points on the fp64 accumulator (ll_gemm_bf16, include/longlive_hip.h LL_EPI_*)."""
    v = (acc.float() + bias.float()).to(bf)
    if epi == 0:
        return v
    if epi == 1:
        return torch.nn.functional.gelu(v, approximate="tanh")
    if epi == 3:
        return (res.float() + v.float()).to(bf)
    B, F = e.shape[:2]
    gate = e[:, :, gate_idx] if mod is None else (mod[gate_idx].float() + e[:, :, gate_idx].float()).to(bf)
    gv = (v.view(B, F, fs, -1).float() * gate.float().unsqueeze(2)).to(bf).reshape(v.shape)
    return (res.float() + gv.float()).to(bf)


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


def test_mxfp8_block_vs_mx_oracle():
    """One real-shape block in steady state (Lk = 18720, roll + insert) with MXFP8 linears against MXRefModel, and against the bf16
    oracle: it must sit closer to the MX restatement than to bf16 (so the pass band excludes "did not quantise")."""
    from longlive_amd.model import CausalWanModelHIP, _kv_commit
    from oracle import ref_model as RM
    cfg = synth.longlive_1_3b(num_layers=1)
    fs, S = cfg.frame_seqlen, 12 * cfg.frame_seqlen
    sd = synth.synth_state_dict(cfg, seed=0, device=DEV, layers=[0])
    m = CausalWanModelHIP(cfg, device=DEV)
    m.load_state_dict(sd)
    for mod in m.modules():
        if hasattr(mod, "max_attention_size"):
            mod.max_attention_size = S
    x0 = synth.hash_normal(71, "blk.x", (1, 3 * fs, cfg.dim), device=DEV).to(bf)
    e0 = (0.3 * synth.hash_normal(71, "blk.e0", (1, 3, 6, cfg.dim), device=DEV)).to(bf)
    ctx = synth.hash_normal(71, "blk.ctx", (1, cfg.text_len, cfg.dim), device=DEV).to(bf)
    k, v = _kv_fill(cfg, 0, S)
    m.set_quant("mxfp8")
    xs = x0.clone()
    kv = dict(k=k.clone(), v=v.clone(), global_end_index=S, local_end_index=S)
    ca = {"k": torch.zeros(1, 512, 12, 128, dtype=bf, device=DEV), "v": torch.zeros(1, 512, 12, 128, dtype=bf, device=DEV), "is_init": False}
    plan = m.block_forward(0, xs, e0, ctx, kv, ca, 3, (30, 52), current_start=S)
    _kv_commit(kv, plan.G_new, plan.E_new)
    m.set_quant(None)
    got, gk, gv = xs.cpu(), kv["k"].cpu(), kv["v"].cpu()
    sdc = {kk: vv.cpu() for kk, vv in sd.items()}
    outs = {}
    for name, cls in (("mx", mx_ref.MXRefModel), ("bf16", RM.RefModel)):
        ref = cls(RM.RefConfig.from_cfg(cfg), sdc, frame_seqlen_for_max_attn=fs)
        ref.max_attention_size = S
        kvr = dict(k=k.cpu().clone(), v=v.cpu().clone(), global_end_index=S, local_end_index=S)
        car = dict(k=torch.zeros(1, 512, 12, 128, dtype=bf), v=torch.zeros(1, 512, 12, 128, dtype=bf), is_init=False)
        y, planr = ref.block(x0.cpu(), 0, e0.cpu(), (3, 30, 52), ctx.cpu(), kvr, car, S, False)
        outs[name] = (y, kvr, planr)
    r_mx, r_bf = rel_l2(got, outs["mx"][0]), rel_l2(got, outs["bf16"][0])
    d_block = rel_l2(x0.cpu(), outs["bf16"][0])
    print(f"mxfp8 block: vs MX oracle relL2 {r_mx:.2e} (cos {cosine(got, outs['mx'][0]):.6f}); vs bf16 oracle {r_bf:.2e}; "
          f"MX oracle vs bf16 oracle {rel_l2(outs['mx'][0], outs['bf16'][0]):.2e}; block update size {d_block:.2e}")
    assert r_mx < r_bf, (r_mx, r_bf)
    assert r_mx < 6e-3 and cosine(got, outs["mx"][0]) > 0.9999, r_mx
    kvr, planr = outs["mx"][1], outs["mx"][2]
    assert (kv["global_end_index"], kv["local_end_index"]) == (planr["G_new"], planr["E_new"])
    sl = torch.linspace(0, S - 1, 64).round().long()
    assert rel_l2(gk[0, sl], kvr["k"][0, sl]) < 5e-3 and rel_l2(gv[0, sl], kvr["v"][0, sl]) < 5e-3


@pytest.mark.skipif(not _have("real_fwd.pt"), reason="golden missing")
def test_mxfp8_steady_state_vs_reference(real30):
    """30 layers, steady state (roll + insert, Lk = 18720) with MXFP8 linears, against the reference's bf16 golden and our bf16 path,
    within the int8 test's bounds."""
    rec = load_golden("real_fwd.pt")
    cfg, gen = real30
    S = 12 * cfg.frame_seqlen
    prompt = {"prompt_embeds": synth.synth_prompt_embeds(cfg, seed=1, device=DEV)}
    noise = synth.synth_noise(cfg, 3, seed=0, device=DEV)
    outs = {}
    for mode in (None, "mxfp8"):
        gen.model.set_quant(mode)
        kv, ca = _new_caches(30, S)
        for i in range(30):
            kv[i]["k"], kv[i]["v"] = _kv_fill(cfg, i, S)
            kv[i]["global_end_index"] = S; kv[i]["local_end_index"] = S
        flow, _ = gen(noise, prompt, torch.full((1, 3), 625.0, device=DEV), kv_cache=kv, crossattn_cache=ca, current_start=S)
        outs[mode] = flow.cpu()
        assert (kv[0]["global_end_index"], kv[0]["local_end_index"]) == tuple(rec["idx_steady"])
    gen.model.set_quant(None)
    r_ref, r_bf = rel_l2(outs["mxfp8"], rec["flow_steady"]), rel_l2(outs["mxfp8"], outs[None])
    c_ref, c_bf = cosine(outs["mxfp8"], rec["flow_steady"]), cosine(outs["mxfp8"], outs[None])
    print(f"mxfp8 steady: vs reference bf16 {r_ref:.2e} (cos {c_ref:.6f}); vs HIP bf16 {r_bf:.2e} (cos {c_bf:.6f})")
    assert r_bf < 6e-2 and c_bf > 0.998
    assert r_ref < 7e-2 and c_ref > 0.997


@pytest.mark.skipif(not _have("config2_pipe.pt"), reason="golden missing")
def test_config2_mxfp8_free_running_vs_reference_bf16(real30):
    """Config 2's 21 frames with MXFP8 linears, free-running, against the reference's bf16 latents: per block rel-L2 <= 7e-2 and
    cosine >= 0.997, and no growth along the stream (the last block within 1.25x of the first)."""
    cfg, gen = real30
    gen.model.set_quant("mxfp8")
    try:
        rec, P, lat, spy = _config2_run(real30, teacher=False, check=False)
    finally:
        gen.model.set_quant(None)
    rs = []
    for blk in range(7):
        a, b = lat[:, 3 * blk: 3 * blk + 3].cpu(), rec["latents"][:, 3 * blk: 3 * blk + 3]
        r, c = rel_l2(a, b), cosine(a, b)
        rs.append(r)
        print(f"config 2 mxfp8 free-running: block {blk} latents vs reference bf16: relL2 {r:.2e} cos {c:.6f}")
        assert r < 7e-2 and c > 0.997, (blk, r, c)
    assert rs[-1] < 1.25 * rs[0], rs
