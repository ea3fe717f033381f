"""MXFP6 block linears on the MI355X (v_mfma_scale_f32_16x16x128_f8f6f4 with E2M3 operands), pinned to the scheme's definition
(tests/mx6_ref.py): the operand / scale lane map with exact data, quantiser bytes, the fused producers and the FFN1 MXFP6 epilogue
bit for bit, every epilogue and the QKV cache slots with exact data, random data against the fp64 product of the dequantised operands
(a bound the MXFP8 and bf16 GEMMs fail), outliers against int8, one real-shape block against Mx6RefModel, the 30-layer steady state and
config 2 free-running against the reference's bf16 goldens, and the mode beside MX self-attention."""
import pytest
import torch

import mx6_ref
import mx_ref
from conftest import load_golden
from longlive_amd import synth
from test_mx_gpu import _epi_ref, _hard_x
from test_shipped_sizes_gpu import _config2_run, _have, _kv_fill, _new_caches, real30  # noqa: F401  (real30: module fixture)
from util import assert_bf16_close, bf, bf16_ulp_distance, cosine, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
U8 = torch.uint8

# measured on one MI355X; the model-level bounds are about twice these.  The block's is 1.23x: twice would reach
# Mx6RefModel's own 6.75e-3 distance to the MXFP8 oracle, and the band must exclude that oracle.
MEASURED = dict(block=4.9e-3, steady_ref=4.9e-2, config2=3.7e-2, toy_attn=2.2e-3)
BLOCK_BOUND = 6.0e-3


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
def _within_1ulp(got, want):
    d = bf16_ulp_distance(got.cpu(), want)
    atol = want.float().pow(2).mean().sqrt().item() * 2 ** -8
    return bool(((d <= 1) | ((got.cpu().float() - want.float()).abs() <= atol)).all())


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


# ---- 7. one block -------------------------------------------------------------------------------------------------------------------
def test_mxfp6_block_vs_mx6_oracle():
    """One real-shape block in steady state (Lk = 18720, roll + insert) against Mx6RefModel.  The bound (about twice the measured
    distance) must exclude the bf16 oracle and the MXFP8 oracle: Mx6RefModel's own distance to each is asserted above it."""
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
    m.set_quant("mxfp6")
    xs = x0.clone()
    kv = dict(k=k.clone(), v=v.clone(), global_end_index=S, local_end_index=S)
    ca = {"k": torch.zeros(1, 512, 12, 128, dtype=bf, device=DEV), "v": torch.zeros(1, 512, 12, 128, dtype=bf, device=DEV), "is_init": False}
    plan = m.block_forward(0, xs, e0, ctx, kv, ca, 3, (30, 52), current_start=S)
    _kv_commit(kv, plan.G_new, plan.E_new)
    m.set_quant(None)
    got = xs.cpu()
    sdc = {kk: vv.cpu() for kk, vv in sd.items()}
    outs = {}
    for name, cls in (("mx6", mx6_ref.Mx6RefModel), ("mx8", mx_ref.MXRefModel), ("bf16", RM.RefModel)):
        ref = cls(RM.RefConfig.from_cfg(cfg), sdc, frame_seqlen_for_max_attn=fs)
        ref.max_attention_size = S
        kvr = dict(k=k.cpu().clone(), v=v.cpu().clone(), global_end_index=S, local_end_index=S)
        car = dict(k=torch.zeros(1, 512, 12, 128, dtype=bf), v=torch.zeros(1, 512, 12, 128, dtype=bf), is_init=False)
        y, planr = ref.block(x0.cpu(), 0, e0.cpu(), (3, 30, 52), ctx.cpu(), kvr, car, S, False)
        outs[name] = (y, kvr, planr)
    r = rel_l2(got, outs["mx6"][0])
    o_bf, o_mx8 = rel_l2(outs["mx6"][0], outs["bf16"][0]), rel_l2(outs["mx6"][0], outs["mx8"][0])
    bound = BLOCK_BOUND
    print(f"mxfp6 block: vs Mx6RefModel relL2 {r:.2e} (cos {cosine(got, outs['mx6'][0]):.6f}); vs bf16 oracle "
          f"{rel_l2(got, outs['bf16'][0]):.2e}, vs MXFP8 oracle {rel_l2(got, outs['mx8'][0]):.2e}; Mx6RefModel vs bf16 oracle {o_bf:.2e}, "
          f"vs MXFP8 oracle {o_mx8:.2e}; bound {bound:.2e}")
    assert o_bf > bound and o_mx8 > bound, (o_bf, o_mx8, bound)
    assert r < bound, r
    kvr, planr = outs["mx6"][1], outs["mx6"][2]
    assert (kv["global_end_index"], kv["local_end_index"]) == (planr["G_new"], planr["E_new"])
    sl = torch.linspace(0, S - 1, 64).round().long()
    gk, gv = kv["k"].cpu(), kv["v"].cpu()
    assert rel_l2(gk[0, sl], kvr["k"][0, sl]) < 5e-3 and rel_l2(gv[0, sl], kvr["v"][0, sl]) < 5e-3


# ---- 8. 30 layers ------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not _have("real_fwd.pt"), reason="golden missing")
def test_mxfp6_steady_state_vs_reference(real30):
    rec = load_golden("real_fwd.pt")
    cfg, gen = real30
    S = 12 * cfg.frame_seqlen
    prompt = {"prompt_embeds": synth.synth_prompt_embeds(cfg, seed=1, device=DEV)}
    noise = synth.synth_noise(cfg, 3, seed=0, device=DEV)
    outs = {}
    for mode in ("mxfp8", "mxfp6"):
        gen.model.set_quant(mode)
        kv, ca = _new_caches(30, S)
        for i in range(30):
            kv[i]["k"], kv[i]["v"] = _kv_fill(cfg, i, S)
            kv[i]["global_end_index"] = S; kv[i]["local_end_index"] = S
        flow, _ = gen(noise, prompt, torch.full((1, 3), 625.0, device=DEV), kv_cache=kv, crossattn_cache=ca, current_start=S)
        outs[mode] = flow.cpu()
        assert (kv[0]["global_end_index"], kv[0]["local_end_index"]) == tuple(rec["idx_steady"])
    gen.model.set_quant(None)
    r, c = rel_l2(outs["mxfp6"], rec["flow_steady"]), cosine(outs["mxfp6"], rec["flow_steady"])
    r8 = rel_l2(outs["mxfp6"], outs["mxfp8"])
    print(f"mxfp6 steady: vs reference bf16 {r:.2e} (cos {c:.6f}); vs the mxfp8 run {r8:.2e}")
    assert r < 2 * MEASURED["steady_ref"] and c > 0.99, (r, c)
    assert r8 > 1e-3, r8


@pytest.mark.skipif(not _have("config2_pipe.pt"), reason="golden missing")
def test_config2_mxfp6_free_running_vs_reference_bf16(real30):
    """Config 2's 21 frames free-running: per block within about twice the measured distance to the reference's bf16 latents, flat
    along the stream (last block <= 1.25x the first), and different from the same run in mxfp8 in every block."""
    cfg, gen = real30
    lats = {}
    try:
        for mode in ("mxfp8", "mxfp6"):
            gen.model.set_quant(mode)
            rec, P, lat, spy = _config2_run(real30, teacher=False, check=False)
            lats[mode] = lat.cpu()
    finally:
        gen.model.set_quant(None)
    rs = []
    for blk in range(7):
        sl = slice(3 * blk, 3 * blk + 3)
        a, b = lats["mxfp6"][:, sl], rec["latents"][:, sl]
        r, c, r8 = rel_l2(a, b), cosine(a, b), rel_l2(a, lats["mxfp8"][:, sl])
        rs.append(r)
        print(f"config 2 mxfp6 free-running: block {blk} vs reference bf16 relL2 {r:.2e} cos {c:.6f}; vs mxfp8 run {r8:.2e}")
        assert r < 2 * MEASURED["config2"] and c > 0.99, (blk, r, c)
        assert r8 > 1e-3, (blk, r8)
    assert rs[-1] < 1.25 * rs[0], rs


# ---- 9. with MX self-attention -----------------------------------------------------------------------------------------------
def test_mxfp6_with_mx_attention_toy_vs_oracle():
    """set_quant("mxfp6") + set_attn_quant("mxfp8") on the toy model over fill, roll and the next frames, against a host model with
    Mx6RefModel's linears and tests/mx_attn_ref.py's attention; it must sit closer to that oracle than to the one with bf16 linears."""
    import mx_attn_ref as MA
    from oracle import ref_model as RM
    from test_mx_attn_gpu import _toy, _toy_caches

    class Mx6MXAttnRef(MA.MXAttnRefModel):
        def __init__(self, *a, m6=True, **kw):
            super().__init__(*a, mx_linears=False, **kw)
            self.m6, self._w6 = m6, {}

        def lin(self, x, name):
            if self.m6 and name.startswith("blocks.") and name.endswith(self._W8A8):
                if name not in self._w6:
                    self._w6[name] = mx6_ref.dequantize(*mx6_ref.quantize(self.sd[name + ".weight"]))
                acc = mx6_ref.mx6_matmul(x.to(self.dtype), self._w6[name]).float()
                return (acc + self.sd[name + ".bias"].float()).to(self.dtype).reshape(*x.shape[:-1], -1)
            return RM.RefModel.lin(self, x, name)

    cfg, sd, gen, S = _toy("mxfp8", "mxfp6")
    fs = cfg.frame_seqlen
    kv, ca = _toy_caches(cfg, S, DEV)
    noise = synth.synth_noise(cfg, 5, seed=5)
    prompt = synth.synth_prompt_embeds(cfg, seed=7, valid_tokens=9)
    oracles = {}
    for name, m6 in (("mx6", True), ("bf16", False)):
        om = Mx6MXAttnRef(RM.RefConfig.from_cfg(cfg), sd, frame_seqlen_for_max_attn=fs, m6=m6)
        oracles[name] = (RM.RefGenerator(om, 5.0), RM.new_kv_cache(1, S, cfg.num_layers, cfg.num_heads, 128),
                         RM.new_crossattn_cache(1, cfg.text_len, cfg.num_layers, cfg.num_heads, 128))
    worst = {"mx6": 0.0, "bf16": 0.0}
    for f in range(5):                       # fill, then rolls
        x = noise[:, f:f + 1]
        t = torch.full((1, 1), 937.5)
        _, x0 = gen(x.to(DEV), {"prompt_embeds": prompt.to(DEV)}, t.to(DEV), kv_cache=kv, crossattn_cache=ca, current_start=f * fs)
        for name, (og, okv, oca) in oracles.items():
            _, r0 = og(x, prompt, t, okv, oca, f * fs)
            worst[name] = max(worst[name], rel_l2(x0.cpu(), r0))
    gen.model.set_quant(None).set_attn_quant(None)
    bound = 2 * MEASURED["toy_attn"]
    print(f"mxfp6 + MX attention, toy: worst x0 rel-L2 vs the MXFP6 + MX-attention oracle {worst['mx6']:.2e}, vs the bf16-linear "
          f"one {worst['bf16']:.2e}; bound {bound:.2e}")
    assert worst["mx6"] < bound, worst
    assert worst["mx6"] < worst["bf16"], worst
