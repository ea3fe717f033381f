"""FP8 rowwise block linears on the MI355X (e4m3fn codes, per-token / per-output-channel fp32 scales, v_mfma_scale_f32_16x16x128_f8f6f4
at unit block scales on the W8A8 kernels' structure), pinned to the scheme's definition (tests/fp8_ref.py): quantiser and producer
bytes, every epilogue and kernel instance with exact data, random data against the fp64 product (a bound the int8 and bf16 GEMMs
fail), outliers against int8, one real-shape block against Fp8RefModel, the 30-layer steady state and config 2 free-running against
the reference's bf16 goldens, and the mode beside MX self-attention."""
import pytest
import torch

import fp8_ref
from conftest import load_golden
from longlive_amd import synth
from quant_exact import epi_tail as _epi_ref
from quant_exact import exact_operands as _exact_operands
from quant_exact import hard_x_f8 as _hard_x
from test_shipped_sizes_gpu import _config2_run, _have, _kv_fill, _new_caches, real30  # noqa: F401  (real30: module fixture)
from util import assert_bf16_close, bf, bf16_ulp_distance, cosine, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
U8 = torch.uint8

# measured on one MI355X; the model-level bounds are about twice these.  The block's is 1.8x: twice would reach
# Fp8RefModel's own 9.0e-3 distance to the bf16 oracle, and the band must exclude that oracle.
MEASURED = dict(block=4.7e-3, steady_ref=4.9e-2, config2=3.4e-2, toy_attn=2.3e-3)
BLOCK_BOUND = 8.5e-3


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
def _within_1ulp(got, want):
    d = bf16_ulp_distance(got.cpu(), want)
    atol = want.float().pow(2).mean().sqrt().item() * 2 ** -8
    return bool(((d <= 1) | ((got.cpu().float() - want.float()).abs() <= atol)).all())


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


# ---- 6. one real-shape block ---------------------------------------------------------------------------------------------------
def test_fp8_rowwise_block_vs_fp8_oracle():
    """One real-shape block in steady state (Lk = 18720, roll + insert) against Fp8RefModel.  The bound (about twice the measured
    distance) must exclude the bf16 oracle and the int8 oracle: Fp8RefModel's own distance to each is asserted above it."""
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
    m.set_quant("fp8_rowwise")
    xs = x0.clone()
    kv = dict(k=k.clone(), v=v.clone(), global_end_index=S, local_end_index=S)
    ca = {"k": torch.zeros(1, 512, 12, 128, dtype=bf, device=DEV), "v": torch.zeros(1, 512, 12, 128, dtype=bf, device=DEV), "is_init": False}
    plan = m.block_forward(0, xs, e0, ctx, kv, ca, 3, (30, 52), current_start=S)
    _kv_commit(kv, plan.G_new, plan.E_new)
    m.set_quant(None)
    got = xs.cpu()
    sdc = {kk: vv.cpu() for kk, vv in sd.items()}
    outs = {}
    for name, make in (("fp8", lambda c: fp8_ref.Fp8RefModel(c, sdc, frame_seqlen_for_max_attn=fs)),
                       ("bf16", lambda c: RM.RefModel(c, sdc, frame_seqlen_for_max_attn=fs)),
                       ("int8", lambda c: RM.RefModel(c, sdc, frame_seqlen_for_max_attn=fs, quant="int8"))):
        ref = make(RM.RefConfig.from_cfg(cfg))
        ref.max_attention_size = S
        kvr = dict(k=k.cpu().clone(), v=v.cpu().clone(), global_end_index=S, local_end_index=S)
        car = dict(k=torch.zeros(1, 512, 12, 128, dtype=bf), v=torch.zeros(1, 512, 12, 128, dtype=bf), is_init=False)
        y, planr = ref.block(x0.cpu(), 0, e0.cpu(), (3, 30, 52), ctx.cpu(), kvr, car, S, False)
        outs[name] = (y, kvr, planr)
    r = rel_l2(got, outs["fp8"][0])
    o_bf, o_i8 = rel_l2(outs["fp8"][0], outs["bf16"][0]), rel_l2(outs["fp8"][0], outs["int8"][0])
    bound = BLOCK_BOUND
    print(f"fp8_rowwise block: vs Fp8RefModel relL2 {r:.2e} (cos {cosine(got, outs['fp8'][0]):.6f}); vs bf16 oracle "
          f"{rel_l2(got, outs['bf16'][0]):.2e}, vs int8 oracle {rel_l2(got, outs['int8'][0]):.2e}; Fp8RefModel vs bf16 oracle {o_bf:.2e}, "
          f"vs int8 oracle {o_i8:.2e}; bound {bound:.2e}")
    assert o_bf > bound and o_i8 > bound, (o_bf, o_i8, bound)
    assert r < bound, r
    kvr, planr = outs["fp8"][1], outs["fp8"][2]
    assert (kv["global_end_index"], kv["local_end_index"]) == (planr["G_new"], planr["E_new"])
    sl = torch.linspace(0, S - 1, 64).round().long()
    gk, gv = kv["k"].cpu(), kv["v"].cpu()
    assert rel_l2(gk[0, sl], kvr["k"][0, sl]) < 5e-3 and rel_l2(gv[0, sl], kvr["v"][0, sl]) < 5e-3


# ---- 7. 30 layers ------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not _have("real_fwd.pt"), reason="golden missing")
def test_fp8_rowwise_steady_state_vs_reference(real30):
    rec = load_golden("real_fwd.pt")
    cfg, gen = real30
    S = 12 * cfg.frame_seqlen
    prompt = {"prompt_embeds": synth.synth_prompt_embeds(cfg, seed=1, device=DEV)}
    noise = synth.synth_noise(cfg, 3, seed=0, device=DEV)
    outs = {}
    for mode in ("int8", "fp8_rowwise"):
        gen.model.set_quant(mode)
        kv, ca = _new_caches(30, S)
        for i in range(30):
            kv[i]["k"], kv[i]["v"] = _kv_fill(cfg, i, S)
            kv[i]["global_end_index"] = S; kv[i]["local_end_index"] = S
        flow, _ = gen(noise, prompt, torch.full((1, 3), 625.0, device=DEV), kv_cache=kv, crossattn_cache=ca, current_start=S)
        outs[mode] = flow.cpu()
        assert (kv[0]["global_end_index"], kv[0]["local_end_index"]) == tuple(rec["idx_steady"])
    gen.model.set_quant(None)
    r, c = rel_l2(outs["fp8_rowwise"], rec["flow_steady"]), cosine(outs["fp8_rowwise"], rec["flow_steady"])
    r_i8 = rel_l2(outs["fp8_rowwise"], outs["int8"])
    print(f"fp8_rowwise steady: vs reference bf16 {r:.2e} (cos {c:.6f}); vs the int8 run {r_i8:.2e}")
    assert r < 2 * MEASURED["steady_ref"] and c > 0.995, (r, c)
    assert r_i8 > 1e-3, r_i8


@pytest.mark.skipif(not _have("config2_pipe.pt"), reason="golden missing")
def test_config2_fp8_rowwise_free_running_vs_reference_bf16(real30):
    """Config 2's 21 frames free-running: per block within about twice the measured distance to the reference's bf16 latents, flat
    along the stream (last block <= 1.25x the first), and different from the same run in int8 in every block."""
    cfg, gen = real30
    lats = {}
    try:
        for mode in ("int8", "fp8_rowwise"):
            gen.model.set_quant(mode)
            rec, P, lat, spy = _config2_run(real30, teacher=False, check=False)
            lats[mode] = lat.cpu()
    finally:
        gen.model.set_quant(None)
    rs = []
    for blk in range(7):
        sl = slice(3 * blk, 3 * blk + 3)
        a, b = lats["fp8_rowwise"][:, sl], rec["latents"][:, sl]
        r, c, r_i8 = rel_l2(a, b), cosine(a, b), rel_l2(a, lats["int8"][:, sl])
        rs.append(r)
        print(f"config 2 fp8_rowwise free-running: block {blk} vs reference bf16 relL2 {r:.2e} cos {c:.6f}; vs int8 run {r_i8:.2e}")
        assert r < 2 * MEASURED["config2"] and c > 0.995, (blk, r, c)
        assert r_i8 > 1e-3, (blk, r_i8)
    assert rs[-1] < 1.25 * rs[0], rs


# ---- 8. with MX self-attention -----------------------------------------------------------------------------------------------
def test_fp8_rowwise_with_mx_attention_toy_vs_oracle():
    """set_quant("fp8_rowwise") + set_attn_quant("mxfp8") on the toy model over fill, roll and the next frames, against a host model
    with Fp8RefModel's linears and tests/mx_attn_ref.py's attention; it must sit closer to that oracle than to the one with bf16
    linears."""
    import mx_attn_ref as MA
    from oracle import ref_model as RM
    from test_mx_attn_gpu import _toy, _toy_caches

    class F8MXAttnRef(MA.MXAttnRefModel):
        def __init__(self, *a, f8=True, **kw):
            super().__init__(*a, mx_linears=False, **kw)
            self.f8, self._wf8 = f8, {}

        def lin(self, x, name):
            if self.f8 and name.startswith("blocks.") and name.endswith(self._W8A8):
                if name not in self._wf8:
                    self._wf8[name] = fp8_ref.quantize(self.sd[name + ".weight"])
                y = fp8_ref.f8_linear(x.to(self.dtype).reshape(-1, x.shape[-1]), *self._wf8[name], self.sd[name + ".bias"])
                return y.to(self.dtype).reshape(*x.shape[:-1], -1)
            return RM.RefModel.lin(self, x, name)

    cfg, sd, gen, S = _toy("mxfp8", "fp8_rowwise")
    fs = cfg.frame_seqlen
    kv, ca = _toy_caches(cfg, S, DEV)
    noise = synth.synth_noise(cfg, 5, seed=5)
    prompt = synth.synth_prompt_embeds(cfg, seed=7, valid_tokens=9)
    oracles = {}
    for name, f8 in (("fp8", True), ("bf16", False)):
        om = F8MXAttnRef(RM.RefConfig.from_cfg(cfg), sd, frame_seqlen_for_max_attn=fs, f8=f8)
        oracles[name] = (RM.RefGenerator(om, 5.0), RM.new_kv_cache(1, S, cfg.num_layers, cfg.num_heads, 128),
                         RM.new_crossattn_cache(1, cfg.text_len, cfg.num_layers, cfg.num_heads, 128))
    worst = {"fp8": 0.0, "bf16": 0.0}
    for f in range(5):                       # fill, then rolls
        x = noise[:, f:f + 1]
        t = torch.full((1, 1), 937.5)
        _, x0 = gen(x.to(DEV), {"prompt_embeds": prompt.to(DEV)}, t.to(DEV), kv_cache=kv, crossattn_cache=ca, current_start=f * fs)
        for name, (og, okv, oca) in oracles.items():
            _, r0 = og(x, prompt, t, okv, oca, f * fs)
            worst[name] = max(worst[name], rel_l2(x0.cpu(), r0))
    gen.model.set_quant(None).set_attn_quant(None)
    bound = 2 * MEASURED["toy_attn"]
    print(f"fp8_rowwise + MX attention, toy: worst x0 rel-L2 vs the FP8 + MX-attention oracle {worst['fp8']:.2e}, vs the bf16-linear "
          f"one {worst['bf16']:.2e}; bound {bound:.2e}")
    assert worst["fp8"] < bound, worst
    assert worst["fp8"] < worst["bf16"], worst
