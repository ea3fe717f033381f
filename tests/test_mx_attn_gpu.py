"""MXFP8 self-attention on the MI355X (flash_attn_mx_kernel, kv_shadow_mx_kernel: v_mfma_scale_f32_32x32x64_f8f6f4), pinned to the
scheme's restatement (tests/mx_attn_ref.py): shadow bytes bit for bit after an unaligned insert, a roll and an outside zero_; both
products' lane maps with exact data; the kernel against the restatement on the production grid and its neighbours, with a bound that
the bf16 kernel fails; the model with and without MX linears against the oracle and the reference's goldens; the switch back to bf16.
The tile, range, row and stride edges of both kernels are pinned bit for bit by tests/test_mx_attn_edges_gpu.py."""
import math

import pytest
import torch

import mx_attn_ref as MA
from conftest import load_golden
from longlive_amd import synth
from model_runs import config2_run as _config2_run
from model_runs import have as _have
from model_runs import kv_fill as _kv_fill
from model_runs import new_caches as _new_caches
from model_runs import real30  # noqa: F401  (module fixture)
from model_runs import toy as _toy
from model_runs import toy_caches as _toy_caches
from quant_exact import unit_c_scale as _unit_c_scale
from quant_ref import make_ref
from util import bf, cosine, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
U8 = torch.uint8

# kernel vs restatement (bf16 outputs of both): fp32 summation order, v_exp_f32's ulp and the rare P^ rounding it flips
KERNEL_BOUND = 3e-3      # measured 1.5e-3 .. 1.9e-3; ll_flash_attn's bf16 output: 5.4e-2 .. 8.9e-2


@pytest.fixture(scope="module")
def ops():
    from longlive_amd import ops as O
    return O


def _cache(S, H=12, B=1, seed=5, kscale=1.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    k = (kscale * torch.randn(B, S, H, 128, generator=g, device=DEV)).to(bf)
    v = (0.5 * torch.randn(B, S, H, 128, generator=g, device=DEV)).to(bf)
    return k, v


def _check_shadow(sh, k, v):
    kq, ks = MA.shadow_k(k)
    vq, vs = MA.shadow_v(v)
    assert torch.equal(sh["ks"].cpu(), ks.cpu()), "K scales"
    assert torch.equal(sh["kq"].view(U8).cpu(), kq.view(U8).cpu()), "K codes"
    assert torch.equal(sh["vs"].cpu(), vs.cpu()), "V scales"
    assert torch.equal(sh["vq"].view(U8).cpu(), vq.view(U8).cpu()), "V codes"


def test_shadow_bytes_after_unaligned_insert_and_roll(ops):
    S = 18720
    k, v = _cache(S)
    sh = ops.kv_shadow_mx_alloc(k)
    ops.kv_shadow_mx(k, v, sh, 0, S)
    _check_shadow(sh, k, v)
    k2, v2 = _cache(4680, seed=9)
    k[:, 4680:9360] = k2                         # both ends unaligned (4680 = 146 x 32 + 8)
    v[:, 4680:9360] = v2
    ops.kv_shadow_mx(k, v, sh, 4680, 9360)
    _check_shadow(sh, k, v)
    ops.kv_roll(k, v, 4680, 9360, 4680)          # the steady-state roll: dst = sink, src = sink + evict
    ops.kv_shadow_mx(k, v, sh, 4680, 9360)
    _check_shadow(sh, k, v)
    # S not a multiple of 32: the padding slots of the last block read as 0
    k3, v3 = _cache(4690, H=2, B=2, seed=3)
    sh3 = ops.kv_shadow_mx_alloc(k3)
    ops.kv_shadow_mx(k3, v3, sh3, 0, 4690)
    _check_shadow(sh3, k3, v3)


def test_lane_maps_with_exact_data(ops):
    """Sparse integer q / k with a distinct power-of-two factor per (row, 32-channel block) on both sides (so per-block scales differ
    by row and block), integer scores, c = 1 (P = 2^integer, exactly representable), and V values that quantise exactly with scales
    differing per (channel, 32-slot block).  A wrong operand map, a scale from the wrong lane or byte, or V^ blocks out of order change
    the result by O(1); the kernel must agree with the restatement to fp32 summation order."""
    B, H, Lq, S = 1, 2, 96, 300
    g = torch.Generator().manual_seed(11)

    def sparse(rows, lo, hi):
        z = torch.randint(-1, 2, (rows, H, 128), generator=g) * (torch.rand(rows, H, 128, generator=g) < 0.08)
        f = 2.0 ** torch.randint(lo, hi, (rows, H, 4, 1), generator=g)
        return (z.reshape(rows, H, 4, 32) * f).reshape(1, rows, H, 128)

    q = sparse(Lq, -1, 1)
    k = sparse(S, 1, 3)
    w = torch.randint(-3, 4, (S, H, 128), generator=g).float()
    vf = 2.0 ** torch.randint(-1, 2, ((S + 31) // 32, 1, H, 128), generator=g)
    v = (w.reshape(-1, 1, H, 128)[: S] * vf.repeat_interleave(32, 0)[:S].reshape(S, 1, H, 128)).reshape(1, S, H, 128)
    q, k, v = q.to(bf), k.to(bf), v.to(bf)
    assert torch.equal(q.float(), q.to(bf).float())
    scale = _unit_c_scale()
    segs = [(0, 100), (164, 300)]
    kd, vd = k.to(DEV), v.to(DEV)
    sh = ops.kv_shadow_mx_alloc(kd)
    ops.kv_shadow_mx(kd, vd, sh, 0, S)
    got = ops.flash_attn_mx(q.to(DEV), sh, segs, scale=scale).float().cpu()
    want = MA.mx_attention_cache(q, k, v, segs, scale=scale, dtype=torch.float64)
    r = rel_l2(got, want.to(bf).float())
    print(f"exact-data lane map: relL2 {r:.2e}, max |diff| to the unrounded fp64 value {(got - want).abs().max().item():.2e}")
    assert torch.equal(got, want.to(bf).float()), r       # every sum is exact: the bf16 outputs are the same bits


def _restated(q, k, v, segs):
    return MA.mx_attention_cache(q, k, v, segs).to(bf).float()


CASES = {
    "production": dict(B=1, Lq=4680, S=18720, segs=[(0, 4680), (4680, 18720)]),
    "filling": dict(B=1, Lq=4680, S=18720, segs=[(0, 4680), (4680, 9360)]),
    "unaligned": dict(B=1, Lq=4680, S=18720, segs=[(0, 4680), (6240, 18720)]),
    "recache": dict(B=1, Lq=18720, S=18720, segs=[(0, 18720)]),
    "batch2": dict(B=2, Lq=1560, S=6240, segs=[(0, 1560), (3120, 6240)]),
    "peaked": dict(B=1, Lq=4680, S=18720, segs=[(0, 4680), (4680, 18720)], peak=True),
}


@pytest.mark.parametrize("case", list(CASES))
def test_kernel_vs_restatement_and_not_bf16(ops, case):
    cfg = CASES[case]
    B, Lq, S, segs = cfg["B"], cfg["Lq"], cfg["S"], cfg["segs"]
    k, v = _cache(S, B=B, seed=len(case))
    g = torch.Generator(device=DEV).manual_seed(17)
    q = torch.randn(B, Lq, 12, 128, generator=g, device=DEV).to(bf)
    if cfg.get("peak"):           # every query's maximum lies in the last 4680 keys, growing towards the end: late lazy rescales
        ramp = torch.linspace(1.0, 3.0, 4680, device=DEV).view(1, -1, 1, 1)
        k[:, S - 4680:] = (k[:, S - 4680:].float() * ramp).to(bf)
        k[:, S - 4680:] += (0.25 * q[:, :1].float() * ramp).to(bf)
    sh = ops.kv_shadow_mx_alloc(k)
    ops.kv_shadow_mx(k, v, sh, 0, S)
    got = ops.flash_attn_mx(q, sh, segs).float()
    want = _restated(q, k, v, segs)
    bf16 = ops.flash_attn(q, k, v, segs).float()
    r, r_bf = rel_l2(got, want), rel_l2(bf16, want)
    print(f"{case}: flash_attn_mx vs restatement relL2 {r:.2e}; ll_flash_attn (bf16) vs restatement {r_bf:.2e}; "
          f"plan: {ops.flash_attn_mx_plan(Lq, 12, B, segs)}")
    assert r < KERNEL_BOUND, r
    assert r_bf > KERNEL_BOUND, r_bf


def test_no_nan_when_a_tile_is_mostly_masked(ops):
    """A range of one slot (tile of 64 with 63 masked keys) and a range starting on the last slot of a 32-block."""
    k, v = _cache(700, H=3, seed=2)
    q = torch.randn(1, 33, 3, 128, device=DEV).to(bf)
    sh = ops.kv_shadow_mx_alloc(k)
    ops.kv_shadow_mx(k, v, sh, 0, 700)
    for segs in ([(5, 6)], [(31, 33), (699, 700)]):
        got = ops.flash_attn_mx(q, sh, segs).float()
        assert torch.isfinite(got).all()
        assert rel_l2(got, _restated(q, k, v, segs)) < KERNEL_BOUND


# ---- model level ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lin", [None, "mxfp8"])
def test_block_vs_mx_attention_oracle(lin):
    """One real-shape block in steady state (Lk = 18720, roll + insert) with MX attention (and bf16 or MX linears) against
    MXAttnRefModel; it must sit closer to it than to the oracle without MX attention."""
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
    m.set_quant(lin).set_attn_quant("mxfp8")
    xs = x0.clone()
    kv = dict(k=k.clone(), v=v.clone(), global_end_index=S, local_end_index=S)
    ca = {"k": torch.zeros(1, 512, 12, 128, dtype=bf, device=DEV), "v": torch.zeros(1, 512, 12, 128, dtype=bf, device=DEV), "is_init": False}
    plan = m.block_forward(0, xs, e0, ctx, kv, ca, 3, (30, 52), current_start=S)
    _kv_commit(kv, plan.G_new, plan.E_new)
    got = xs.cpu()
    _check_shadow(kv["_ll_mx"], kv["k"], kv["v"])
    sdc = {kk: vv.cpu() for kk, vv in sd.items()}
    outs = {}
    refs = (("mxattn", lambda *a, **kw: MA.MXAttnRefModel(*a, linears=lin, **kw)),
            ("plain", lambda *a, **kw: make_ref(lin, *a, **kw)))
    for name, cls in refs:
        ref = cls(RM.RefConfig.from_cfg(cfg), sdc, frame_seqlen_for_max_attn=fs)
        ref.max_attention_size = S
        kvr = dict(k=k.cpu().clone(), v=v.cpu().clone(), global_end_index=S, local_end_index=S)
        car = dict(k=torch.zeros(1, 512, 12, 128, dtype=bf), v=torch.zeros(1, 512, 12, 128, dtype=bf), is_init=False)
        y, _ = ref.block(x0.cpu(), 0, e0.cpu(), (3, 30, 52), ctx.cpu(), kvr, car, S, False)
        outs[name] = y
    # the block's update (output - input): the residual stream itself hides most of the attention's share
    x0c = x0.cpu().float()
    r_mx, r_plain = rel_l2(got.float() - x0c, outs["mxattn"].float() - x0c), rel_l2(got.float() - x0c, outs["plain"].float() - x0c)
    print(f"block (linears {lin}) with MX attention, update vs MX-attention oracle relL2 {r_mx:.2e}; vs the oracle without it "
          f"{r_plain:.2e}; oracles apart {rel_l2(outs['mxattn'].float() - x0c, outs['plain'].float() - x0c):.2e}; "
          f"output relL2 {rel_l2(got, outs['mxattn']):.2e}")
    assert r_mx < r_plain, (r_mx, r_plain)
    assert rel_l2(got, outs["mxattn"]) < 6e-3 and cosine(got, outs["mxattn"]) > 0.9999


@pytest.mark.skipif(not _have("real_fwd.pt"), reason="golden missing")
@pytest.mark.parametrize("lin", [None, "mxfp8"])
def test_steady_state_30_layers_vs_reference(real30, lin):
    """30 layers, steady state (roll + insert, Lk = 18720) with MX attention, against the reference's bf16 golden and against our
    path without MX attention (which it must differ from: the mode is on)."""
    rec = load_golden("real_fwd.pt")
    cfg, gen = real30
    S = 12 * cfg.frame_seqlen
    prompt = {"prompt_embeds": synth.synth_prompt_embeds(cfg, seed=1, device=DEV)}
    noise = synth.synth_noise(cfg, 3, seed=0, device=DEV)
    outs = {}
    gen.model.set_quant(lin)
    try:
        for amode in (None, "mxfp8"):
            gen.model.set_attn_quant(amode)
            kv, ca = _new_caches(30, S)
            for i in range(30):
                kv[i]["k"], kv[i]["v"] = _kv_fill(cfg, i, S)
                kv[i]["global_end_index"] = S; kv[i]["local_end_index"] = S
            flow, _ = gen(noise, prompt, torch.full((1, 3), 625.0, device=DEV), kv_cache=kv, crossattn_cache=ca, current_start=S)
            outs[amode] = flow.cpu()
            assert (kv[0]["global_end_index"], kv[0]["local_end_index"]) == tuple(rec["idx_steady"])
    finally:
        gen.model.set_quant(None)
        gen.model.set_attn_quant(None)
    r_ref, r_off = rel_l2(outs["mxfp8"], rec["flow_steady"]), rel_l2(outs["mxfp8"], outs[None])
    c_ref = cosine(outs["mxfp8"], rec["flow_steady"])
    print(f"steady 30 layers, linears {lin}, MX attention: vs reference bf16 {r_ref:.2e} (cos {c_ref:.6f}); vs same linears without "
          f"MX attention {r_off:.2e}")
    assert r_ref < 7e-2 and c_ref > 0.997
    assert r_off > 1e-3, r_off


# config 2 free-running, per block vs the reference's bf16 latents: measured 8.3e-3 (bf16 linears) and 3.50e-2 .. 3.55e-2 (MX linears)
CONFIG2_BOUND = {None: 1.7e-2, "mxfp8": 7e-2}


@pytest.mark.skipif(not _have("config2_pipe.pt"), reason="golden missing")
@pytest.mark.parametrize("lin", [None, "mxfp8"])
def test_config2_free_running_vs_reference_bf16(real30, lin):
    """Config 2's 21 frames with MX attention, free-running, against the reference's bf16 latents: per block within about twice the
    measured rel-L2 and no growth along the stream (the last block within 1.25x of the first).  The same run with bf16 attention
    must differ from it in every block (the mode is on)."""
    cfg, gen = real30
    gen.model.set_quant(lin)
    lats = {}
    try:
        for amode in ("mxfp8", None):
            gen.model.set_attn_quant(amode)
            rec, P, lat, spy = _config2_run(real30, teacher=False, check=False)
            lats[amode] = lat.cpu()
    finally:
        gen.model.set_quant(None)
        gen.model.set_attn_quant(None)
    rs = []
    for blk in range(7):
        sl = slice(3 * blk, 3 * blk + 3)
        a, b, off = lats["mxfp8"][:, sl], rec["latents"][:, sl], lats[None][:, sl]
        r, c, r_off = rel_l2(a, b), cosine(a, b), rel_l2(a, off)
        rs.append(r)
        print(f"config 2 (linears {lin}) MX attention free-running: block {blk} vs reference bf16: relL2 {r:.2e} cos {c:.6f}; "
              f"vs bf16 attention {r_off:.2e}")
        assert r < CONFIG2_BOUND[lin] and c > 0.997, (blk, r, c)
        assert r_off > 1e-3, (blk, r_off)
    assert rs[-1] < 1.25 * rs[0], rs


def _interactive_run(lin, attn):
    """Fill + roll, then the interactive pipelines' global_sink=False switch: k / v zeroed in place outside the model, one recache
    forward (sink_recache_after_switch) and the next frame, against MXAttnRefModel (with the same linears) doing the same.  Returns
    the worst rel-L2 of x0 over the forwards; checks the shadow bytes after the zero_ + recache when MX attention is on."""
    from oracle import ref_model as RM
    cfg, sd, gen, S = _toy(attn, lin)
    fs = cfg.frame_seqlen
    kv, ca = _toy_caches(cfg, S, DEV)
    om = MA.MXAttnRefModel(RM.RefConfig.from_cfg(cfg), sd, frame_seqlen_for_max_attn=fs, linears=lin)
    og = RM.RefGenerator(om, 5.0)
    okv = RM.new_kv_cache(1, S, cfg.num_layers, cfg.num_heads, 128)
    oca = RM.new_crossattn_cache(1, cfg.text_len, cfg.num_layers, cfg.num_heads, 128)
    noise = synth.synth_noise(cfg, 6, seed=5)
    prompts = [synth.synth_prompt_embeds(cfg, seed=s, valid_tokens=9) for s in (7, 8)]
    worst = 0.0

    def step(f, prompt, recache=False):
        nonlocal worst
        x = noise[:, f:f + 1]
        t = torch.full((1, 1), 0.0 if recache else 937.5)
        _, x0 = gen(x.to(DEV), {"prompt_embeds": prompt.to(DEV)}, t.to(DEV), kv_cache=kv, crossattn_cache=ca, current_start=f * fs,
                    sink_recache_after_switch=recache)
        _, r0 = og(x, prompt, t, okv, oca, f * fs, sink_recache_after_switch=recache)
        worst = max(worst, rel_l2(x0.cpu(), r0))
        assert (kv[0]["global_end_index"], kv[0]["local_end_index"]) == (okv[0]["global_end_index"], okv[0]["local_end_index"])

    for f in range(4):                       # fill, then a roll
        step(f, prompts[0])
    for blk in kv:                           # the switch: outside in-place zero_ (bumps the version counters)
        blk["k"].zero_(); blk["v"].zero_()
    for blk in okv:
        blk["k"].zero_(); blk["v"].zero_()
    for blk in ca:
        blk["is_init"] = False
    for blk in oca:
        blk["is_init"] = False
    step(3, prompts[1], recache=True)        # recompute of the last frame under the new prompt
    if attn == "mxfp8":
        for blk in kv:
            _check_shadow(blk["_ll_mx"], blk["k"], blk["v"])
    step(4, prompts[1])
    return worst


# worst x0 rel-L2 to MXAttnRefModel over the interactive sequence (toy model), measured with MX attention; the bound is twice that.
# The same sequence with bf16 attention measured 2.30e-3 / 2.81e-3 against that oracle: in the toy model the attention's
# quantisation is a small share of x0, so what tells the modes apart is that the MX run sits closer to the oracle than it.
INTERACTIVE_MEASURED = {None: 1.66e-3, "mxfp8": 2.35e-3}


@pytest.mark.parametrize("lin", [None, "mxfp8"])
def test_interactive_switch_external_zero_vs_oracle(lin):
    worst = _interactive_run(lin, "mxfp8")
    worst_off = _interactive_run(lin, None)
    bound = 2 * INTERACTIVE_MEASURED[lin]
    print(f"interactive switch (linears {lin}): worst rel-L2 vs MX-attention oracle {worst:.2e} with MX attention, {worst_off:.2e} "
          f"with bf16 attention; bound {bound:.2e}")
    assert worst < bound, worst
    assert worst < worst_off, (worst, worst_off)


def test_toggle_back_to_bf16_is_bit_identical_and_launches_nothing_mx():
    from longlive_amd import ops as O
    outs = {}
    for name, modes in (("never", [None, None, None]), ("toggled", ["mxfp8", None, None])):
        cfg, sd, gen, S = _toy(None)
        fs = cfg.frame_seqlen
        kv, ca = _toy_caches(cfg, S, DEV)
        noise = synth.synth_noise(cfg, 3, seed=5)
        prompt = synth.synth_prompt_embeds(cfg, seed=7, valid_tokens=9)
        res = []
        for f, mode in enumerate(modes):
            gen.model.set_attn_quant(mode)
            if f == 2:
                O.timer = O.KernelTimer()
            try:
                _, x0 = gen(noise[:, f:f + 1].to(DEV), {"prompt_embeds": prompt.to(DEV)}, torch.full((1, 1), 937.5, device=DEV),
                            kv_cache=kv, crossattn_cache=ca, current_start=f * fs)
                torch.cuda.synchronize()
                if f == 2:
                    tags = set(O.timer.records)
            finally:
                O.timer = None
            res.append(x0.cpu())
        outs[name] = (res, tags)
        if name == "toggled":
            assert all("_ll_mx" not in blk for blk in kv)
    # after the switch back no MX kernel runs (the first forward's MX output legitimately differs); a model switched on and off
    # before its first forward computes the never-switched model's bits
    assert not any("mx" in t for t in outs["toggled"][1]), outs["toggled"][1]
    assert any(t.startswith("flash_attn_self") for t in outs["toggled"][1])
    cfg, sd, gen, S = _toy(None)
    kv, ca = _toy_caches(cfg, S, DEV)
    gen.model.set_attn_quant("mxfp8")
    gen.model.set_attn_quant(None)
    noise = synth.synth_noise(cfg, 1, seed=5)
    prompt = synth.synth_prompt_embeds(cfg, seed=7, valid_tokens=9)
    _, x0 = gen(noise[:, :1].to(DEV), {"prompt_embeds": prompt.to(DEV)}, torch.full((1, 1), 937.5, device=DEV), kv_cache=kv,
                crossattn_cache=ca, current_start=0)
    assert torch.equal(x0.cpu(), outs["never"][0][0])
