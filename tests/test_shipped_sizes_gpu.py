"""Parity and invariants at the sizes that SHIP (BASELINE.json configs 1-5), through the C ABI on the MI355X.

  * attention on the two production launch grids -- Lq 4680 x Lk 18720 x 12 heads (228 workgroups) and the recache launch
    Lq = Lk = 18720 (888 workgroups): exact fp64 on sampled query rows that hit every (head, q-tile) workgroup, the
    XCD-aware placement on/off bit-identical, and every output element against the plain (non-pipelined) kernel;
  * config 1 ("G5"): the reference's CausalInferencePipeline at the real 1.3B shape, 4 latent frames, one step;
  * config 4's prompt-switch forward (reference `_recache_after_switch`) at the real shape, both global_sink settings;
  * one real-shape block against the reference's CausalWanAttentionBlock (tests/golden/real_block.pt);
  * full-length property runs of config 3 (240 latent frames) and config 5 (INT8).  (INT8 against its oracle, at steady state and
    through config 2 is tests/test_quant_model_gpu.py's "int8" row.)

Tolerances: attention max-abs <= 1.2e-2 vs fp64 (bf16 P and O, fp32 accumulation); end to end rel-L2 <= 3e-2 and cosine
>= 0.9995 per forward against the reference's bf16 CPU run; integer state exact."""
import math
import os

import pytest
import torch

from conftest import load_golden
from longlive_amd import synth
from model_runs import config2_run as _config2_run
from model_runs import have as _have
from model_runs import kv_fill as _kv_fill
from model_runs import new_caches as _new_caches
from model_runs import pipe_args as _pipe_args
from model_runs import real30  # noqa: F401  (module fixture)
import trace_driver as TD
from util import bf, cosine, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _tuning(key, value):
    from longlive_amd import _lib
    _lib.check(_lib.load().ll_set_tuning(key.encode(), int(value)), "ll_set_tuning")


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Lq", [4680, 18720])
def test_flash_attn_production_grids(Lq):
    from longlive_amd import ops
    H, Lk, D = 12, 18720, 128
    q = synth.hash_normal(201, f"q{Lq}", (1, Lq, H, D), device=DEV).to(bf)
    k = synth.hash_normal(202, "k", (1, Lk, H, D), device=DEV).to(bf)
    v = (0.7 * synth.hash_normal(203, "v", (1, Lk, H, D), device=DEV)).to(bf)
    from longlive_amd import _lib
    import ctypes as C
    buf = C.create_string_buffer(256)
    _lib.check(_lib.load().ll_flash_attn_plan(Lq, H, 1, Lk, 0, 1, buf, 256), "plan")
    assert b"flash_attn_asm_kernel" in buf.value, buf.value     # the shipped launch: one 4-wave workgroup per (head, q-tile) pair
    try:
        _tuning("attn_xcd", 1)
        got = ops.flash_attn(q, k, v, [(0, Lk)])                    # shipped: flash_attn_asm_kernel, 228 / 888 workgroups, XCD-aware placement
        _tuning("attn_xcd", 0)
        got0 = ops.flash_attn(q, k, v, [(0, Lk)])
        _tuning("attn_xcd", 1)
        _tuning("attn_asm", 0)                 # round 1-2's kernel: 8 waves x 32 rows, ping-pong wave groups
        pipe = ops.flash_attn(q, k, v, [(0, Lk)])
        _tuning("attn_xcd", 0)
        pipe0 = ops.flash_attn(q, k, v, [(0, Lk)])
        _tuning("attn_variant", 0)             # plain kernel: grid (q-tile, head, batch), no remap, no pipelining
        plain = ops.flash_attn(q, k, v, [(0, Lk)])
    finally:
        _tuning("attn_xcd", 1)
        _tuning("attn_variant", 2)
        _tuning("attn_asm", 1)
    assert torch.equal(got, got0) and torch.equal(pipe, pipe0), "XCD-aware workgroup placement must not change a single bit"
    # every element: a wrong (head, q-tile) mapping or a dropped key tile is an O(1) error, far above two kernels' rounding
    d = (got.float() - plain.float()).abs()
    assert d.max().item() < 8e-3, d.max().item()
    # ... and relative to the SIGNAL: at 18720 keys the output's own standard deviation is ~0.7 / sqrt(18720 / e) = 8e-3, so the
    # absolute bounds here are ~1 sigma; a dropped key tile (1 of 293) or a 1 % mis-scale is invisible to them but not to these
    rel_plain = ((got.double() - plain.double()).norm() / plain.double().norm()).item()
    assert rel_plain < 5e-3, rel_plain
    assert torch.equal(pipe, plain), "the ping-pong kernel and the plain one round identically"
    # sampled rows, exact: two rows of every (head, 256-row q-tile) workgroup, in different waves / lane halves; plus the
    # first and last rows
    nqt = (Lq + 255) // 256
    worst = worst_rel = 0.0
    scale = 1.0 / math.sqrt(D)
    for h in range(H):
        rows = set()
        for t in range(nqt):
            for r in ((37 * t + 11 * h) % 256, (101 * t + 53 * h + 128) % 256):
                rows.add(min(t * 256 + r, Lq - 1))
        rows |= {0, Lq - 1}
        idx = torch.tensor(sorted(rows), device=DEV)
        s = (q[0, idx, h].double() @ k[0, :, h].double().t()) * scale
        ref = torch.softmax(s, dim=-1) @ v[0, :, h].double()
        err = (got[0, idx, h].double() - ref).abs().max().item()
        worst = max(worst, err)
        rel = ((got[0, idx, h].double() - ref).norm() / ref.norm()).item()
        worst_rel = max(worst_rel, rel)
        assert rel < 6e-3, (h, rel)            # per head, against exact arithmetic
    print(f"Lq={Lq}: max abs err vs fp64 on sampled rows {worst:.2e}, worst per-head rel-L2 {worst_rel:.2e}; vs plain kernel (all elements) "
          f"max abs {d.max().item():.2e}, rel-L2 {rel_plain:.2e}")
    assert worst < 1.2e-2, worst


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not _have("config1_pipe.pt"), reason="golden missing")
def test_config1_pipeline_vs_reference(real30):
    """BASELINE config 1: 4-frame clip, one denoising step, through OUR CausalInferencePipeline with the HIP generator,
    against the reference's CausalInferencePipeline run on CPU (oracle/make_golden.py::gen_config1)."""
    from longlive_amd.pipeline import CausalInferencePipeline
    rec = load_golden("config1_pipe.pt")
    cfg, gen = real30
    prompt = {"prompt_embeds": synth.synth_prompt_embeds(cfg, seed=1, device=DEV)}
    P = CausalInferencePipeline(_pipe_args(steps=(1000,), nfb=1), DEV, generator=gen, text_encoder=lambda text_prompts: prompt)
    _, lat = P.inference(synth.synth_noise(cfg, 4, seed=0, device=DEV), ["p0"], return_latents=True)
    r, c = rel_l2(lat.cpu(), rec["latents"]), cosine(lat.cpu(), rec["latents"])
    print(f"config 1 latents: relL2 {r:.2e} cos {c:.6f}")
    assert r < 3e-2 and c > 0.9995
    for f in range(4):                      # every frame separately (frame f attends to frames < f through the KV cache)
        assert rel_l2(lat[:, f].cpu(), rec["latents"][:, f]) < 3e-2, f
    assert (P.kv_cache1[0]["global_end_index"], P.kv_cache1[0]["local_end_index"]) == tuple(rec["idx"])
    assert list(P.kv_cache1[0]["k"].shape) == rec["kv_shape"]
    sl = rec["slots"]
    assert rel_l2(P.kv_cache1[0]["k"][0, sl].cpu(), rec["k_l0"]) < 1e-2
    assert rel_l2(P.kv_cache1[0]["v"][0, sl].cpu(), rec["v_l0"]) < 1e-2
    assert rel_l2(P.kv_cache1[29]["k"][0, sl].cpu(), rec["k_l29"]) < 5e-2
    assert rel_l2(P.kv_cache1[29]["v"][0, sl].cpu(), rec["v_l29"]) < 5e-2


@pytest.mark.skipif(not _have("real_recache.pt"), reason="golden missing")
@pytest.mark.parametrize("gs", [False, True])
def test_real_shape_recache_vs_reference(gs):
    """Config 4's prompt switch at the real shape (2 layers): OUR InteractiveCausalInferencePipeline._recache_after_switch
    -- zero / keep the caches, ONE forward over 12 frames with L = Lk = 18720 (the 888-workgroup attention launch), cross
    cache reset -- against the reference's method on CPU: x0 of three frames, 96 sampled slots of every cache, indices.
    Run in full and with the shipped kv_only shortcut: the caches must not differ by a bit."""
    from longlive_amd.pipeline import InteractiveCausalInferencePipeline
    from longlive_amd.wan_wrapper import WanDiffusionWrapper
    rec = load_golden("real_recache.pt")
    want = rec[f"gs{int(gs)}"]
    cfg = synth.longlive_1_3b(num_layers=2)
    fs, S = cfg.frame_seqlen, 12 * cfg.frame_seqlen
    gen = WanDiffusionWrapper(timestep_shift=5.0, local_attn_size=12, sink_size=3, cfg=cfg, device=DEV,
                              state_dict=synth.synth_state_dict(cfg, seed=0, device=DEV, layers=[0, 1]))
    output = synth.synth_noise(cfg, 24, seed=7, device=DEV)
    new_prompt = {"prompt_embeds": synth.synth_prompt_embeds(cfg, seed=2, device=DEV)}
    results = []
    for kv_only in (False, True):
        gen.supports_kv_only = kv_only
        I = InteractiveCausalInferencePipeline(_pipe_args(global_sink=gs), DEV, generator=gen)
        I.kv_cache1, I.crossattn_cache = _new_caches(2, S, ref_style=True)
        for i, c in enumerate(I.kv_cache1):
            c["k"], c["v"] = _kv_fill(cfg, i, S)
            c["global_end_index"].fill_(24 * fs); c["local_end_index"].fill_(S)
        I._set_all_modules_max_attention_size(12)
        x0s = []
        orig = gen.forward

        def spy(*a, **k):
            out = orig(*a, **k)
            x0s.append(out[1])
            return out
        gen.forward = spy
        try:
            I._recache_after_switch(output, 24, new_prompt)
        finally:
            gen.forward = orig
        assert len(x0s) == 1
        results.append(([c["k"].clone() for c in I.kv_cache1], [c["v"].clone() for c in I.kv_cache1]))
        assert (int(I.kv_cache1[0]["global_end_index"]), int(I.kv_cache1[0]["local_end_index"])) == tuple(want["idx"])
        assert [bool(c["is_init"]) for c in I.crossattn_cache] == want["ca_init"]
        if not kv_only:
            x0 = x0s[0][:, rec["frames"]].cpu()
            r, c = rel_l2(x0, want["x0_frames"]), cosine(x0, want["x0_frames"])
            print(f"recache gs={gs}: x0 relL2 {r:.2e} cos {c:.6f}")
            assert r < 3e-2 and c > 0.9995
            for i in range(2):
                for nm in ("k", "v"):
                    a, b = I.kv_cache1[i][nm][0, rec["slots"]].cpu(), want[nm][i]
                    za, zb = a.float().abs().sum(dim=(1, 2)) == 0, b.float().abs().sum(dim=(1, 2)) == 0
                    assert torch.equal(za, zb), f"layer {i} {nm}: different slot occupancy"
                    assert rel_l2(a, b) < (1e-2 if i == 0 else 3e-2), (i, nm, rel_l2(a, b))
    gen.supports_kv_only = True
    for a, b in zip(results[0][0] + results[0][1], results[1][0] + results[1][1]):
        assert torch.equal(a, b), "kv_only recache must leave bit-identical caches"


@pytest.mark.skipif(not _have("real_block.pt"), reason="golden missing")
@pytest.mark.parametrize("kernels", ["generated", "hip"])
def test_real_shape_block_vs_reference(kernels):
    """ONE CausalWanAttentionBlock at the real shape in steady state (full 18720-slot cache: roll + insert, Lk = 18720)
    against the reference block's CPU output (oracle/make_golden.py::gen_real_block): 48 sampled output rows, 64 sampled
    cache slots, end indices -- a per-block bound that a 30-layer rel-L2 cannot hide a wrong tile under.  Both kernel families
    are held to it: the shipped generated set (flash_attn_asm_kernel, gemm_asm_*) and the HIP set it replaced."""
    if kernels == "hip":
        _tuning("gemm_asm", 0); _tuning("attn_asm", 0)
    try:
        _real_shape_block(kernels)
    finally:
        _tuning("gemm_asm", 35); _tuning("attn_asm", 1)


def _real_shape_block(kernels):
    from longlive_amd.model import CausalWanModelHIP, _kv_commit
    rec = load_golden("real_block.pt")
    cfg = synth.longlive_1_3b(num_layers=1)
    fs, S = cfg.frame_seqlen, 12 * cfg.frame_seqlen
    m = CausalWanModelHIP(cfg, device=DEV)
    m.load_state_dict(synth.synth_state_dict(cfg, seed=0, device=DEV, layers=[0]))
    for mod in m.modules():
        if hasattr(mod, "max_attention_size"):
            mod.max_attention_size = S
    xs = synth.hash_normal(71, "blk.x", (1, 3 * fs, cfg.dim), device=DEV).to(bf)
    e0 = (0.3 * synth.hash_normal(71, "blk.e0", (1, 3, 6, cfg.dim), device=DEV)).to(bf)
    ctx = synth.hash_normal(71, "blk.ctx", (1, cfg.text_len, cfg.dim), device=DEV).to(bf)
    k, v = _kv_fill(cfg, 0, S)
    kv = dict(k=k, v=v, global_end_index=S, local_end_index=S)
    ca = {"k": torch.zeros(1, 512, 12, 128, dtype=bf, device=DEV), "v": torch.zeros(1, 512, 12, 128, dtype=bf, device=DEV),
          "is_init": False}
    plan = m.block_forward(0, xs, e0, ctx, kv, ca, 3, (30, 52), current_start=S)
    _kv_commit(kv, plan.G_new, plan.E_new)
    y = xs[0, rec["rows"].to(DEV)].cpu()
    r, c = rel_l2(y, rec["y_rows"]), cosine(y, rec["y_rows"])
    print(f"real block ({kernels} kernels): relL2 {r:.2e} cos {c:.6f}")
    assert r < 6e-3 and c > 0.9999, (r, c)
    assert (kv["global_end_index"], kv["local_end_index"]) == tuple(rec["idx"])
    sl = rec["slots"].to(DEV)
    assert rel_l2(kv["k"][0, sl].cpu(), rec["k_slots"]) < 5e-3
    assert torch.equal(kv["v"][0, sl].cpu()[: 48], rec["v_slots"][: 48])       # rolled (old) slots: bit-exact copies
    assert rel_l2(kv["v"][0, sl].cpu(), rec["v_slots"]) < 5e-3
    assert abs(float(xs.float().mean()) - rec["y_mean"]) < 2e-3 and abs(float(xs.float().std()) / rec["y_std"] - 1) < 2e-3


def _long_run(gen, cfg, T, quant):
    from longlive_amd.pipeline import CausalInferencePipeline
    gen.model.set_quant(quant)
    prompt = {"prompt_embeds": synth.synth_prompt_embeds(cfg, seed=1, device=DEV)}
    P = CausalInferencePipeline(_pipe_args(), DEV, generator=gen, text_encoder=lambda text_prompts: prompt)
    P.randn_like = TD.HashRandn(43)
    _, lat = P.inference(synth.synth_noise(cfg, T, seed=0, device=DEV), ["p0"], return_latents=True)
    gen.model.set_quant(None)
    return P, lat


def _check_long(P, lat, cfg, T):
    fs = cfg.frame_seqlen
    assert lat.shape == (1, T, 16, 60, 104) and torch.isfinite(lat.float()).all()
    # the state machine's invariants after T frames: global end = T frames, local end = the full 12-frame window
    for c in (P.kv_cache1[0], P.kv_cache1[29]):
        assert (c["global_end_index"], c["local_end_index"]) == (T * fs, 12 * fs)
    # no drift / blow-up over the stream: per-frame statistics of late frames stay in the band of the early ones
    std = lat.float().std(dim=(0, 2, 3, 4))
    assert 0.3 < float(std.min()) and float(std.max()) < 3.0, (float(std.min()), float(std.max()))
    # the sink (first 3 frames' K) is still in place and untouched by 70+ rolls: slots [0, 3 fs) are non-zero and identical
    # in every later block (checked: they equal what block 0 wrote, because the window never overwrites them)
    assert float(P.kv_cache1[0]["k"][0, : 3 * fs].float().abs().sum()) > 0


@pytest.mark.skipif(not _have("config2_pipe.pt"), reason="golden missing")
def test_config2_pipeline_vs_reference_teacher_forced(real30):
    """Every forward of config 2 entered from the reference's history: per-forward bound of SURVEY.md section 8c (rel-L2 <= 3e-2,
    cosine >= 0.9995) on all 28 denoising forwards (19 of them against whole tensors, the rest on the 8192-element sample), the
    block's latents, and the cache slots the context pass wrote (layer 0 <= 1e-2, deeper layers <= 5e-2, occupancy and end
    indices exact) -- through blocks 4-6, where the window rolls."""
    rec, P, lat, spy = _config2_run(real30, teacher=True)
    for r in spy.rows:
        if "rel" in r:
            assert r["rel"] < 3e-2 and r["cos"] > 0.9995, r
        assert r["rel_sample"] < 3e-2 and r["cos_sample"] > 0.9995, r
    for r in spy.kv_rows:
        assert r["rel"] < (1e-2 if r["layer"] == 0 else 5e-2), r
    assert torch.equal(lat.cpu(), rec["latents"])           # teacher-forced: the pipeline carried the reference's latents


@pytest.mark.skipif(not _have("config2_pipe.pt"), reason="golden missing")
def test_config2_pipeline_vs_reference_free_running(real30):
    """The same 35 forwards with OUR history only (our x0 re-noised, our caches): what a user gets.  bf16 rounding differences
    between two implementations compound through x0 -> re-noise -> KV cache -> later blocks; the growth per block is printed and
    recorded in DESIGN.md section 2.  Bounds: every block's latents rel-L2 <= 3e-2 / cosine >= 0.9995 against the reference."""
    rec, P, lat, spy = _config2_run(real30, teacher=False)
    for blk in range(7):
        a, b = lat[:, 3 * blk: 3 * blk + 3].cpu(), rec["latents"][:, 3 * blk: 3 * blk + 3]
        r, c = rel_l2(a, b), cosine(a, b)
        print(f"config 2 free-running: block {blk} latents relL2 {r:.2e} cos {c:.6f}")
        assert r < 3e-2 and c > 0.9995, (blk, r, c)
    assert (P.kv_cache1[0]["global_end_index"], P.kv_cache1[29]["local_end_index"]) == (21 * cfg_fs(real30), 12 * cfg_fs(real30))


def cfg_fs(real30):
    return real30[0].frame_seqlen


@pytest.mark.skipif(not (_have("config2_pipe.pt") and _have("config2_recache.pt")), reason="golden missing")
@pytest.mark.parametrize("gs", [True, False])
def test_config2_switch_at_full_depth_vs_reference(real30, gs):
    """Config 4's switch at full depth on the state config 2 left: the reference ran its 21 frames, then
    `_recache_after_switch(latents, 21, new prompt)` -- ONE 30-layer forward over frames 9..20 (L = Lk = 18720) -- with global_sink
    True (caches kept, sink slots protected) and False (caches zeroed, sink rewritten).  Here: our pipeline teacher-forced through
    the same 21 frames (caches written by OUR kernels from the reference's latents), then OUR `_recache_after_switch`.  x0 of three
    frames, 96 sampled slots of K / V of layers 0 / 14 / 29, occupancy and end indices."""
    from longlive_amd.pipeline import InteractiveCausalInferencePipeline
    rec, P, lat, _ = _config2_run(real30, teacher=True)
    rr = load_golden("config2_recache.pt")
    want = rr[f"gs{int(gs)}"]
    cfg, gen = real30
    new_prompt = {"prompt_embeds": synth.synth_prompt_embeds(cfg, seed=rr["prompt_seed"], device=DEV)}
    P._join_context()
    I = InteractiveCausalInferencePipeline(_pipe_args(global_sink=gs), DEV, generator=gen)
    I.kv_cache1, I.crossattn_cache = P.kv_cache1, P.crossattn_cache
    I._set_all_modules_max_attention_size(12)
    x0s, orig, kv_only = [], gen.forward, gen.supports_kv_only

    def spy(*a, **k):
        out = orig(*a, **k)
        x0s.append(out[1])
        return out
    gen.forward, gen.supports_kv_only = spy, False          # the full forward: its x0 is what is compared
    try:
        I._recache_after_switch(lat, rr["start_frame"], new_prompt)
    finally:
        gen.forward, gen.supports_kv_only = orig, kv_only
    torch.cuda.synchronize()
    assert len(x0s) == 1 and x0s[0].shape[1] == 12
    x0 = x0s[0][:, rr["frames"]].cpu()
    r, c = rel_l2(x0, want["x0_frames"]), cosine(x0, want["x0_frames"])
    print(f"config 2 switch gs={gs}: x0 relL2 {r:.2e} cos {c:.6f}")
    assert r < 3e-2 and c > 0.9995
    assert (int(I.kv_cache1[0]["global_end_index"]), int(I.kv_cache1[0]["local_end_index"])) == tuple(want["idx"])
    sl = rr["slots"].to(DEV)
    for li, layer in enumerate(rr["layers"]):
        for nm in ("k", "v"):
            a, b = I.kv_cache1[layer][nm][0, sl].cpu(), want[nm][li]
            za, zb = a.float().abs().sum(dim=(1, 2)) == 0, b.float().abs().sum(dim=(1, 2)) == 0
            assert torch.equal(za, zb), f"layer {layer} {nm}: different slot occupancy"
            e = rel_l2(a, b)
            print(f"config 2 switch gs={gs}: layer {layer} {nm} slots relL2 {e:.2e}")
            assert e < (1e-2 if layer == 0 else 5e-2), (layer, nm, e)


@pytest.mark.skipif(not (_have("config4_pipe.pt") and _have("config2_pipe.pt")), reason="golden missing")
def test_config4_interactive_vs_reference_at_full_depth(real30):
    """BASELINE config 4 END TO END at full depth against the reference's own InteractiveCausalInferencePipeline.inference
    (oracle/make_golden.py::gen_config4: 30 layers, 60x104, T = 21, prompts p0 -> p1 at frame 12, `global_sink` false): OUR
    interactive pipeline free-running on the MI355X -- blocks 0-3 under p0, the KV-recache forward (caches zeroed, 12 frames in one
    forward under p1, sink rewritten), blocks 4-6 under p1 on the recached window as it rolls.  Compared: the generator-call sequence
    (timestep, current_start, frames, recache flag) of all 36 calls; latents before the switch against config 2's golden (the
    reference's run reproduces it bit for bit up to there) and after it against this one, per block; an 8192-element sample of every
    x0 after the switch; 24 sampled K / V slots of layers 0 / 14 / 29 + end indices after the recache and after every later context
    pass.  Bounds: rel-L2 <= 3e-2 / cosine >= 0.9995 per forward and per block, cache slots 1.2e-2 (layer 0) / 5e-2."""
    from longlive_amd.pipeline import InteractiveCausalInferencePipeline
    rec, rec2 = load_golden("config4_pipe.pt"), load_golden("config2_pipe.pt")
    cfg, gen = real30
    fs, SW = cfg.frame_seqlen, rec["switch_frame"]
    prompts = {f"p{i}": {"prompt_embeds": synth.synth_prompt_embeds(cfg, seed=sd, device=DEV)} for i, sd in enumerate(rec["prompt_seeds"])}
    I = InteractiveCausalInferencePipeline(_pipe_args(global_sink=False), DEV, generator=gen, text_encoder=lambda text_prompts: prompts[text_prompts[0]])
    I.randn_like = TD.HashRandn(rec["renoise_seed"])
    calls, orig = [], gen.forward
    sl, samp = rec["slots"].to(DEV), rec["sample_idx"].to(DEV)

    def spy(*a, **k):
        out = orig(*a, **k)
        want = rec["calls"][len(calls)]
        nf = k["noisy_image_or_video"].shape[1]
        got = dict(t=float(k["timestep"].flatten()[0]), current_start=int(k["current_start"]), frames=nf,
                   recache=bool(k.get("sink_recache_after_switch", False)))
        assert abs(got["t"] - want["t"]) < 1e-3 and (got["current_start"], got["frames"], got["recache"]) == (want["current_start"], want["frames"], want["recache"]), (len(calls), got, {kk: want[kk] for kk in got})
        row = dict(n=len(calls), **got)
        if "x0_sample" in want and out is not None and out[1] is not None:
            g = out[1].flatten()[samp].cpu()
            row.update(rel=rel_l2(g, want["x0_sample"]), cos=cosine(g, want["x0_sample"]))
        if "kv" in want:
            torch.cuda.synchronize()                      # (a context pass may run on the pipeline's second stream)
            kv = k["kv_cache"]
            assert (int(kv[0]["global_end_index"]), int(kv[0]["local_end_index"])) == tuple(want["kv"]["idx"]), (len(calls), want["kv"]["idx"])
            row["kv"] = {}
            for li, layer in enumerate(rec["layers"]):
                for nm in ("k", "v"):
                    a_, b_ = kv[layer][nm][0, sl].cpu(), want["kv"][nm][li]
                    assert torch.equal(a_.float().abs().sum(dim=(1, 2)) == 0, b_.float().abs().sum(dim=(1, 2)) == 0), (len(calls), layer, nm, "slot occupancy")
                    row["kv"][f"L{layer}.{nm}"] = rel_l2(a_, b_)
        calls.append(row)
        return out
    gen.forward = spy
    try:
        _, lat = I.inference(synth.synth_noise(cfg, rec["T"], seed=rec["noise_seed"], device=DEV), text_prompts_list=[["p0"], ["p1"]],
                             switch_frame_indices=[SW], return_latents=True)
    finally:
        gen.forward = orig
    assert len(calls) == 36
    for r in calls:
        if "rel" in r:
            print(f"config 4: call {r['n']} (frame {r['current_start'] // fs}, t={r['t']:.0f}): x0 sample relL2 {r['rel']:.2e} cos {r['cos']:.6f}")
            assert r["rel"] < 3e-2 and r["cos"] > 0.9995, r
        if "kv" in r:
            print(f"config 4: call {r['n']} ({'recache' if r['frames'] == 12 else 'context pass'} at frame {r['current_start'] // fs}) cache slots: "
                  + "  ".join(f"{k_} {v_:.1e}" for k_, v_ in r["kv"].items()))
            for k_, v_ in r["kv"].items():
                assert v_ < (1.2e-2 if k_.startswith("L0.") else 5e-2), (r["n"], k_, v_)      # free-running: layer 0's K / V carry the latents' own 8e-3
    want_lat = torch.cat([rec2["latents"][:, :SW], rec["latents_after_switch"]], dim=1)
    for blk in range(7):
        a_, b_ = lat[:, 3 * blk: 3 * blk + 3].cpu(), want_lat[:, 3 * blk: 3 * blk + 3]
        r_, c_ = rel_l2(a_, b_), cosine(a_, b_)
        print(f"config 4: block {blk} ({'p0' if blk < 4 else 'p1, after the switch'}) latents relL2 {r_:.2e} cos {c_:.6f}")
        assert r_ < 3e-2 and c_ > 0.9995, (blk, r_, c_)
    assert calls[20]["frames"] == 12 and calls[20]["recache"]           # the switch took effect at block 4 (frame 12)


@pytest.mark.skipif(not _have("config3_pipe.pt"), reason="golden missing")
def test_config3_sixteen_blocks_vs_reference(real30):
    """BASELINE config 3's regime over a longer horizon than config 2: 48 latent frames = 16 blocks = 80 forwards of the reference's
    CausalInferencePipeline at full depth (oracle/make_golden.py::gen_config3), the non-sink window turning over three times.  OUR
    pipeline free-running: per block an 8192-element sample of the latents and the end indices after its context pass, after blocks
    3 / 7 / 11 / 15 also 24 sampled K / V slots of layers 0 / 14 / 29; the last two blocks' latents whole.  Per block rel-L2 <= 3e-2 / cosine >= 0.9995, and NO GROWTH
    along the stream: the last block within 1.15x of the first."""
    from longlive_amd.pipeline import CausalInferencePipeline
    rec = load_golden("config3_pipe.pt")
    cfg, gen = real30
    T = rec["T"]
    prompt = {"prompt_embeds": synth.synth_prompt_embeds(cfg, seed=rec["prompt_seed"], device=DEV)}
    P = CausalInferencePipeline(_pipe_args(), DEV, generator=gen, text_encoder=lambda text_prompts: prompt)
    P.randn_like = TD.HashRandn(rec["renoise_seed"])
    sl, samp = rec["slots"].to(DEV), rec["sample_idx"].to(DEV)
    noise = synth.synth_noise(cfg, T, seed=rec["noise_seed"], device=DEV)
    out = torch.zeros_like(noise)
    rs = []
    for blk, (start, lat) in enumerate(P.stream(noise, ["p0"], output=out)):
        P._join_context()
        torch.cuda.synchronize()
        want = rec["blocks"][blk]
        g = lat.flatten()[samp].cpu()
        r, c = rel_l2(g, want["latent_sample"]), cosine(g, want["latent_sample"])
        kvr = {}
        for li, layer in enumerate(rec["layers"] if "k" in want else []):          # (the golden keeps cache slots for blocks 3 / 7 / 11 / 15)
            for nm in ("k", "v"):
                a, b = P.kv_cache1[layer][nm][0, sl].cpu(), want[nm][li]
                assert torch.equal(a.float().abs().sum(dim=(1, 2)) == 0, b.float().abs().sum(dim=(1, 2)) == 0), (blk, layer, nm)
                kvr[f"L{layer}.{nm}"] = rel_l2(a, b)
        idx = (int(P.kv_cache1[0]["global_end_index"]), int(P.kv_cache1[0]["local_end_index"]))
        assert idx == tuple(want["idx"]), (blk, idx, want["idx"])
        print(f"config 3 (16 blocks): block {blk}: latents sample relL2 {r:.2e} cos {c:.6f}  " + "  ".join(f"{k} {v:.1e}" for k, v in kvr.items()))
        assert r < 3e-2 and c > 0.9995, (blk, r, c)
        for k, v in kvr.items():
            assert v < (1.2e-2 if k.startswith("L0.") else 5e-2), (blk, k, v)      # free-running: layer 0's K / V carry the latents' own 8e-3
        rs.append(r)
    assert len(rs) == T // 3
    tail = out[:, T - 6:].cpu()
    rt = rel_l2(tail, rec["latents_tail"])
    print(f"config 3 (16 blocks): last two blocks whole: relL2 {rt:.2e} cos {cosine(tail, rec['latents_tail']):.6f}")
    assert rt < 3e-2 and rs[-1] < 1.15 * rs[0], (rt, rs)


def test_config3_60s_single_prompt_property(real30):
    """BASELINE config 3 at full length: 240 latent frames (960 pixel frames = 60 s), bf16, sliding KV cache + frame sink."""
    cfg, gen = real30
    P, lat = _long_run(gen, cfg, 240, None)
    _check_long(P, lat, cfg, 240)
    # prefix property: the stream is causal, so the first 21 frames equal a 21-frame run bit for bit
    P2, lat2 = _long_run(gen, cfg, 21, None)
    assert torch.equal(lat[:, :21], lat2)


def test_config4_interactive_full_length(real30):
    """BASELINE config 4 at full length: 240 latent frames, 6 prompts, switches at 40 / 80 / 120 / 160 / 200
    (configs/longlive_interactive_inference.yaml:21-27; global_sink = false), the KV-recache forward on every switch
    (interactive_causal_inference.py:34-106).  ~11 s on one MI355X.  Switch frames that are not block starts take effect at the
    block that contains them: blocks 14, 27, 40, 54, 67 (the reference's own rule, :258-262)."""
    from longlive_amd.pipeline import InteractiveCausalInferencePipeline
    cfg, gen = real30
    T, sw = 240, [40, 80, 120, 160, 200]
    prompts = {f"p{i}": {"prompt_embeds": synth.synth_prompt_embeds(cfg, seed=1 + i, device=DEV)} for i in range(6)}
    I = InteractiveCausalInferencePipeline(_pipe_args(global_sink=False), DEV, generator=gen, text_encoder=lambda text_prompts: prompts[text_prompts[0]])
    I.randn_like = TD.HashRandn(47)
    _, lat = I.inference(synth.synth_noise(cfg, T, seed=0, device=DEV), text_prompts_list=[[f"p{i}"] for i in range(6)],
                         switch_frame_indices=sw, return_latents=True, profile=True)
    pr = I.last_profile
    assert list(pr["switch_blocks"]) == [14, 27, 40, 54, 67], pr["switch_blocks"]
    fs = cfg.frame_seqlen
    assert lat.shape == (1, T, 16, 60, 104) and torch.isfinite(lat.float()).all()
    for c in (I.kv_cache1[0], I.kv_cache1[29]):
        assert (c["global_end_index"], c["local_end_index"]) == (374400, 18720) == (T * fs, 12 * fs)
    std = lat.float().std(dim=(0, 2, 3, 4))
    assert 0.3 < float(std.min()) and float(std.max()) < 3.0, (float(std.min()), float(std.max()))
    print(f"config 4: switch blocks {pr['switch_blocks']}, switch latencies {[round(x, 1) for x in (pr.get('switch_latency_ms') or [])]} ms")


def test_config5_int8_long_run_property(real30):
    """BASELINE config 5 (one of its 8 replicas) at its STATED size: 240 s = 960 latent frames (3840 pixel frames), W8A8 block
    linears, sliding KV cache + frame sink.  ~45 s on one MI355X.  960 frames is also the longest stream the RoPE frame table
    admits (1024 entries: the last block's start_frame is 957)."""
    cfg, gen = real30
    T = int(os.environ.get("LONGLIVE_CONFIG5_FRAMES", "960"))
    assert T % 3 == 0 and T - 3 + 3 <= 1024, "RoPE frame index must stay below 1024"
    P, lat = _long_run(gen, cfg, T, "int8")
    _check_long(P, lat, cfg, T)
    if T == 960:
        assert (P.kv_cache1[0]["global_end_index"], P.kv_cache1[0]["local_end_index"]) == (1497600, 18720)


# ---------------------------------------------------------------------------------------------------------------------
def test_batch2_throughput_mode_is_bit_identical_to_two_streams(real30):
    """Throughput mode of BASELINE config 5 (`num_samples` prompts per GPU, configs/longlive_inference.yaml:23, inference.py:193-195):
    TWO independent prompt streams batched through one forward (B = 2: every GEMM sees M = 9360 and reads its weights once, the
    self-attention launch has 456 workgroups).  Real shape, 30 layers, 12 latent frames (4 AR blocks: direct insert, roll and the
    full 12-frame window).  The batched latents must equal the two streams run one at a time BIT FOR BIT: no kernel may mix rows of
    different samples, and a row's arithmetic may not depend on where its tile falls."""
    from longlive_amd.pipeline import CausalInferencePipeline
    cfg, gen = real30
    T = 12
    noises = [synth.synth_noise(cfg, T, seed=s, device=DEV) for s in (0, 1)]
    prompts = [synth.synth_prompt_embeds(cfg, seed=11 + s, device=DEV) for s in (0, 1)]

    class PerSampleRandn:                                 # re-noise source: sample b of a batch draws what stream b draws alone
        def __init__(self, streams):
            self.streams, self.i = streams, 0

        def __call__(self, like):                          # like: [B * F, 16, h, w]
            per = like.shape[0] // len(self.streams)
            x = torch.cat([synth.hash_normal(77 + s, f"renoise.{self.i}", (per,) + tuple(like.shape[1:])).to(like.dtype) for s in self.streams])
            self.i += 1
            return x.to(like.device)

    def run(noise, prompt, streams):
        P = CausalInferencePipeline(_pipe_args(), DEV, generator=gen, text_encoder=lambda text_prompts: {"prompt_embeds": prompt})
        P.randn_like = PerSampleRandn(streams)
        _, lat = P.inference(noise, ["p"] * noise.shape[0], return_latents=True)
        return lat

    singles = [run(noises[s], prompts[s], [s]) for s in (0, 1)]
    both = run(torch.cat(noises), torch.cat(prompts), [0, 1])
    assert both.shape == (2, T, 16, 60, 104) and torch.isfinite(both.float()).all()
    assert not torch.equal(singles[0], singles[1])
    for s in (0, 1):
        assert torch.equal(both[s:s + 1], singles[s]), f"sample {s}: {(both[s:s + 1].float() - singles[s].float()).abs().max().item()}"
