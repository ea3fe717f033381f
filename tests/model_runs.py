"""Shared set-up of the model-level GPU tests (plain helpers and one fixture, no tests): the 30-layer generator, caches and their
synthetic fill, one real-shape block in steady state, the 30-layer steady-state forward, BASELINE config 2 through our pipeline
with a spy on the generator, and the toy model."""
import os
from types import SimpleNamespace

import pytest
import torch

import trace_driver as TD
from conftest import GOLDEN, load_golden
from longlive_amd import synth
from oracle import ref_model as RM
from util import bf, cosine, rel_l2

DEV = "cuda"


def have(name):
    return os.path.exists(os.path.join(GOLDEN, name))


def pipe_args(steps=(1000, 750, 500, 250), nfb=3, global_sink=True):
    return SimpleNamespace(model_kwargs=SimpleNamespace(local_attn_size=12, sink_size=3, timestep_shift=5.0),
                           denoising_step_list=list(steps), warp_denoising_step=True, num_frame_per_block=nfb,
                           context_noise=0, global_sink=global_sink)


@pytest.fixture(scope="module")
def real30():
    """One random-init LongLive-1.3B (30 layers) generator shared by the tests of a module (imported by name where it is used)."""
    from longlive_amd.wan_wrapper import WanDiffusionWrapper
    cfg = synth.longlive_1_3b()
    gen = WanDiffusionWrapper(timestep_shift=5.0, local_attn_size=12, sink_size=3, cfg=cfg, device=DEV,
                              state_dict=synth.synth_state_dict(cfg, seed=0, device=DEV))
    for mod in gen.model.modules():
        if hasattr(mod, "max_attention_size"):
            mod.max_attention_size = 12 * cfg.frame_seqlen
    yield cfg, gen
    gen.model.set_quant(None)


def new_caches(n_layers, S, ref_style=False):
    if ref_style:      # exactly what the reference allocates (pipeline/causal_inference.py:255-293)
        kv = [{"k": torch.zeros([1, S, 12, 128], dtype=bf, device=DEV), "v": torch.zeros([1, S, 12, 128], dtype=bf, device=DEV),
               "global_end_index": torch.tensor([0], dtype=torch.long, device=DEV),
               "local_end_index": torch.tensor([0], dtype=torch.long, device=DEV)} for _ in range(n_layers)]
    else:
        kv = [dict(k=torch.zeros(1, S, 12, 128, dtype=bf, device=DEV), v=torch.zeros(1, S, 12, 128, dtype=bf, device=DEV),
                   global_end_index=0, local_end_index=0) for _ in range(n_layers)]
    ca = [{"k": torch.zeros([1, 512, 12, 128], dtype=bf, device=DEV), "v": torch.zeros([1, 512, 12, 128], dtype=bf, device=DEV),
           "is_init": False} for _ in range(n_layers)]
    return kv, ca


def kv_fill(cfg, layer, S, seed=61):
    k = synth.hash_normal(seed, f"kv.{layer}.k", (1, S, cfg.num_heads, cfg.head_dim), device=DEV).to(bf)
    v = (0.5 * synth.hash_normal(seed, f"kv.{layer}.v", (1, S, cfg.num_heads, cfg.head_dim), device=DEV)).to(bf)
    return k, v


# ---------------------------------------------------------------------------------------------------------------------
class RealBlock:
    """ONE block at the real shape in steady state (full 18720-slot cache: roll + insert, Lk = 18720): the model, its weights and
    the hash inputs of `seed`, run on the GPU in any set_quant mode and on the host by any oracle model."""

    def __init__(self, seed):
        from longlive_amd.model import CausalWanModelHIP
        self.cfg = cfg = synth.longlive_1_3b(num_layers=1)
        self.fs, self.S = cfg.frame_seqlen, 12 * cfg.frame_seqlen
        self.sd = synth.synth_state_dict(cfg, seed=0, device=DEV, layers=[0])
        self.m = CausalWanModelHIP(cfg, device=DEV)
        self.m.load_state_dict(self.sd)
        for mod in self.m.modules():
            if hasattr(mod, "max_attention_size"):
                mod.max_attention_size = self.S
        self.x0 = synth.hash_normal(seed, "blk.x", (1, 3 * self.fs, cfg.dim), device=DEV).to(bf)
        self.e0 = (0.3 * synth.hash_normal(seed, "blk.e0", (1, 3, 6, cfg.dim), device=DEV)).to(bf)
        self.ctx = synth.hash_normal(seed, "blk.ctx", (1, cfg.text_len, cfg.dim), device=DEV).to(bf)
        self.k, self.v = kv_fill(cfg, 0, self.S)
        self.slots = torch.linspace(0, self.S - 1, 64).round().long()          # the cache slots the block tests compare

    def run(self, quant):
        """The block on the GPU with set_quant(quant): (output on the host, the committed cache dict)."""
        from longlive_amd.model import _kv_commit
        S = self.S
        self.m.set_quant(quant)
        try:
            xs = self.x0.clone()
            kv = dict(k=self.k.clone(), v=self.v.clone(), global_end_index=S, local_end_index=S)
            ca = {"k": torch.zeros(1, 512, 12, 128, dtype=bf, device=DEV), "v": torch.zeros(1, 512, 12, 128, dtype=bf, device=DEV),
                  "is_init": False}
            plan = self.m.block_forward(0, xs, self.e0, self.ctx, kv, ca, 3, (30, 52), current_start=S)
            _kv_commit(kv, plan.G_new, plan.E_new)
        finally:
            self.m.set_quant(None)
        return xs.cpu(), kv

    def oracle(self, make):
        """The block on the host by make(RefConfig, state dict on the host, **kw): (output, cache dict, plan)."""
        S = self.S
        ref = make(RM.RefConfig.from_cfg(self.cfg), {kk: vv.cpu() for kk, vv in self.sd.items()}, frame_seqlen_for_max_attn=self.fs)
        ref.max_attention_size = S
        kvr = dict(k=self.k.cpu().clone(), v=self.v.cpu().clone(), global_end_index=S, local_end_index=S)
        car = dict(k=torch.zeros(1, 512, 12, 128, dtype=bf), v=torch.zeros(1, 512, 12, 128, dtype=bf), is_init=False)
        y, planr = ref.block(self.x0.cpu(), 0, self.e0.cpu(), (3, 30, 52), self.ctx.cpu(), kvr, car, S, False)
        return y, kvr, planr


def steady_flow(real30):
    """The 30-layer steady-state forward of real_fwd.pt (roll + insert, Lk = 18720) in whatever modes the generator is set to: the
    flow on the host.  The end indices are checked against the golden's."""
    rec = load_golden("real_fwd.pt")
    cfg, gen = real30
    S = 12 * cfg.frame_seqlen
    prompt = {"prompt_embeds": synth.synth_prompt_embeds(cfg, seed=1, device=DEV)}
    noise = synth.synth_noise(cfg, 3, seed=0, device=DEV)
    kv, ca = new_caches(30, S)
    for i in range(30):
        kv[i]["k"], kv[i]["v"] = kv_fill(cfg, i, S)
        kv[i]["global_end_index"] = S; kv[i]["local_end_index"] = S
    flow, _ = gen(noise, prompt, torch.full((1, 3), 625.0, device=DEV), kv_cache=kv, crossattn_cache=ca, current_start=S)
    assert (kv[0]["global_end_index"], kv[0]["local_end_index"]) == tuple(rec["idx_steady"])
    return flow.cpu()


# ---------------------------------------------------------------------------------------------------------------------
# BASELINE config 2 EXACTLY, against the reference's own pipeline at full depth and size (oracle/make_golden.py::gen_config2):
# 30 layers, 60x104, T = 21, steps [1000, 750, 500, 250] + re-noise + clean-context pass, window 12 / sink 3 -- 7 blocks, the
# window fills in blocks 0-3 and ROLLS in blocks 4-6, every cache entry written by the model itself (no synthetic cache content).
class Config2Spy:
    """Sits on generator.forward while OUR CausalInferencePipeline runs.  Call n = 5 * block + j: j < 4 are the denoising
    forwards, j = 4 the clean-context pass.  Records rel-L2 / cosine of every x0 against the reference's; after the context pass
    compares the sampled K / V slots and the end indices.  teacher=True: the reference's x0 is handed back to the pipeline instead
    of ours wherever the golden stores it whole (every block's last step = the latents; all steps of blocks 0 / 4 / 6), so that
    every forward is entered from the REFERENCE's history (latents, re-noise input, and caches that OUR kernels wrote from the
    reference's latents) -- errors cannot compound across blocks."""

    def __init__(self, gen, rec, teacher, check=True):
        self.gen, self.rec, self.teacher, self.orig, self.check = gen, rec, teacher, gen.forward, check
        self.n, self.rows, self.kv_rows = 0, [], []

    def __enter__(self):
        self.gen.forward = self
        return self

    def __exit__(self, *exc):
        self.gen.forward = self.orig

    def __call__(self, *a, **k):
        out = self.orig(*a, **k)
        blk, j = divmod(self.n, 5)
        self.n += 1
        b = self.rec["blocks"][blk]
        want_call = self.rec["calls"][self.n - 1]
        assert int(k["current_start"]) == want_call["current_start"], (self.n - 1, k["current_start"], want_call)
        assert abs(float(k["timestep"].flatten()[0]) - want_call["t"]) < 1e-3, (self.n - 1, want_call)
        if j < 4:
            x0 = out[1]
            full = self.rec["latents"][:, 3 * blk: 3 * blk + 3] if j == 3 else (b["x0_steps"][j] if b["x0_steps"] else None)
            got_s = x0.flatten()[self.rec["sample_idx"].to(x0.device)].cpu()
            row = dict(block=blk, step=j, rel_sample=rel_l2(got_s, b["x0_samples"][j]), cos_sample=cosine(got_s, b["x0_samples"][j]))
            if full is not None:
                row.update(rel=rel_l2(x0.cpu(), full), cos=cosine(x0.cpu(), full))
                if self.teacher:
                    out = (out[0], full.to(device=x0.device, dtype=x0.dtype))
            self.rows.append(row)
        else:
            torch.cuda.synchronize()                     # the context pass may run on the pipeline's second stream
            kv = k["kv_cache"]
            idx = (int(kv[0]["global_end_index"]), int(kv[0]["local_end_index"]))
            assert idx == tuple(b["idx"]), (blk, idx, b["idx"])
            sl = self.rec["slots"].to(DEV)
            for li, layer in enumerate(self.rec["layers"]):
                for nm in ("k", "v"):
                    got, want = kv[layer][nm][0, sl].cpu(), b[nm][li]
                    za, zb = got.float().abs().sum(dim=(1, 2)) == 0, want.float().abs().sum(dim=(1, 2)) == 0
                    assert torch.equal(za, zb) or not self.check, f"block {blk} layer {layer} {nm}: different slot occupancy"
                    self.kv_rows.append(dict(block=blk, layer=layer, what=nm, rel=rel_l2(got, want)))
        return out


def config2_run(real30, teacher, check=True):
    from longlive_amd.pipeline import CausalInferencePipeline
    rec = load_golden("config2_pipe.pt")
    cfg, gen = real30
    prompt = {"prompt_embeds": synth.synth_prompt_embeds(cfg, seed=rec["prompt_seed"], device=DEV)}
    P = CausalInferencePipeline(pipe_args(), DEV, generator=gen, text_encoder=lambda text_prompts: prompt)
    P.randn_like = TD.HashRandn(rec["renoise_seed"])
    assert [float(x) for x in P.denoising_step_list] == rec["steps"]
    with Config2Spy(gen, rec, teacher, check) as spy:
        _, lat = P.inference(synth.synth_noise(cfg, rec["T"], seed=rec["noise_seed"], device=DEV), ["p0"], return_latents=True)
    assert spy.n == 35
    tag = "teacher-forced" if teacher else "free-running"
    for r in spy.rows:
        print(f"config 2 {tag}: block {r['block']} step {r['step']}: "
              + (f"relL2 {r['rel']:.2e} cos {r['cos']:.6f}  " if "rel" in r else "")
              + f"(8192-sample relL2 {r['rel_sample']:.2e} cos {r['cos_sample']:.6f})")
    for blk in range(7):
        rows = [r for r in spy.kv_rows if r["block"] == blk]
        print(f"config 2 {tag}: block {blk} cache slots: "
              + "  ".join(f"L{r['layer']}.{r['what']} {r['rel']:.1e}" for r in rows))
    return rec, P, lat, spy


# ---------------------------------------------------------------------------------------------------------------------
def toy(attn_quant, lin=None):
    from longlive_amd.wan_wrapper import WanDiffusionWrapper
    cfg = synth.toy_config(local_attn_size=3, sink_size=1)
    sd = synth.synth_state_dict(cfg, seed=3)
    gen = WanDiffusionWrapper(timestep_shift=5.0, local_attn_size=3, sink_size=1, cfg=cfg, device=DEV, state_dict=sd)
    S = 3 * cfg.frame_seqlen
    for m in gen.model.modules():
        if hasattr(m, "max_attention_size"):
            m.max_attention_size = S
    gen.model.set_quant(lin).set_attn_quant(attn_quant)
    return cfg, sd, gen, S


def toy_caches(cfg, S, dev):
    kv = [dict(k=torch.zeros(1, S, cfg.num_heads, 128, dtype=bf, device=dev), v=torch.zeros(1, S, cfg.num_heads, 128, dtype=bf, device=dev),
               global_end_index=0, local_end_index=0) for _ in range(cfg.num_layers)]
    ca = [dict(k=torch.zeros(1, cfg.text_len, cfg.num_heads, 128, dtype=bf, device=dev),
               v=torch.zeros(1, cfg.text_len, cfg.num_heads, 128, dtype=bf, device=dev), is_init=False) for _ in range(cfg.num_layers)]
    return kv, ca
