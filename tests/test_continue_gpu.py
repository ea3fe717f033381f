"""Continuing a clip on the GPU (`initial_latent` on the pipelines): a run resumed from its own first n latents reproduces the
uninterrupted run bit for bit -- latents, every layer's K/V, end indices --, with the context passes on one stream and overlapped on
two; the interactive pipeline likewise, switch inside or after the prefix; `stream` / `stream_video` against `inference`; irregular
prefixes; and uint8 frames through the encoder into a continued run.

Toy recipe of tests/test_model_gpu.py: width 1536, 2 layers, 8 x 12 latents, window 12, sink 3, 3 frames per block, TD.HashRandn."""
from types import SimpleNamespace

import pytest
import torch

import trace_driver as TD
import vae_enc_ref as ER
from longlive_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda"
T_FULL, SEED = 18, 47


def _pipe_args(global_sink=True):
    return SimpleNamespace(model_kwargs=SimpleNamespace(local_attn_size=12, sink_size=3, timestep_shift=5.0),
                           denoising_step_list=[1000, 750, 500, 250], warp_denoising_step=True, num_frame_per_block=3,
                           context_noise=0, global_sink=global_sink)


@pytest.fixture(scope="module")
def toy():
    from longlive_amd.wan_wrapper import WanDiffusionWrapper
    cfg = synth.WanConfig(num_layers=2, lat_h=8, lat_w=12, local_attn_size=12, sink_size=3)
    sd = synth.synth_state_dict(cfg, seed=21, device=DEV)
    gen = WanDiffusionWrapper(timestep_shift=5.0, local_attn_size=12, sink_size=3, cfg=cfg, device=DEV, state_dict=sd)
    table = {f"p{i}": synth.synth_prompt_embeds(cfg, seed=31 + i, device=DEV) for i in range(3)}
    enc = lambda text_prompts: {"prompt_embeds": table[text_prompts[0]]}      # noqa: E731
    noise = synth.synth_noise(cfg, T_FULL, seed=45, device=DEV)
    return SimpleNamespace(cfg=cfg, gen=gen, enc=enc, noise=noise, fs=cfg.frame_seqlen)


def _pipe(toy, interactive=False, overlap=False, drawn=0, vae=None):
    from longlive_amd.pipeline import CausalInferencePipeline, InteractiveCausalInferencePipeline
    cls = InteractiveCausalInferencePipeline if interactive else CausalInferencePipeline
    P = cls(_pipe_args(False), DEV, generator=toy.gen, text_encoder=toy.enc, vae=vae)
    P.overlap_context = overlap
    P.randn_like = TD.HashRandn(SEED)
    P.randn_like.i = drawn                     # re-noise draws the skipped blocks would have made: three per generated block
    return P


def _state(P, lat):
    torch.cuda.synchronize()
    return SimpleNamespace(lat=lat.clone(), kv=[c[x].clone() for c in P.kv_cache1 for x in ("k", "v")],
                           idx=[(c["global_end_index"], c["local_end_index"]) for c in P.kv_cache1])


def _same(got, want, n=0):
    assert got.idx == want.idx
    assert torch.equal(got.lat[:, n:], want.lat[:, n:]), "generated latents differ"
    assert torch.equal(got.lat[:, :n], want.lat[:, :n]), "the prefix was not returned as given"
    for i, (a, b) in enumerate(zip(got.kv, want.kv)):
        assert torch.equal(a, b), f"layer {i // 2} {'kv'[i % 2]} differs"


@pytest.fixture(scope="module")
def full(toy):
    """The uninterrupted 18-frame run on one stream: computed once, left unchanged."""
    P = _pipe(toy)
    _, lat = P.inference(toy.noise, ["p0"], return_latents=True)
    return _state(P, lat)


@pytest.fixture(scope="module")
def full_interactive(toy):
    """18 frames, prompt switch at frame 12, uninterrupted, one stream."""
    P = _pipe(toy, interactive=True)
    _, lat = P.inference(toy.noise, text_prompts_list=[["p0"], ["p1"]], switch_frame_indices=[12], return_latents=True)
    return _state(P, lat)


# ---- resume identity ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("overlap", [False, True], ids=["one_stream", "overlap_context"])
@pytest.mark.parametrize("n", [3, 12, 15])
def test_resumed_run_equals_the_uninterrupted_run(toy, full, n, overlap):
    """n = 12 fills the window in the prefill, n = 15 rolls it there.  Twice each: an ordering that only holds by luck would show."""
    assert full.idx == [(T_FULL * toy.fs, 12 * toy.fs)] * 2
    for rep in range(2):
        P = _pipe(toy, overlap=overlap, drawn=3 * (n // 3))
        _, lat = P.inference(toy.noise[:, n:], ["p0"], initial_latent=full.lat[:, :n], return_latents=True)
        assert lat.shape == full.lat.shape
        _same(_state(P, lat), full, n)


@pytest.mark.parametrize("overlap", [False, True], ids=["one_stream", "overlap_context"])
def test_interactive_resume_before_the_switch_equals_the_uninterrupted_run(toy, full_interactive, overlap):
    n = 6
    for rep in range(2):
        P = _pipe(toy, interactive=True, overlap=overlap, drawn=3 * (n // 3))
        _, lat = P.inference(toy.noise[:, n:], text_prompts_list=[["p0"], ["p1"]], switch_frame_indices=[12], return_latents=True,
                             initial_latent=full_interactive.lat[:, :n], profile=True)
        _same(_state(P, lat), full_interactive, n)
        assert P.last_profile["switch_blocks"] == [2] and "prefill" in P.last_profile["times_ms"]      # generated blocks 6, 9, then 12


def test_interactive_switch_inside_the_prefix_recaches_prefix_frames(toy, full):
    """Switch index 3 <= n = 6: the first generated block switches, its recache re-encodes the 6 prefix frames under the new prompt.
    No uninterrupted run leaves this state (limits); the overlapped schedule must equal the one-stream one."""
    n, runs = 6, []
    for overlap in (False, True, True):
        P = _pipe(toy, interactive=True, overlap=overlap, drawn=3 * (n // 3))
        _, lat = P.inference(toy.noise[:, n:], text_prompts_list=[["p0"], ["p1"]], switch_frame_indices=[3], return_latents=True,
                             initial_latent=full.lat[:, :n], profile=True)
        assert P.last_profile["switch_blocks"] == [0]
        runs.append(_state(P, lat))
    assert torch.isfinite(runs[0].lat.float()).all() and runs[0].idx == [(T_FULL * toy.fs, 12 * toy.fs)] * 2
    assert not torch.equal(runs[0].lat[:, n:], full.lat[:, n:])              # the new prompt took effect from the first new block
    for got in runs[1:]:
        _same(got, runs[0], n)


class _Spy(torch.nn.Module):
    """The generator behind a recorder of (kv_only, waits on per-layer events, records them, HIP stream) per call."""

    def __init__(self, gen):
        super().__init__()
        self.gen, self.model, self.calls = gen, gen.model, []
        self.supports_kv_only, self.supports_layer_events = gen.supports_kv_only, gen.supports_layer_events

    def get_scheduler(self):
        return self.gen.get_scheduler()

    def forward(self, *a, **kw):
        self.calls.append((bool(kw.get("kv_only")), "layer_wait" in kw, "layer_record" in kw, torch.cuda.current_stream().cuda_stream))
        return self.gen(*a, **kw)


@pytest.mark.parametrize("n", [1, 3, 4, 12])
def test_first_new_block_is_ordered_behind_the_whole_prefill(toy, full, n):
    """A prefill pass records layer i's event after its last access to the SELF-attention cache and fills layer i's cross-attention
    K/V afterwards; the first pass of a run is the one that fills them.  So the first denoising forward may not follow the prefill
    one layer behind on the per-layer events, as it follows a generated block's context pass: the main stream joins the aux stream
    after the prefill.  Seen from the calls: prefill passes record events on the aux stream, the first denoising forward waits on
    none (it is ordered behind the join), the second block's first forward does (the steady-state overlap is kept)."""
    from longlive_amd.pipeline import CausalInferencePipeline
    spy = _Spy(toy.gen)
    P = CausalInferencePipeline(_pipe_args(False), DEV, generator=spy, text_encoder=toy.enc)
    P.randn_like = TD.HashRandn(SEED)
    joins = []
    join = P._join_context
    P._join_context = lambda: (joins.append((len(spy.calls), P._ctx_pending)), join())[1]
    main = torch.cuda.current_stream().cuda_stream
    P.inference(toy.noise[:, :6], ["p0"], initial_latent=full.lat[:, :n])
    k = len(P._prefix_blocks(n))
    aux = P._aux.cuda_stream
    assert aux != main
    assert spy.calls[:k] == [(True, False, True, aux)] * k
    assert (k, True) in joins, "no join between the last prefill pass and the first new block"
    assert spy.calls[k:k + 4] == [(False, False, False, main)] * 4               # block n: behind the join, no event waits
    assert spy.calls[k + 4] == (True, False, True, aux)                         # its context pass
    assert spy.calls[k + 5] == (False, True, False, main)                       # block n + 3 follows it one layer behind
    assert spy.calls[k + 6:k + 9] == [(False, False, False, main)] * 3


# ---- stream / stream_video ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,starts", [(6, [0, 3, 6, 9]), (4, [0, 1, 4, 7])])
def test_stream_yields_prefix_blocks_first_and_equals_inference(toy, full, n, starts):
    T = 6
    prefix, noise = full.lat[:, :n], toy.noise[:, :T]
    P = _pipe(toy, overlap=True)
    _, lat = P.inference(noise, ["p0"], initial_latent=prefix, return_latents=True)
    want = _state(P, lat)
    S = _pipe(toy, overlap=True)
    out = torch.zeros_like(lat)
    got = [(s, b.clone()) for s, b in S.stream(noise, ["p0"], output=out, initial_latent=prefix)]
    assert [s for s, _ in got] == starts
    cat = torch.cat([b for _, b in got], 1)
    assert torch.equal(cat, want.lat) and torch.equal(out, want.lat) and torch.equal(cat[:, :n], prefix)
    _same(_state(S, out), want, n)
    assert P.last_profile is None


@pytest.fixture(scope="module")
def vae():
    from longlive_amd.vae import WanVAEWrapper
    cfg = synth.VaeConfig()
    sd = dict(synth.synth_vae_state_dict(cfg, seed=5))
    sd.update(synth.synth_vae_encoder_state_dict(cfg, seed=ER.ENC_SEED))
    m = WanVAEWrapper(device=DEV, chunk=2)
    m.load_state_dict(sd)
    return m


@pytest.mark.parametrize("n", [3, 4])
def test_video_of_a_continued_clip(toy, full, vae, n):
    """1 + 4 (n + T - 1) frames decoded from all n + T latents; stream_video's chunks concatenated equal inference's video bit for bit,
    with the blocks decoded in line or on the side stream, in either entry point."""
    T = 6
    prefix, noise = full.lat[:, :n], toy.noise[:, :T]
    P = _pipe(toy, overlap=True, vae=vae)
    video, lat = P.inference(noise, ["p0"], initial_latent=prefix, return_latents=True)
    assert video.shape == (1, 1 + 4 * (n + T - 1), 3, 64, 96) and float(video.min()) >= 0.0 and float(video.max()) <= 1.0
    assert torch.equal(video, (vae.decode_to_pixel(lat, use_cache=False) * 0.5 + 0.5).clamp(0, 1))
    P.overlap_decode = True
    P.randn_like = TD.HashRandn(SEED)
    side_video, side_lat = P.inference(noise, ["p0"], initial_latent=prefix, return_latents=True)
    assert torch.equal(side_lat, lat) and torch.equal(side_video, video)
    for overlap_decode in (False, True):
        S = _pipe(toy, overlap=True, vae=vae)
        chunks = [(s, v.clone()) for s, v in S.stream_video(noise, ["p0"], overlap_decode=overlap_decode, initial_latent=prefix)]
        assert [s for s, _ in chunks] == ([0, 3, 6] if n == 3 else [0, 1, 4, 7]), overlap_decode
        assert chunks[0][1].shape[1] == 1 + 4 * ((3 if n == 3 else 1) - 1)
        assert torch.equal(torch.cat([v for _, v in chunks], 1), video), overlap_decode


# ---- irregular prefixes, end to end ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("overlap", [False, True], ids=["one_stream", "overlap_context"])
@pytest.mark.parametrize("n", [1, 4])
def test_irregular_prefixes(toy, full, n, overlap):
    T = 6
    prefix = full.lat[:, 2:2 + n]
    P = _pipe(toy, overlap=overlap)
    _, lat = P.inference(toy.noise[:, :T], ["p0"], initial_latent=prefix, return_latents=True)
    torch.cuda.synchronize()
    assert lat.shape[1] == n + T and torch.isfinite(lat.float()).all() and torch.equal(lat[:, :n], prefix)
    assert 0.2 < float(lat[:, n:].float().std()) < 3.0
    assert all(c["global_end_index"] == (n + T) * toy.fs and c["local_end_index"] == (n + T) * toy.fs for c in P.kv_cache1)


def test_frames_to_continued_run_end_to_end(toy, vae):
    """9 uint8 frames -> encode_frames_to_latent -> inference(initial_latent=): the same bits as encoding the fp32 planes and passing
    those latents (fp32, cast once by the pipeline) or their bf16 cast by hand."""
    f = torch.randint(0, 256, (1, 9, 64, 96, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(23)).to(DEV)
    latent = vae.encode_frames_to_latent(f)
    assert latent.shape == (1, 3, 16, 8, 12) and latent.dtype == torch.float32
    by_hand = vae.encode_to_latent((f.cpu().float() / 127.5 - 1).permute(0, 4, 1, 2, 3).to(DEV))
    assert torch.equal(latent, by_hand)
    runs = []
    for prefix in (latent, by_hand.to(torch.bfloat16)):
        P = _pipe(toy, overlap=True, vae=vae)
        video, lat = P.inference(toy.noise[:, :6], ["p0"], initial_latent=prefix, return_latents=True)
        runs.append((video, _state(P, lat)))
    assert runs[0][0].shape == (1, 33, 3, 64, 96) and torch.equal(runs[0][0], runs[1][0])
    assert torch.equal(runs[0][1].lat[:, :3], latent.to(torch.bfloat16))
    _same(runs[0][1], runs[1][1], 3)
