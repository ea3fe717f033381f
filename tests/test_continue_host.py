"""Continuing a clip, host side (no GPU): the generator calls that `initial_latent` adds to the two pipelines -- the prefix blocks as
clean-context passes, then the usual 4 + 1 calls per new block on a timeline that starts at frame n --, the interactive switch rule on
that timeline, the cache size, the refusals, the CLI's frame selection, and the uint8 intake entry point at the C-ABI boundary."""
import os
import re
from types import SimpleNamespace

import pytest
import torch
import torch.nn as nn

from longlive_amd import _lib, cli, synth
from longlive_amd.pipeline import CausalInferencePipeline, InteractiveCausalInferencePipeline
from oracle import ref_ops as R
import trace_driver as TD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS = 4                                             # tokens per frame of the 4 x 4 latents below
STEPS = [1000.0, 937.5, 833.3333, 625.0]           # [1000, 750, 500, 250] warped by shift 5: 1000 * 5 s / (1 + 4 s)
CTX = 0.0                                          # context_noise


class RecordingGenerator(nn.Module):
    """Records (start frame, frames, timestep, kv_only, prompt, recache flag) and the input of every call; returns half the input,
    like tests/test_pipeline_host.py's fake."""

    supports_kv_only = True

    def __init__(self):
        super().__init__()
        self.scheduler = R.FlowMatchSchedulerRef(5.0)
        self.log, self.inputs, self.kv_shapes = [], [], []
        self.model = SimpleNamespace(num_frame_per_block=1, local_attn_size=-1, max_attention_size=0, block_mask=None,
                                     named_modules=lambda: [], _prepare_blockwise_causal_attn_mask=lambda **kw: None)

    def get_scheduler(self):
        return self.scheduler

    def forward(self, noisy_image_or_video, conditional_dict, timestep, kv_cache=None, crossattn_cache=None, current_start=None,
                sink_recache_after_switch=False, kv_only=False, **kw):
        x = noisy_image_or_video
        ts = set(round(float(v), 4) for v in timestep.flatten().tolist())
        assert len(ts) == 1 and current_start % FS == 0 and tuple(timestep.shape) == (x.shape[0], x.shape[1])
        self.log.append((current_start // FS, int(x.shape[1]), ts.pop(), bool(kv_only), conditional_dict["name"],
                         bool(sink_recache_after_switch)))
        self.inputs.append(x.clone())
        self.kv_shapes.append(tuple(kv_cache[0]["k"].shape))
        x0 = (0.5 * x.float() + 0.01 * (len(self.log) % 7)).to(x.dtype)
        return x0, x0


def _args(local_attn_size=12, gs=True):
    return SimpleNamespace(model_kwargs=SimpleNamespace(local_attn_size=local_attn_size, sink_size=3, timestep_shift=5.0),
                           denoising_step_list=[1000, 750, 500, 250], warp_denoising_step=True, num_frame_per_block=3,
                           context_noise=0, global_sink=gs)


ENC = lambda text_prompts: {"prompt_embeds": torch.zeros(1, 1), "name": text_prompts[0]}      # noqa: E731
CFG = synth.WanConfig(lat_h=4, lat_w=4)


def _pipe(cls=CausalInferencePipeline, **kw):
    fg = RecordingGenerator()
    P = cls(_args(**kw), "cpu", generator=fg, text_encoder=ENC)
    P.num_transformer_blocks, P.frame_seq_length = 2, FS
    P.randn_like = TD.HashRandn(5)
    return P, fg


def _prefix(n):
    return synth.synth_noise(CFG, n, seed=9, name="prefix") if n else torch.zeros(1, 0, 16, 4, 4, dtype=torch.bfloat16)


def _block_calls(start, prompt="p0"):
    return [(start, 3, pytest.approx(t, abs=1e-3), False, prompt, False) for t in STEPS] + [(start, 3, CTX, True, prompt, False)]


def _prefill_calls(n, prompt="p0"):
    sizes = ([n % 3] if n % 3 else []) + [3] * (n // 3)
    out, start = [], 0
    for f in sizes:
        out.append((start, f, CTX, True, prompt, False))
        start += f
    return out


# ---- call sequences -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 6, 15, 1, 4])
def test_prefix_blocks_are_context_passes_then_new_blocks_follow(n):
    T = 6
    noise, prefix = synth.synth_noise(CFG, T, seed=3), _prefix(n)
    P, fg = _pipe()
    video, lat = P.inference(noise, ["p0"], return_latents=True, initial_latent=prefix)
    want = _prefill_calls(n) + _block_calls(n) + _block_calls(n + 3)
    assert fg.log == want
    assert {3: [3], 6: [3, 3], 15: [3] * 5, 1: [1], 4: [1, 3]}[n] == [c[1] for c in fg.log[:len(_prefill_calls(n))]]
    # the prefix blocks are the prefix itself, in order; the new blocks start from the noise of the T new frames
    k = len(_prefill_calls(n))
    assert torch.equal(torch.cat(fg.inputs[:k], 1), prefix)
    assert torch.equal(fg.inputs[k], noise[:, 0:3]) and torch.equal(fg.inputs[k + 5], noise[:, 3:6])
    assert video is None and lat.shape[1] == n + T and torch.equal(lat[:, :n], prefix)
    assert torch.equal(lat[:, n:n + 3], fg.inputs[k + 4]) and torch.equal(lat[:, n + 3:], fg.inputs[k + 9])     # what the context pass read
    assert P.last_profile is None

    # stream: the same calls, the prefix blocks yielded first with their starts
    P2, fg2 = _pipe()
    out = torch.zeros(1, n + T, 16, 4, 4, dtype=noise.dtype)
    got = list(P2.stream(noise, ["p0"], output=out, initial_latent=prefix))
    assert fg2.log == want
    assert [s for s, _ in got] == [c[0] for c in _prefill_calls(n)] + [n, n + 3]
    assert torch.equal(torch.cat([b for _, b in got], 1), lat) and torch.equal(out, lat)


def test_initial_latent_is_cast_once_to_the_dtype_of_noise():
    noise = synth.synth_noise(CFG, 3, seed=3)
    prefix = _prefix(4).float() * 1.001                      # fp32 values that bf16 cannot hold
    P, fg = _pipe()
    _, lat = P.inference(noise, ["p0"], return_latents=True, initial_latent=prefix)
    assert lat.dtype == noise.dtype and torch.equal(lat[:, :4], prefix.to(noise.dtype))
    assert torch.equal(torch.cat(fg.inputs[:2], 1), prefix.to(noise.dtype))


def test_without_initial_latent_the_sequence_is_todays():
    noise = synth.synth_noise(CFG, 6, seed=3)
    runs = []
    for kw in ({}, {"initial_latent": None}):
        P, fg = _pipe()
        _, lat = P.inference(noise, ["p0"], return_latents=True, **kw)
        runs.append((fg.log, lat))
    assert runs[0][0] == runs[1][0] == _block_calls(0) + _block_calls(3)
    assert torch.equal(runs[0][1], runs[1][1]) and runs[0][1].shape == noise.shape
    P, fg = _pipe()
    assert [s for s, _ in P.stream(noise, ["p0"], initial_latent=None)] == [0, 3] and fg.log == runs[0][0]
    I, fg = _pipe(InteractiveCausalInferencePipeline, gs=False)
    I.inference(noise, text_prompts_list=[["p0"], ["p1"]], switch_frame_indices=[3], initial_latent=None)
    assert fg.log == _block_calls(0) + [(0, 3, CTX, True, "p1", True)] + _block_calls(3, "p1")


@pytest.mark.parametrize("switch,at", [(4, 6), (6, 6), (10, 12)])
def test_interactive_switch_rule_on_the_continued_timeline(switch, at):
    """n = 6, T = 9: the prefix is prefilled under the first prompt; an index <= n switches at the first GENERATED block (start 6) and
    the recache then covers prefix frames only; an index > n switches at the first block whose start >= index, and the recache reads
    prefix and generated frames from the combined output."""
    n, T = 6, 9
    noise, prefix = synth.synth_noise(CFG, T, seed=3), _prefix(n)
    I, fg = _pipe(InteractiveCausalInferencePipeline, gs=False)
    _, lat = I.inference(noise, text_prompts_list=[["p0"], ["p1"]], switch_frame_indices=[switch], return_latents=True,
                         initial_latent=prefix)
    want = _prefill_calls(n)
    for start in (6, 9, 12):
        if start == at:
            want.append((0, at, CTX, True, "p1", True))          # min(window 12, frames so far) frames, from frame 0, new prompt
        want += _block_calls(start, "p0" if start < at else "p1")
    assert fg.log == want
    rc = fg.log.index((0, at, CTX, True, "p1", True))
    assert torch.equal(fg.inputs[rc], lat[:, :at]) and torch.equal(fg.inputs[rc][:, :n], prefix)
    assert torch.equal(lat[:, :n], prefix) and lat.shape[1] == n + T


def test_global_attention_sizes_the_cache_to_the_whole_timeline():
    for n in (0, 4):
        P, fg = _pipe(local_attn_size=-1)
        P.inference(synth.synth_noise(CFG, 6, seed=3), ["p0"], initial_latent=_prefix(n) if n else None)
        assert set(fg.kv_shapes) == {(1, (n + 6) * FS, P.num_heads, P.head_dim)}
    P, fg = _pipe(local_attn_size=12)
    P.inference(synth.synth_noise(CFG, 6, seed=3), ["p0"], initial_latent=_prefix(4))
    assert set(fg.kv_shapes) == {(1, 12 * FS, P.num_heads, P.head_dim)}


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
BAD = {
    "rank": (lambda: _prefix(3)[0], "expected a tensor"),
    "batch": (lambda: _prefix(3).repeat(2, 1, 1, 1, 1), "does not share"),
    "height": (lambda: _prefix(3)[:, :, :, :2], "does not share"),
    "width": (lambda: _prefix(3)[..., :2], "does not share"),
    "device": (lambda: _prefix(3).to("meta"), "noise on cpu"),
    "empty": (lambda: _prefix(0), "no frame"),
    "rope": (lambda: torch.zeros(1, 1020, 16, 4, 4, dtype=torch.bfloat16), r"1020 given \+ 6 new frames = 1026 exceed the 1024-frame RoPE table"),
}


@pytest.mark.parametrize("entry", ["inference", "stream", "stream_video", "interactive"])
@pytest.mark.parametrize("what", sorted(BAD))
def test_bad_prefixes_are_refused_before_the_generator_is_called(entry, what):
    make, needle = BAD[what]
    noise = synth.synth_noise(CFG, 6, seed=3)
    P, fg = _pipe(InteractiveCausalInferencePipeline if entry == "interactive" else CausalInferencePipeline)
    P.vae = SimpleNamespace(model=SimpleNamespace(clear_cache=lambda: None))
    with pytest.raises(ValueError, match=needle):
        if entry == "inference":
            P.inference(noise, ["p0"], initial_latent=make())
        elif entry == "interactive":
            P.inference(noise, text_prompts_list=[["p0"]], switch_frame_indices=[], initial_latent=make())
        else:
            next(getattr(P, entry)(noise, ["p0"], initial_latent=make()))
    assert fg.log == [] and P.kv_cache1 is None


def test_the_longest_timeline_the_rope_table_holds_is_accepted():
    P, _ = _pipe()
    assert P._check_prefix(torch.zeros(1, 6, 16, 4, 4), torch.zeros(1, 1018, 16, 4, 4)).shape[1] == 1018


def test_the_rope_limit_is_the_generators_own():
    """The early refusal reads the length of the model's frame-axis RoPE table (CausalWanModelHIP.rope_frames, which builds the table);
    1024 is only the fallback for generators that do not state one."""
    from longlive_amd.model import CausalWanModelHIP
    assert CausalWanModelHIP.rope_frames == 1024 == CausalInferencePipeline.ROPE_FRAMES
    P, fg = _pipe()
    fg.model.rope_frames = 64
    assert P._check_prefix(torch.zeros(1, 6, 16, 4, 4), torch.zeros(1, 58, 16, 4, 4)).shape[1] == 58
    with pytest.raises(ValueError, match=r"59 given \+ 6 new frames = 65 exceed the 64-frame RoPE table"):
        P.inference(torch.zeros(1, 6, 16, 4, 4, dtype=torch.bfloat16), ["p0"], initial_latent=torch.zeros(1, 59, 16, 4, 4))
    assert fg.log == []


# ---- CLI: frame selection, readers ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("total,cap,want", [
    (1, None, (0, 1)), (4, None, (3, 4)), (5, None, (0, 5)), (8, None, (3, 8)), (9, None, (0, 9)), (81, None, (0, 81)), (83, None, (2, 83)),
    (1, 1, (0, 1)), (4, 9, (3, 4)), (5, 4, (4, 5)), (8, 5, (3, 8)), (9, 8, (4, 9)), (81, 21, (60, 81)), (83, 80, (6, 83)), (83, 1000, (2, 83)),
])
def test_select_clip_frames_takes_the_last_1_plus_4k(total, cap, want):
    s = cli.select_clip_frames(total, cap)
    assert (s.start, s.stop) == want and s.step is None and (s.stop - s.start) % 4 == 1
    assert s.stop == total and s.stop - s.start <= (total if cap is None else min(total, cap)) < s.stop - s.start + 4


def test_select_clip_frames_refuses_empty_clips_and_caps():
    for total, cap in ((0, None), (5, 0), (5, -3)):
        with pytest.raises(ValueError):
            cli.select_clip_frames(total, cap)


def test_load_clip_reads_avi_and_pt_checks_the_size_and_names_the_formats(tmp_path):
    frames = torch.randint(0, 256, (6, 32, 32, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(1))
    cli.write_avi_rgb24(str(tmp_path / "c.avi"), frames)
    torch.save(frames, str(tmp_path / "c.pt"))
    for name in ("c.avi", "c.pt"):
        got = cli.load_clip(cli.Config(input_video=str(tmp_path / name)), 4, 4)
        assert got.dtype == torch.uint8 and torch.equal(got, frames[1:])
        assert torch.equal(cli.load_clip(cli.Config(input_video=str(tmp_path / name), input_frames=4), 4, 4), frames[5:])
    assert cli.load_clip(cli.Config(), 4, 4) is None
    with pytest.raises(ValueError, match="32x32.*64x32.*not resized"):
        cli.load_clip(cli.Config(input_video=str(tmp_path / "c.avi")), 4, 8)
    torch.save(frames.float(), str(tmp_path / "f.pt"))
    with pytest.raises(ValueError, match="expected uint8 frames"):
        cli.load_clip(cli.Config(input_video=str(tmp_path / "f.pt")), 4, 4)
    try:
        import av                                   # noqa: F401
        import torchvision.io                       # noqa: F401
    except ImportError:
        with pytest.raises(RuntimeError, match=r"\.avi.*\.pt"):
            cli.read_input_video(str(tmp_path / "c.mp4"))


# ---- C ABI ----------------------------------------------------------------------------------------------------------------------------
def test_intake_entry_point_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "longlive_hip.h")).read()
    body = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"\bint\s+ll_pixels_u8_to_cl\s*\(([^;]*?)\)\s*;", body, flags=re.S)
    assert m and len([a for a in m.group(1).split(",") if a.strip()]) == 8
    assert "const uint8_t* px" in m.group(1) and "long long stride_t" in m.group(1)
    assert len(_lib.SIGNATURES["ll_pixels_u8_to_cl"]) == 8
    lib = _lib.load()
    assert hasattr(lib, "ll_pixels_u8_to_cl") and _lib.ABI_VERSION == 111 == lib.ll_version()
    version_comment = header[header.index("ABI version of this header"):header.index("#define LL_ABI_VERSION")]
    assert "ll_pixels_u8_to_cl" in version_comment


@pytest.mark.parametrize("call,needle", [
    (lambda L: L.ll_pixels_u8_to_cl(0, 192, 16, 1, 8, 8, 8, None), "ll_pixels_u8_to_cl: null operand"),
    (lambda L: L.ll_pixels_u8_to_cl(16, 192, 0, 1, 8, 8, 8, None), "ll_pixels_u8_to_cl: null operand"),
    (lambda L: L.ll_pixels_u8_to_cl(16, 192, 16, 1, 8, 8, 12, None), "Cpad=12"),
    (lambda L: L.ll_pixels_u8_to_cl(16, 192, 16, 0, 8, 8, 8, None), "empty input"),
    (lambda L: L.ll_pixels_u8_to_cl(16, 191, 16, 2, 8, 8, 8, None), "stride_t=191"),
])
def test_intake_rejects_bad_arguments_before_launch(call, needle):
    lib = _lib.load()
    rc = call(lib)
    assert rc == -1, rc
    msg = lib.ll_last_error().decode()
    assert needle in msg, msg


def test_intake_wrappers_refuse_host_tensors():
    from longlive_amd import ops
    from longlive_amd.vae import WanVAEWrapper
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.pixels_u8_to_cl(torch.zeros(1, 8, 8, 3, dtype=torch.uint8))
    vae = WanVAEWrapper(device="cpu")
    with pytest.raises(RuntimeError, match="no CPU path"):
        vae.encode_frames_to_latent(torch.zeros(1, 1, 8, 8, 3, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="uint8 frames"):
        vae.encode_frames_to_latent(torch.zeros(1, 3, 1, 8, 8))
