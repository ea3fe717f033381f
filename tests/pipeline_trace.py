"""What the delivery path around the pipelines does, recorded through the public API alone, so that the same module runs against any
version of the `longlive_amd` package (`use_package_source`; tools/record_pipeline_goldens.py records the goldens from the commit the
later ones are to equal).

Host half (`host_cases`, `run_host`): CausalInferencePipeline / InteractiveCausalInferencePipeline on the CPU over a recording fake
generator, fake text encoder and fake VAE, with recorders over ops.jpeg_encode / ops.jpeg_bytes and -- with profile=True -- over
torch.cuda.Event, so last_profile is the same with and without a device.  The log: every generator call (start, frames, timestep,
kv_only, prompt, recache flag), every VAE call (method, latent frames, use_cache, frames, yuv_range; clear_cache), every JPEG encode
with its quality, every fetch, every profiler event.

Device half (`schedule_cases`, `run_schedule`): the toy pipeline and VAE of tests/test_frames_out_gpu.py with the generator, the VAE's
decode methods, the JPEG ops, Stream.wait_stream / wait_event, Event.record and Tensor.record_stream wrapped (all call through).  The
log: (operation, role of the current stream, roles of the streams named); a role is the stream's index by first appearance."""
import contextlib
import hashlib
import json
import os
import sys
from types import SimpleNamespace

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FS = 4                                              # tokens per frame of the host half's 4 x 4 latents
T_NEW, NF = 9, 3                                    # a first, a steady and a last block
FORMS = {"float": {"frames": "float"}, "uint8": {"frames": "uint8"}, "jpeg": {"frames": "jpeg", "jpeg_quality": 75},
         "yuv420": {"frames": "yuv420", "yuv_range": "full"}}
ENTRIES = ("inference", "stream", "stream_video", "interactive")
BAD_FORMS = [{"frames": "rgb"}, {"frames": None}, {"frames": "jpeg", "jpeg_quality": 0}, {"frames": "jpeg", "jpeg_quality": 101},
             {"frames": "jpeg", "jpeg_quality": True}, {"frames": "jpeg", "jpeg_quality": 7.5}, {"frames": "yuv420", "yuv_range": "tv"},
             {"frames": "yuv420", "yuv_range": None}]


def use_package_source(root: str):
    """Imports `longlive_amd` from `root` (a checkout of another commit, or a copy of its package) instead of this tree's."""
    for name in [m for m in sys.modules if m == "longlive_amd" or m.startswith("longlive_amd.")]:
        del sys.modules[name]
    sys.path.insert(0, os.path.abspath(root))
    import longlive_amd
    assert os.path.abspath(longlive_amd.__file__).startswith(os.path.abspath(root)), longlive_amd.__file__
    return longlive_amd


def canonical(doc):
    """`doc` as it comes back from a JSON file (tuples are lists there)."""
    return json.loads(json.dumps(doc))


def _args(gs=True):
    return SimpleNamespace(model_kwargs=SimpleNamespace(local_attn_size=12, sink_size=3, timestep_shift=5.0),
                           denoising_step_list=[1000, 750, 500, 250], warp_denoising_step=True, num_frame_per_block=NF,
                           context_noise=0, global_sink=gs)


def _call(P, entry, noise, prefix, form, profile=False):
    """One run of an entry point; the switch of the interactive one falls on the second generated block."""
    n = 0 if prefix is None else prefix.shape[1]
    kw = dict(form, initial_latent=prefix)
    if entry == "inference":
        return P.inference(noise, ["p0"], profile=profile, **kw)
    if entry == "interactive":
        return P.inference(noise, text_prompts_list=[["p0"], ["p1"]], switch_frame_indices=[n + NF], profile=profile, **kw)
    if entry == "stream":
        return list(P.stream(noise, ["p0"], initial_latent=prefix))
    return list(P.stream_video(noise, ["p0"], **kw))


# ---- host half ----------------------------------------------------------------------------------------------------------------------
class RecordingGenerator(nn.Module):
    """tests/test_continue_host.py's fake, logging into the shared log."""
    supports_kv_only = True

    def __init__(self, log):
        super().__init__()
        from oracle import ref_ops as R
        self.scheduler, self.log = R.FlowMatchSchedulerRef(5.0), log
        self.model = SimpleNamespace(num_frame_per_block=1, local_attn_size=-1, max_attention_size=0, block_mask=None,
                                     named_modules=lambda: [], _prepare_blockwise_causal_attn_mask=lambda **kw: None)

    def get_scheduler(self):
        return self.scheduler

    def forward(self, noisy_image_or_video, conditional_dict, timestep, kv_cache=None, crossattn_cache=None, current_start=None,
                sink_recache_after_switch=False, kv_only=False, **kw):
        x = noisy_image_or_video
        ts = set(round(float(v), 4) for v in timestep.flatten().tolist())
        assert len(ts) == 1 and current_start % FS == 0
        self.log.append(("gen", current_start // FS, int(x.shape[1]), ts.pop(), bool(kv_only), conditional_dict["name"],
                         bool(sink_recache_after_switch)))
        x0 = (0.5 * x.float() + 0.01 * (len(self.log) % 7)).to(x.dtype)
        return x0, x0


class RecordingVAE:
    """The three methods of WanVAEWrapper the pipelines call, with its signatures; outputs have the shapes of 8 x 8 pixel latents."""

    def __init__(self, log):
        self.log = log
        self.model = SimpleNamespace(clear_cache=lambda: log.append(("vae", "clear_cache")))

    def decode_to_pixel(self, latent, use_cache=False):
        self.log.append(("vae", "decode_to_pixel", int(latent.shape[1]), bool(use_cache), None, None))
        return torch.zeros(latent.shape[0], 4 * latent.shape[1], 3, 8, 8)

    def decode_to_frames(self, latent, use_cache=False, frames="uint8", yuv_range="limited"):
        self.log.append(("vae", "decode_to_frames", int(latent.shape[1]), bool(use_cache), frames, yuv_range))
        shape = (8, 8, 3) if frames == "uint8" else (96,)
        return torch.zeros(latent.shape[0], 4 * latent.shape[1], *shape, dtype=torch.uint8)


class _FakeEvent:
    log = None

    def __init__(self, enable_timing=False):
        pass

    def record(self, stream=None):
        self.log.append(("event",))

    def elapsed_time(self, other):
        return 1.0


@contextlib.contextmanager
def _host_patches(log, profile):
    from longlive_amd import ops
    saved = ops.jpeg_encode, ops.jpeg_bytes, torch.cuda.Event, torch.cuda.is_available, torch.cuda.synchronize

    def jpeg_encode(frames, quality=90):
        log.append(("jpeg_encode", list(frames.shape), quality))
        return frames, frames.shape[0]

    def jpeg_bytes(buf, sizes):
        log.append(("fetch", int(sizes)))
        return [b"jpeg"] * int(sizes)
    try:
        ops.jpeg_encode, ops.jpeg_bytes = jpeg_encode, jpeg_bytes
        if profile:                                 # the profiler runs (on fake events) whether or not there is a device
            _FakeEvent.log = log
            torch.cuda.Event, torch.cuda.is_available, torch.cuda.synchronize = _FakeEvent, (lambda: True), (lambda *a: None)
        yield
    finally:
        ops.jpeg_encode, ops.jpeg_bytes, torch.cuda.Event, torch.cuda.is_available, torch.cuda.synchronize = saved


def _host_pipe(entry, log):
    import trace_driver as TD
    from longlive_amd.pipeline import CausalInferencePipeline, InteractiveCausalInferencePipeline

    def encoder(text_prompts):
        log.append(("text", text_prompts[0]))
        return {"prompt_embeds": torch.zeros(1, 1), "name": text_prompts[0]}
    cls = InteractiveCausalInferencePipeline if entry == "interactive" else CausalInferencePipeline
    P = cls(_args(gs=False), "cpu", generator=RecordingGenerator(log), text_encoder=encoder, vae=RecordingVAE(log))
    P.num_transformer_blocks, P.frame_seq_length = 2, FS
    P.randn_like = TD.HashRandn(5)
    return P


def host_cases():
    """entry / form / prefix / profile; `stream` takes no form, and only the two `inference`s profile."""
    out = []
    for entry in ENTRIES:
        for form in (("-",) if entry == "stream" else FORMS):
            for n in (0, 4):
                for profile in ((False, True) if entry in ("inference", "interactive") else (False,)):
                    out.append(f"{entry}/{form}/prefix{n}/{'profile' if profile else 'plain'}")
    return out


def _host_inputs(n):
    from longlive_amd import synth
    cfg = synth.WanConfig(lat_h=4, lat_w=4)
    return synth.synth_noise(cfg, T_NEW, seed=3), (synth.synth_noise(cfg, n, seed=9, name="prefix") if n else None)


def _describe(result):
    """Shapes and types of what an entry point handed back (the values are the fakes')."""
    if torch.is_tensor(result):
        return [str(result.dtype).replace("torch.", ""), list(result.shape)]
    if isinstance(result, (list, tuple)):
        return [_describe(r) for r in result]
    return result.decode() if isinstance(result, bytes) else result


def run_host(case: str):
    entry, form, prefix, how = case.split("/")
    log, profile = [], how == "profile"
    noise, pre = _host_inputs(int(prefix[len("prefix"):]))
    with _host_patches(log, profile):
        P = _host_pipe(entry, log)
        result = _call(P, entry, noise, pre, FORMS.get(form, {}), profile)
        doc = {"log": log, "returned": _describe(result)}
        if profile:
            rep = P.last_profile
            doc["last_profile"] = {"keys": sorted(rep), "phases": sorted(rep["times_ms"]), "blocks": len(rep["block_times_ms"]),
                                   "switch_blocks": rep["switch_blocks"]}
    return canonical(doc)


def run_refusal(entry: str, bad: dict):
    """(the error, the log) of an entry point given a bad form: the log is to be empty."""
    log = []
    noise, pre = _host_inputs(4)
    with _host_patches(log, False):
        P = _host_pipe(entry, log)
        try:
            _call(P, entry, noise, pre, bad)
        except ValueError as exc:
            return exc, log
    return None, log


# ---- device half --------------------------------------------------------------------------------------------------------------------
SCHED_ENTRIES = ("stream_video", "inference", "interactive")


def schedule_cases(entry):
    return [f"{entry}/{form}/prefix{n}/{'overlap' if ov else 'serial'}" for form in ("float", "jpeg", "yuv420") for n in (0, 4)
            for ov in (False, True)]


def make_toy(dev="cuda"):
    """The toy generator, encoder and VAE of tests/test_frames_out_gpu.py, and the inputs of every case."""
    import test_model_gpu as TM
    from longlive_amd import synth
    from longlive_amd.vae import WanVAEWrapper
    cfg, gen, enc = TM._pipe_generator()
    vae = WanVAEWrapper(device=dev, chunk=2)
    vae.load_state_dict(synth.synth_vae_state_dict(synth.VaeConfig(), seed=5))
    noise = synth.synth_noise(cfg, T_NEW, seed=41, device=dev)
    prefix = synth.synth_noise(cfg, 4, seed=9, name="prefix", device=dev)
    return SimpleNamespace(TM=TM, gen=gen, enc=enc, vae=vae, noise=noise, prefix=prefix, dev=dev)


class _Roles:
    def __init__(self):
        self.log, self.streams, self.events = [], {}, {}

    def stream(self, s):
        return None if s is None else self.streams.setdefault(s.cuda_stream, len(self.streams))

    def event(self, e):
        return self.events.setdefault(id(e), len(self.events))

    def note(self, op, *more):
        self.log.append([op, self.stream(torch.cuda.current_stream()), *more])


@contextlib.contextmanager
def _schedule_patches(toy, R: _Roles):
    from longlive_amd import ops
    S, E = torch.cuda.Stream, torch.cuda.Event
    saved = (toy.gen.forward, toy.vae.decode_to_pixel, toy.vae.decode_to_frames, ops.jpeg_encode, ops.jpeg_bytes, S.wait_stream,
             S.wait_event, E.record)
    gen_forward, to_pixel, to_frames, encode, fetch, wait_stream, wait_event, record = saved
    keep = []                                       # events stay alive while their ids are in use

    def forward(*a, **k):
        R.note("generator", int(k["current_start"]), bool(k.get("kv_only", False)))
        return gen_forward(*a, **k)

    def decode_to_pixel(latent, use_cache=False):
        R.note("decode_to_pixel", int(latent.shape[1]), bool(use_cache))
        return to_pixel(latent, use_cache=use_cache)

    def decode_to_frames(latent, use_cache=False, frames="uint8", yuv_range="limited"):
        R.note("decode_to_frames", int(latent.shape[1]), bool(use_cache), frames, yuv_range)
        return to_frames(latent, use_cache=use_cache, frames=frames, yuv_range=yuv_range)

    def jpeg_encode(frames, quality=90):
        R.note("jpeg_encode", int(frames.shape[0]), quality)
        return encode(frames, quality)

    def jpeg_bytes(buf, sizes):
        R.note("fetch")
        return fetch(buf, sizes)

    def s_wait_stream(self, other):
        R.note("wait_stream", R.stream(self), R.stream(other))
        return wait_stream(self, other)

    def s_wait_event(self, event):
        keep.append(event)
        R.note("wait_event", R.stream(self), R.event(event))
        return wait_event(self, event)

    def e_record(self, stream=None):
        keep.append(self)
        R.note("record", R.stream(torch.cuda.current_stream() if stream is None else stream), R.event(self))
        return record(self, stream) if stream is not None else record(self)

    def t_record_stream(self, stream):
        R.note("record_stream", R.stream(stream))
        return torch._C.TensorBase.record_stream(self, stream)
    try:
        toy.gen.forward, toy.vae.decode_to_pixel, toy.vae.decode_to_frames = forward, decode_to_pixel, decode_to_frames
        ops.jpeg_encode, ops.jpeg_bytes = jpeg_encode, jpeg_bytes
        S.wait_stream, S.wait_event, E.record = s_wait_stream, s_wait_event, e_record
        torch.Tensor.record_stream = t_record_stream
        yield
    finally:
        del toy.gen.forward, toy.vae.decode_to_pixel, toy.vae.decode_to_frames, torch.Tensor.record_stream
        ops.jpeg_encode, ops.jpeg_bytes, S.wait_stream, S.wait_event, E.record = saved[3:]


def _sha(result) -> str:
    h = hashlib.sha256()

    def feed(r):
        if torch.is_tensor(r):
            h.update(r.contiguous().cpu().view(torch.uint8).numpy().tobytes())
        elif isinstance(r, bytes):
            h.update(r)
        elif isinstance(r, (list, tuple)):
            for u in r:
                feed(u)
        else:
            h.update(repr(r).encode())
    feed(result)
    return h.hexdigest()


def run_schedule(toy, case: str):
    """{"log", "sha256"} of one case, on a pipeline of its own: the streams a case makes are then drawn from the pool one after the
    other, so no two of them share a handle."""
    from longlive_amd.pipeline import CausalInferencePipeline, InteractiveCausalInferencePipeline
    entry, form, prefix, how = case.split("/")
    cls = InteractiveCausalInferencePipeline if entry == "interactive" else CausalInferencePipeline
    P = cls(toy.TM._pipe_args(), toy.dev, generator=toy.gen, text_encoder=toy.enc, vae=toy.vae)
    P.randn_like = toy.TM.TD.HashRandn(43)
    P.overlap_decode = how == "overlap"
    form = dict(FORMS[form], **({"overlap_decode": how == "overlap"} if entry == "stream_video" else {}))
    R = _Roles()
    R.stream(torch.cuda.current_stream())           # role 0: the caller's stream
    with _schedule_patches(toy, R):
        result = _call(P, entry, toy.noise, toy.prefix if prefix == "prefix4" else None, form)
    torch.cuda.synchronize()
    return canonical({"log": R.log, "sha256": _sha(result)})
