"""Host launch trace of longlive_amd/vae.py: the real WanVAEDecoderHIP / WanVAEEncoderHIP run on CPU tensors through their public
methods with every `ops` function they call replaced by a recorder, so what is pinned is the host logic alone -- which launches, in
which order, on which views, and which launch produced every frame a launch reads.  No device and no built library are needed.

Provenance stamps: every output a recorder writes is filled with a value of its own (a bf16 bit pattern, so copies, views and
permutes keep it exactly); the parameters are stamped the same way, by name.  A recorder then notes, per frame of every bf16 operand,
the stamp it finds: a parameter's name, the number of the output that frame came from, or 0 for zeros (the start of a stream).  The
torch operations that are device work (copies, fills, concatenations; not views, not `empty`) are interleaved with their shapes.

  python tests/vae_trace.py --dump FILE [--vae OTHER_VAE_PY]     # the full trace, to diff two versions of vae.py call by call
"""
import contextlib
import hashlib
import inspect
import json
import os
import sys

import torch
from torch.utils._python_dispatch import TorchDispatchMode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

bf16 = torch.bfloat16
STAMP0 = 0x3F80                 # stamp s is the bf16 with bits STAMP0 + s (1.0 and up: finite, positive, distinct); 0 stays 0.0
OPS = ["conv_cl", "conv_cl_rms", "conv_cl_rms_ok", "rms_silu_cl", "gemm", "softmax_rows", "vae_unscale_cl", "cl_to_tchw_clamp",
       "cl_to_frames_u8", "conv_cl_down", "conv_cl_tdown", "pixels_to_cl", "pixels_u8_to_cl", "vae_scale_tchw"]
TORCH_WORK = {"copy_", "zero_", "zeros", "fill_", "clone", "cat", "stack", "_to_copy"}
SETTINGS = ("rms_ok_cout96", "rms_ok_never", "LL_VAE_FUSE=0")


def use_vae_source(path: str):
    """Loads another version of vae.py (a saved copy of an earlier commit's) as longlive_amd.vae, against the same ops and library."""
    import importlib.util
    import longlive_amd
    spec = importlib.util.spec_from_file_location("longlive_amd.vae", path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules["longlive_amd.vae"] = mod
    spec.loader.exec_module(mod)
    longlive_amd.vae = mod
    return mod


class Recorder(TorchDispatchMode):
    def __init__(self, rms_ok):
        super().__init__()
        self.trace, self.names, self.next_stamp, self.quiet, self.rms_ok = [], {}, 1, 0, rms_ok

    # -- stamps ----------------------------------------------------------------------------------------------------
    def stamp(self, t: torch.Tensor, name=None) -> int:
        s, self.next_stamp = self.next_stamp, self.next_stamp + 1
        if name is not None:
            self.names[s] = name
        self.quiet += 1
        if t.dtype == bf16:
            t.view(torch.int16).fill_(STAMP0 + s)
        else:
            t.fill_(s % 251)                      # fp32 / uint8 results leave through torch.cat: nothing reads them back
        self.quiet -= 1
        return s - self.first_out + 1 if name is None else s

    def _label(self, bits: int):
        if bits == 0:
            return 0
        s = bits - STAMP0
        return self.names[s] if s in self.names else s - self.first_out + 1

    def _found(self, t: torch.Tensor):
        """Per frame (4-D operands) or for the whole operand: the stamp of its first and of its last element, once when they agree."""
        if t.dtype != bf16 or t.numel() == 0:
            return None
        out = []
        for f in (t if t.dim() == 4 else [t]):
            flat = f.reshape(-1).view(torch.int16)
            a, b = self._label(int(flat[0])), self._label(int(flat[-1]))
            out.append(a if a == b else [a, b])
        return out

    def _describe(self, v, written=False):
        if isinstance(v, torch.Tensor):
            d = {"shape": list(v.shape), "offset": v.storage_offset(), "dtype": str(v.dtype).replace("torch.", ""),
                 "contiguous": v.is_contiguous()}
            if not written:                       # (what an output operand holds before the launch is whatever `empty` found)
                self.quiet += 1
                d["from"] = self._found(v)
                self.quiet -= 1
            return d
        if isinstance(v, (tuple, list)):
            return [self._describe(u) for u in v]
        return v if isinstance(v, (bool, int, str, type(None))) else round(float(v), 9)

    # -- ll calls --------------------------------------------------------------------------------------------------
    def stub(self, name: str, real):
        sig = inspect.signature(real)
        body = getattr(self, "_" + name)

        def call(*a, **k):
            b = sig.bind(*a, **k)
            b.apply_defaults()
            row = {"ll": name, "args": {n: self._describe(v, n in ("out", "out_rms")) for n, v in b.arguments.items()}}
            self.trace.append(row)
            outs = body(**b.arguments)
            ret, written = outs if isinstance(outs, tuple) else (outs, [outs])
            row["wrote"] = [self.stamp(t) for t in written if isinstance(t, torch.Tensor)]
            return ret
        return call

    @staticmethod
    def _new(like, *shape, dtype=bf16):
        return torch.empty(*shape, dtype=dtype, device=like.device)

    def _conv_shape(self, x, geo, upsample=False):
        cin, cout, kpad, kt, kh = geo
        T = x.shape[0] - (2 if kt > 1 else 0)
        assert T >= 1 and x.shape[3] == cin and x.is_contiguous(), (tuple(x.shape), geo)
        return (T, x.shape[1] << upsample, x.shape[2] << upsample, cout)

    def _conv_cl(self, x, packed, bias, geo, upsample, res, out):
        shape = self._conv_shape(x, geo, upsample)
        out = self._new(x, *shape) if out is None else out
        assert tuple(out.shape) == shape and (res is None or res.shape == out.shape)
        return out

    def _conv_cl_rms_ok(self, geo, H, W, upsample):
        return bool(self.rms_ok(geo)), []

    def _conv_cl_rms(self, x, packed, bias, geo, gamma, out_rms, silu, upsample, res, want_raw):
        assert self.rms_ok(geo), "conv_cl_rms where conv_cl_rms_ok said no"
        shape = self._conv_shape(x, geo, upsample)
        assert tuple(out_rms.shape) == shape and out_rms.is_contiguous() and (res is None or tuple(res.shape) == shape)
        raw = self._new(x, *shape) if want_raw else None
        return raw, [raw, out_rms]

    def _rms_silu_cl(self, x, gamma, silu, out):
        assert gamma.numel() == x.shape[-1]
        out = torch.empty_like(x) if out is None else out
        assert out.shape == x.shape and out.is_contiguous()
        return out

    def _gemm(self, x, w, bias, epilogue, out, res, **rest):
        N, K = w.shape
        assert x.shape[-1] == K and bias.numel() == N and x.is_contiguous() and w.is_contiguous()
        out = self._new(x, *x.shape[:-1], N) if out is None else out
        assert out.numel() == x.numel() // K * N and out.is_contiguous()
        return out

    def _softmax_rows(self, s, scale, n_valid, out):
        return torch.empty_like(s) if out is None else out

    def _vae_unscale_cl(self, z, mean, inv_std):
        T, C, h, w = z.shape
        assert z.is_contiguous()
        return self._new(z, T, h, w, C)

    def _cl_to_tchw_clamp(self, x):
        T, H, W, C = x.shape
        return self._new(x, T, 3, H, W, dtype=torch.float32)

    def _cl_to_frames_u8(self, x, out):
        T, H, W, C = x.shape
        return self._new(x, T, H, W, 3, dtype=torch.uint8) if out is None else out

    def _down(self, kind, x, geo, out):
        cin, cout, kpad, kt, kh = geo
        assert (kt, kh) == ((3, 1) if kind else (1, 3)) and x.shape[3] == cin and x.is_contiguous()
        T, H, W = x.shape[0] - kind, x.shape[1], x.shape[2]
        assert T >= 1
        shape = (T // 2, H, W) if kind else (T, H // 2, W // 2)
        out = self._new(x, *shape, cout) if out is None else out
        assert tuple(out.shape[:3]) == shape and out.shape[3] >= cout and out.is_contiguous()
        return out

    def _conv_cl_down(self, x, packed, bias, geo, out):
        return self._down(0, x, geo, out)

    def _conv_cl_tdown(self, x, packed, bias, geo, out):
        return self._down(1, x, geo, out)

    def _pixels_to_cl(self, px, channel_dim, cpad, out):
        shape = (px.shape[1 - channel_dim], px.shape[2], px.shape[3], cpad)
        out = self._new(px, *shape) if out is None else out
        assert tuple(out.shape) == shape and out.is_contiguous()
        return out

    def _pixels_u8_to_cl(self, frames, cpad, out):
        shape = (*frames.shape[:3], cpad)
        out = self._new(frames, *shape) if out is None else out
        assert tuple(out.shape) == shape and out.is_contiguous()
        return out

    def _vae_scale_tchw(self, mu, mean, inv_std):
        T, h, w, ld = mu.shape
        return self._new(mu, T, mean.numel(), h, w, dtype=torch.float32)

    # -- torch device work -----------------------------------------------------------------------------------------
    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        out = func(*args, **(kwargs or {}))
        name = func._schema.name.split("::")[-1]
        if not self.quiet and self.tracing and name in TORCH_WORK:
            flat = [a for arg in args for a in (arg if isinstance(arg, (list, tuple)) else [arg])]
            self.trace.append({"torch": name, "in": [list(a.shape) for a in flat if isinstance(a, torch.Tensor)],
                               "out": list(out.shape) if isinstance(out, torch.Tensor) else None})
        return out


@contextlib.contextmanager
def _host_only(rec: Recorder, env_fuse):
    """ops -> recorders, _lib.load -> raises, Tensor.is_cuda -> True, LL_VAE_FUSE as asked; all put back afterwards."""
    from longlive_amd import _lib, ops

    def no_library():
        raise RuntimeError("vae_trace: an ops function that is not stubbed reached the library")
    saved = {n: getattr(ops, n) for n in OPS}
    saved_load, saved_env = _lib.load, os.environ.get("LL_VAE_FUSE")
    try:
        for n in OPS:
            setattr(ops, n, rec.stub(n, saved[n]))
        _lib.load = no_library
        torch.Tensor.is_cuda = property(lambda self: True)
        os.environ.pop("LL_VAE_FUSE", None)
        if env_fuse is not None:
            os.environ["LL_VAE_FUSE"] = env_fuse
        yield
    finally:
        for n in OPS:
            setattr(ops, n, saved[n])
        _lib.load = saved_load
        del torch.Tensor.is_cuda
        os.environ.pop("LL_VAE_FUSE", None)
        if saved_env is not None:
            os.environ["LL_VAE_FUSE"] = saved_env


def _stamped_state_dict(rec: Recorder, shapes):
    sd = {}
    for name, shape in shapes.items():
        sd[name] = torch.empty(shape, dtype=bf16)
        rec.stamp(sd[name], name)
    return sd


def _decoder_calls(vae_mod, cfg):
    from longlive_amd import synth
    m = vae_mod.WanVAEDecoderHIP(cfg, device="cpu", chunk=2)
    z = torch.zeros(4, 16, 2, 4, dtype=bf16)
    return m, synth.vae_decoder_param_shapes(cfg), [lambda: m.decode(z), lambda: m.decode(z[:2], keep_cache=True),
                                                    lambda: m.decode(z[:1], keep_cache=True, frames="uint8")]


def _encoder_calls(vae_mod, cfg):
    from longlive_amd import synth
    m = vae_mod.WanVAEEncoderHIP(cfg, device="cpu", chunk=4)
    px = torch.zeros(3, 9, 16, 32)
    u8 = torch.zeros(4, 16, 32, 3, dtype=torch.uint8)
    return m, synth.vae_encoder_param_shapes(cfg), [lambda: m.encode(px), lambda: m.encode(px[:, :5], keep_cache=True),
                                                    lambda: m.encode(u8, keep_cache=True)]


SCENARIOS = {"decoder": _decoder_calls, "encoder": _encoder_calls}


def run(scenario: str, setting: str):
    """The trace (a list of rows) of one scenario under one setting."""
    from longlive_amd import synth
    import longlive_amd.vae as vae_mod
    assert setting in SETTINGS
    rec = Recorder((lambda geo: geo[1] == 96) if setting == "rms_ok_cout96" else (lambda geo: False))
    rec.tracing, rec.first_out = False, 0
    with _host_only(rec, "0" if setting == "LL_VAE_FUSE=0" else None), rec:
        m, shapes, calls = SCENARIOS[scenario](vae_mod, synth.VaeConfig())
        m.load_state_dict(_stamped_state_dict(rec, shapes))
        rec.first_out = rec.next_stamp
        calls[0]()                                # untraced: the one-time weight packing happens here
        rec.trace.clear()
        rec.tracing = True
        for i, call in enumerate(calls):
            rec.trace.append({"call": i})
            out = call()
            rec.trace.append({"returned": list(out.shape), "dtype": str(out.dtype).replace("torch.", "")})
    return rec.trace


def canonical(trace) -> str:
    return json.dumps(trace, sort_keys=True, separators=(",", ":"))


def summary(trace) -> dict:
    counts = {}
    for row in trace:
        key = row.get("ll") or ("torch." + row["torch"] if "torch" in row else None)
        if key:
            counts[key] = counts.get(key, 0) + 1
    return {"counts": dict(sorted(counts.items())), "sha256": hashlib.sha256(canonical(trace).encode()).hexdigest()}


def all_summaries() -> dict:
    return {sc: {st: summary(run(sc, st)) for st in SETTINGS} for sc in SCENARIOS}


def main(argv):
    if "--vae" in argv:
        use_vae_source(argv[argv.index("--vae") + 1])
    path = argv[argv.index("--dump") + 1]
    with open(path, "w") as f:
        for sc in SCENARIOS:
            for st in SETTINGS:
                f.write(f"## {sc} / {st}\n")
                f.writelines(json.dumps(row, sort_keys=True) + "\n" for row in run(sc, st))
    print(f"{path}: written")


if __name__ == "__main__":
    main(sys.argv[1:])
