"""Host call trace of longlive_amd/ops.py: every public wrapper, and CausalWanModelHIP.forward_frames over them, run on CPU tensors
against a recording fake of liblonglive_hip.so, so what is pinned is the checking layer alone -- which entry a call reaches, with which
integers, floats and pointers, under which timer tag and work value, what it returns and what it refuses.  No device and no built
library are needed.  tools/record_ops_goldens.py records tests/golden/ops_call_trace.json from the commit later ones are to equal;
tests/test_ops_trace_host.py holds the working tree to it.

A row per library call: [entry, args] with integers as they are, floats rounded to 9 places, null pointers 0, pointers into a case's
named inputs "name+byte_offset" (offset from the start of that input's storage), pointers into tensors the wrapper allocated
"new<k>+byte_offset" (k by first appearance), plan buffers "buf", byref arguments "ref"; entries that answer a question carry the
answer.  After a launch the timer row ["timer", tag, work]; after the call what came back (shape, dtype, strides, label per tensor)
or ["raises", type, message].

  python tests/ops_trace.py --dump FILE [--source DIR]     # every row of every case, to diff two versions of the package
"""
import contextlib
import ctypes
import functools
import hashlib
import inspect
import json
import os
import sys

import numpy as np
import torch
from torch.utils._python_dispatch import TorchDispatchMode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from pipeline_trace import use_package_source  # noqa: E402,F401  (the recorder imports the package of another commit through it)

bf16, f32, i8, u8, i32 = torch.bfloat16, torch.float32, torch.int8, torch.uint8, torch.int32

# Public functions that never reach the library: arithmetic and views on the host.  Everything else must be exercised by a case.
HOST_ONLY = {
    "yuv420_bytes": "arithmetic", "yuv_chroma_shape": "arithmetic", "cover_window": "arithmetic", "resize_taps": "numpy tables",
    "yuv420_planes": "views of a buffer", "pack_conv_weight": "torch repacking at load", "jpeg_bytes": "host read of the encoder's buffers",
    "png_bytes": "jpeg_bytes under its other name",
}
# Entries of _lib.SIGNATURES that neither ops.py nor model.py calls (bench.py, tools, synth.py and the tests call them on the library).
NEVER_CALLED = ("ll_version", "ll_last_error", "ll_set_tuning", "ll_gemm_plan", "ll_gemm_plan_epi", "ll_flash_attn_plan", "ll_synth_hash",
                "ll_jpeg_decode_pixels")
ANSWERS = {"ll_gemm_ksplit_plan": 0, "ll_gemm_ksplit_workspace_bytes": 4096, "ll_gemm_ssq_planes": 0, "ll_flash_attn_q_ok": 0,
           "ll_flash_attn_qnorm_ok": 0, "ll_conv_cl_rms_ok": 0}
SIZES = {"ll_jpeg_sizes": (4096, 8192), "ll_png_sizes": (2048, 1024), "ll_zlib_sizes": (512, 256), "ll_jpeg_decode_sizes": (1024, 2048),
         "ll_jpeg_decode_split_sizes": (4096,)}
STATUS_ARG = {"ll_jpeg_decode_coefficients": 13, "ll_jpeg_decode_coefficients_split": 13, "ll_jpeg_decode_u8": 14, "ll_jpeg_decode_u8_split": 14}


def public_functions(ops):
    """name -> callable for every public function of ops (its own functions and the names bound over shared bodies)."""
    return {n: f for n, f in sorted(vars(ops).items()) if not n.startswith("_") and callable(f) and not inspect.isclass(f)
            and (isinstance(f, functools.partial) or getattr(f, "__module__", None) == ops.__name__)}


class Trace(TorchDispatchMode):
    """The rows of one case; as a dispatch mode it sends allocations on a device to the host and keeps every new storage alive, so
    that an address names one tensor for the whole case."""

    def __init__(self, inputs, answers):
        super().__init__()
        self.rows, self.answers, self.events = [], dict(ANSWERS, **(answers or {})), 0
        self.named, self.fresh, self.fresh_at, self.numbered = [], [], {}, {}
        for name, t in inputs.items():
            if isinstance(t, torch.Tensor) and t.numel():
                st = t.untyped_storage()
                self.named.append((st.data_ptr(), st.nbytes(), name, st))

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        kwargs = dict(kwargs or {})
        if kwargs.get("device") is not None and torch.device(kwargs["device"]).type == "cuda":
            kwargs["device"] = torch.device("cpu")
        out = func(*args, **kwargs)
        for t in (out if isinstance(out, (tuple, list)) else [out]):
            if isinstance(t, torch.Tensor) and t.numel():
                st = t.untyped_storage()
                if st.data_ptr() not in self.fresh_at:
                    self.fresh_at[st.data_ptr()] = len(self.fresh)
                    self.fresh.append((st.data_ptr(), st.nbytes(), st))
        return out

    def label(self, p):
        if not p:
            return 0
        for base, n, name, _ in self.named:
            if base <= p < base + n:
                return f"{name}+{p - base}"
        k = self.fresh_at.get(p)
        if k is None:
            k = next((i for i, (base, n, _) in enumerate(self.fresh) if base <= p < base + n), None)
        assert k is not None, f"a pointer {p:#x} into nothing this case made"
        base = self.fresh[k][0]
        return f"new{self.numbered.setdefault(base, len(self.numbered))}+{p - base}"

    def describe(self, v):
        if isinstance(v, torch.Tensor):
            return {"shape": list(v.shape), "dtype": str(v.dtype).replace("torch.", ""), "strides": list(v.stride()),
                    "at": self.label(v.data_ptr()) if v.numel() else 0}
        if isinstance(v, (tuple, list)):
            return [self.describe(u) for u in v]
        if isinstance(v, dict):
            return {k: self.describe(u) for k, u in sorted(v.items())}
        return v if isinstance(v, (bool, int, str, type(None))) else round(float(v), 9)


class FakeLibrary:
    def __init__(self, trace: Trace, signatures):
        self._trace, self._sig = trace, signatures

    def __getattr__(self, entry):
        if not entry.startswith("ll_"):
            raise AttributeError(entry)
        argtypes = self._sig[entry]
        tr = self._trace

        def call(*args):
            assert len(args) == len(argtypes), f"{entry}: {len(args)} arguments for {len(argtypes)}"
            row = []
            for a, ty in zip(args, argtypes):
                if ty is ctypes.c_void_p:
                    row.append(tr.label(a))
                elif ty is ctypes.c_char_p:
                    a.value = f"plan of {entry}".encode()
                    row.append("buf")
                elif ty is ctypes.c_float:
                    row.append(round(float(a), 9))
                elif ty in (ctypes.c_int, ctypes.c_longlong, ctypes.c_uint, ctypes.c_ulonglong):
                    assert isinstance(a, int) and not isinstance(a, bool), f"{entry}: {a!r} where the ABI takes an integer"
                    row.append(a)
                else:
                    row.append("ref")
            if entry in SIZES:
                refs = [a for a, ty in zip(args, argtypes) if ty not in (ctypes.c_int, ctypes.c_longlong)]
                for ref, value in zip(refs, SIZES[entry]):
                    ref._obj.value = value
            if entry in STATUS_ARG:                 # the segments' status words, which `check` reads back
                nseg = args[3]
                words = (tr.answers.get("jpeg_status") or [0] * nseg)[:nseg]
                ctypes.memmove(args[STATUS_ARG[entry]], (ctypes.c_int32 * nseg)(*words), 4 * nseg)
            if entry in tr.answers:
                tr.rows.append([entry, row, tr.answers[entry]])
                return tr.answers[entry]
            tr.rows.append([entry, row])
            return 0
        return call


class _Timer:
    def __init__(self, trace):
        self.trace = trace

    def begin(self, tag):
        return tag

    def end(self, tag, start, work):
        assert start == tag
        self.trace.rows.append(["timer", tag, float(work)])


class _Stream:
    cuda_stream = 0

    def wait_event(self, ev):
        pass


@contextlib.contextmanager
def host_only(trace: Trace, timed: bool, used=None):
    """_lib.load -> the fake, Tensor.is_cuda -> True (but for tensors marked `_ll_cpu`), ops._stream -> 0, torch.cuda's stream, device
    and Event -> stubs, ops.timer -> a recorder or None, the wrappers' caches empty; `used` collects the public functions called.  All
    put back afterwards."""
    from longlive_amd import _lib, ops

    class Event:
        def __init__(self, *a, **k):
            trace.events += 1

        def record(self, *a):
            pass

    pub = public_functions(ops)

    def counted(name, f):
        def g(*a, **k):
            used.add(name)
            return f(*a, **k)
        return g
    saved = dict(load=_lib.load, stream=ops._stream, timer=ops.timer, cur=torch.cuda.current_stream, dev=torch.cuda.current_device,
                 event=torch.cuda.Event, lazy=torch.cuda._lazy_init)
    try:
        fake = FakeLibrary(trace, _lib.SIGNATURES)
        _lib.load = lambda: fake
        ops._stream = lambda: 0
        ops.timer = _Timer(trace) if timed else None
        torch.cuda.current_stream = lambda device=None: _Stream()
        torch.cuda.current_device = lambda: 0
        torch.cuda.Event = Event
        torch.cuda._lazy_init = lambda: None
        torch.Tensor.is_cuda = property(lambda self: not getattr(self, "_ll_cpu", False))
        ops._zero16.clear(); ops._ksplit_ws.clear(); ops._resize_tables.cache_clear()
        if used is not None:
            for n, f in pub.items():
                setattr(ops, n, counted(n, f))
        yield
    finally:
        for n, f in pub.items():
            setattr(ops, n, f)
        _lib.load, ops._stream, ops.timer = saved["load"], saved["stream"], saved["timer"]
        torch.cuda.current_stream, torch.cuda.current_device, torch.cuda.Event = saved["cur"], saved["dev"], saved["event"]
        torch.cuda._lazy_init = saved["lazy"]
        del torch.Tensor.is_cuda
        ops._zero16.clear(); ops._ksplit_ws.clear(); ops._resize_tables.cache_clear()


# ---- wrapper cases ---------------------------------------------------------------------------------------------------------------
def Z(*shape, dtype=bf16):
    return torch.zeros(*shape, dtype=dtype)


def cpu(t):
    t._ll_cpu = True
    return t


CASES = {}      # name -> (inputs factory, call(ops, inputs), answers)
ADDED = {}      # the same for names ops gained after the golden was recorded, and the recorded case whose rows each must repeat


def case(name, inputs, call, **answers):
    assert name not in CASES, name
    CASES[name] = (inputs, call, answers)


def added(name, same_as, call):
    ADDED[name] = (CASES[same_as][0], call, CASES[same_as][2], same_as)


def _lin(M=4, N=256, K=128, **more):
    return lambda: dict(x=Z(M, K), w=Z(N, K), bias=Z(N), **{k: v() for k, v in more.items()})


def _ln(**more):
    return lambda: dict(x=Z(1, 4, 256), e=Z(1, 2, 6, 256), mod=Z(6, 256), tab=Z(1, 2, 6, 256, dtype=f32), w=Z(256), b=Z(256),
                        **{k: v() for k, v in more.items()})


FORMATS = ("q8", "f8", "mx", "mx6", "mx4")
QUANTIZERS = {"q8": "quantize_rows", "f8": "quantize_rows_f8", "mx": "quantize_mx", "mx6": "quantize_mx6", "mx4": "quantize_mx4"}
GEMMS = {"w8a8": ("Q8", "Q8"), "f8": ("F8", "F8"), "mx": ("MX", "MX"), "mx6": ("MX6", "MX6"), "mx4w6": ("MX6", "MX4"), "mx4": ("MX4", "MX4")}


def _pair(o, fmt, shape):
    return getattr(o, fmt).empty(shape, torch.device("cpu"))


def _producers():
    case("ln_modulate", _ln(), lambda o, i: o.ln_modulate(i["x"], i["e"], i["mod"], 0, 1, 2, 1e-6))
    case("ln_modulate/premod,out,tag", _ln(out=lambda: Z(1, 4, 256)), lambda o, i: o.ln_modulate(i["x"], i["e"], None, 3, 4, 2, 1e-6, out=i["out"], tag="t"))
    case("ln_modulate/cpu", _ln(), lambda o, i: o.ln_modulate(cpu(i["x"]), i["e"], i["mod"], 0, 1, 2, 1e-6))
    case("ln_modulate/e dtype", _ln(), lambda o, i: o.ln_modulate(i["x"], i["e"].float(), i["mod"], 0, 1, 2, 1e-6))
    case("ln_modulate/frames", _ln(), lambda o, i: o.ln_modulate(i["x"], i["e"], i["mod"], 0, 1, 3, 1e-6))
    case("ln_modulate/mod size", _ln(), lambda o, i: o.ln_modulate(i["x"], i["e"], i["mod"][:5], 0, 1, 2, 1e-6))
    case("ln_modulate/out shape", _ln(out=lambda: Z(4, 256)), lambda o, i: o.ln_modulate(i["x"], i["e"], i["mod"], 0, 1, 2, 1e-6, out=i["out"]))
    case("ln_modulate_tab", _ln(), lambda o, i: o.ln_modulate_tab(i["x"], i["tab"], 0, 1, 2, 1e-6))
    case("ln_modulate_tab/q8", _ln(), lambda o, i: o.ln_modulate_tab(i["x"], i["tab"], 3, 4, 2, 1e-6, q8=True, tag="t"))
    added("ln_modulate_tab_q8", "ln_modulate_tab/q8", lambda o, i: o.ln_modulate_tab_q8(i["x"], i["tab"], 3, 4, 2, 1e-6, tag="t"))
    case("ln_modulate_tab/tab dtype", _ln(), lambda o, i: o.ln_modulate_tab(i["x"], i["e"], 0, 1, 2, 1e-6))
    case("ln_modulate_tab/x strided", _ln(), lambda o, i: o.ln_modulate_tab(i["x"].transpose(1, 2), i["tab"], 0, 1, 2, 1e-6))
    case("ln_modulate_tab/frames", _ln(), lambda o, i: o.ln_modulate_tab(i["x"], i["tab"], 0, 1, 1, 1e-6))
    case("layernorm_affine", _ln(), lambda o, i: o.layernorm_affine(i["x"], i["w"], i["b"], 1e-6))
    case("layernorm_affine/out", _ln(out=lambda: Z(1, 4, 256)), lambda o, i: o.layernorm_affine(i["x"], i["w"], i["b"], 1e-5, out=i["out"]))
    case("layernorm_affine/w size", _ln(), lambda o, i: o.layernorm_affine(i["x"], i["w"][:255], i["b"], 1e-6))
    case("layernorm_affine/b dtype", _ln(), lambda o, i: o.layernorm_affine(i["x"], i["w"], i["b"].float(), 1e-6))
    for f in FORMATS:
        case(f"ln_modulate_{f}", _ln(), lambda o, i, f=f: getattr(o, "ln_modulate_" + f)(i["x"], i["e"], i["mod"], 0, 1, 2, 1e-6))
        case(f"ln_modulate_{f}/premod,tag", _ln(), lambda o, i, f=f: getattr(o, "ln_modulate_" + f)(i["x"], i["e"], None, 3, 4, 2, 1e-6, tag="t"))
        case(f"ln_modulate_{f}/frames", _ln(), lambda o, i, f=f: getattr(o, "ln_modulate_" + f)(i["x"], i["e"], i["mod"], 0, 1, 3, 1e-6))
        case(f"ln_modulate_{f}/x dtype", _ln(), lambda o, i, f=f: getattr(o, "ln_modulate_" + f)(i["x"].float(), i["e"], i["mod"], 0, 1, 2, 1e-6))
        if f != "q8":
            case(f"ln_modulate_tab_{f}", _ln(), lambda o, i, f=f: getattr(o, "ln_modulate_tab_" + f)(i["x"], i["tab"], 0, 1, 2, 1e-6))
            case(f"ln_modulate_tab_{f}/frames", _ln(), lambda o, i, f=f: getattr(o, "ln_modulate_tab_" + f)(i["x"], i["tab"], 0, 1, 1, 1e-6, tag="t"))
        case(f"layernorm_affine_{f}", _ln(), lambda o, i, f=f: getattr(o, "layernorm_affine_" + f)(i["x"], i["w"], i["b"], 1e-6))
        case(f"layernorm_affine_{f}/cpu", _ln(), lambda o, i, f=f: getattr(o, "layernorm_affine_" + f)(i["x"], cpu(i["w"]), i["b"], 1e-6))
        case(f"{QUANTIZERS[f]}", _ln(), lambda o, i, f=f: getattr(o, QUANTIZERS[f])(i["x"]))
        case(f"{QUANTIZERS[f]}/strided", _ln(), lambda o, i, f=f: getattr(o, QUANTIZERS[f])(i["x"][..., :128]))
    case("quantize_rows/q,scale", _ln(q=lambda: Z(1, 4, 256, dtype=i8), scale=lambda: Z(4, dtype=f32)),
         lambda o, i: o.quantize_rows(i["x"], i["q"], i["scale"]))
    case("quantize_rows/scale size", _ln(scale=lambda: Z(3, dtype=f32)), lambda o, i: o.quantize_rows(i["x"], scale=i["scale"]))
    case("quantize_mx/tag", _ln(), lambda o, i: o.quantize_mx(i["x"], tag="t"))
    for f in ("mx6", "mx4"):      # a packed format over a K that is no multiple of 256
        case(f"quantize_{f}/K=128", lambda: dict(x=Z(4, 128)), lambda o, i, f=f: getattr(o, "quantize_" + f)(i["x"]))
        case(f"ln_modulate_{f}/C=128", lambda: dict(x=Z(1, 4, 128), e=Z(1, 2, 6, 128)),
             lambda o, i, f=f: getattr(o, "ln_modulate_" + f)(i["x"], i["e"], None, 0, 1, 2, 1e-6))
    case("modulation_table", lambda: dict(e=Z(1, 2, 6, 256), mods=Z(3, 6, 256)), lambda o, i: o.modulation_table(i["e"], i["mods"]))
    case("modulation_table/mods shape", lambda: dict(e=Z(1, 2, 6, 256), mods=Z(3, 5, 256)), lambda o, i: o.modulation_table(i["e"], i["mods"]))
    case("modulation_table_f32", lambda: dict(e=Z(1, 2, 6, 256), mods=Z(3, 6, 256)), lambda o, i: o.modulation_table_f32(i["e"], i["mods"], 0b010010))
    case("rmsnorm", lambda: dict(x=Z(2, 3, 256), w=Z(256)), lambda o, i: o.rmsnorm(i["x"], i["w"], 1e-6))
    case("rmsnorm/column slice,out", lambda: dict(x=Z(6, 768), w=Z(256), out=Z(6, 512)),
         lambda o, i: o.rmsnorm(i["x"][:, 256:512], i["w"], 1e-6, out=i["out"], C=256))
    case("rmsnorm/w size", lambda: dict(x=Z(2, 3, 256), w=Z(128)), lambda o, i: o.rmsnorm(i["x"], i["w"], 1e-6))


def _gemms():
    case("gemm", _lin(), lambda o, i: o.gemm(i["x"], i["w"], i["bias"]))
    case("gemm/3-D x,gelu,tag", lambda: dict(x=Z(2, 3, 128), w=Z(256, 128), bias=Z(256)),
         lambda o, i: o.gemm(i["x"], i["w"], i["bias"], o.EPI_BIAS_GELU, tag="t"))
    case("gemm/ksplit", _lin(), lambda o, i: o.gemm(i["x"], i["w"], i["bias"]), ll_gemm_ksplit_plan=4)
    case("gemm/ksplit,res", _lin(res=lambda: Z(4, 256)), lambda o, i: o.gemm(i["x"], i["w"], i["bias"], o.EPI_BIAS_RES, res=i["res"]),
         ll_gemm_ksplit_plan=2)
    case("gemm/ksplit not asked: gelu", _lin(), lambda o, i: o.gemm(i["x"], i["w"], i["bias"], o.EPI_BIAS_GELU), ll_gemm_ksplit_plan=4)
    case("gemm/ksplit not asked: rows", _lin(M=1025), lambda o, i: o.gemm(i["x"], i["w"], i["bias"]), ll_gemm_ksplit_plan=4)
    case("gemm/ksplit twice: one workspace", _lin(), lambda o, i: [o.gemm(i["x"], i["w"], i["bias"]), o.gemm(i["x"], i["w"], i["bias"])],
         ll_gemm_ksplit_plan=4)
    ep = dict(res=lambda: Z(4, 256), e=lambda: Z(1, 2, 6, 256), mod=lambda: Z(6, 256), out=lambda: Z(4, 256))
    case("gemm/res,out", _lin(**ep), lambda o, i: o.gemm(i["x"], i["w"], i["bias"], o.EPI_BIAS_RES, out=i["out"], res=i["res"]))
    case("gemm/gate", _lin(**ep), lambda o, i: o.gemm(i["x"], i["w"], i["bias"], o.EPI_BIAS_GATE_RES, out=i["res"], res=i["res"], e=i["e"],
                                                      mod=i["mod"], gate_idx=2, rows_per_batch=4, frame_len=2))
    case("gemm/gate,premod", _lin(**ep), lambda o, i: o.gemm(i["x"], i["w"], i["bias"], o.EPI_BIAS_GATE_RES, res=i["res"], e=i["e"],
                                                             gate_idx=5, rows_per_batch=4, frame_len=2))
    case("gemm/res missing", _lin(), lambda o, i: o.gemm(i["x"], i["w"], i["bias"], o.EPI_BIAS_RES))
    case("gemm/res size", _lin(**ep), lambda o, i: o.gemm(i["x"], i["w"], i["bias"], o.EPI_BIAS_RES, res=i["res"][:3]))
    case("gemm/e shape", _lin(**ep), lambda o, i: o.gemm(i["x"], i["w"], i["bias"], o.EPI_BIAS_GATE_RES, res=i["res"], e=i["e"], frame_len=4))
    case("gemm/mod dtype", _lin(**ep), lambda o, i: o.gemm(i["x"], i["w"], i["bias"], o.EPI_BIAS_GATE_RES, res=i["res"], e=i["e"],
                                                           mod=i["mod"].float(), frame_len=2))
    case("gemm/cpu", _lin(), lambda o, i: o.gemm(cpu(i["x"]), i["w"], i["bias"]))
    case("gemm/w dtype", _lin(), lambda o, i: o.gemm(i["x"], i["w"].float(), i["bias"]))
    case("gemm/x strided", _lin(), lambda o, i: o.gemm(i["x"][:, ::2], i["w"], i["bias"]))
    case("gemm/w shape", _lin(), lambda o, i: o.gemm(i["x"], i["w"][:, :64], i["bias"]))
    case("gemm/bias size", _lin(), lambda o, i: o.gemm(i["x"], i["w"], i["bias"][:255]))
    case("gemm/out size", _lin(out=lambda: Z(4, 128)), lambda o, i: o.gemm(i["x"], i["w"], i["bias"], out=i["out"]))
    case("gemm_ssq_planes", dict, lambda o, i: o.gemm_ssq_planes(4, 256, 128), ll_gemm_ssq_planes=2)
    case("gemm_ssq/0 planes", _lin(), lambda o, i: o.gemm_ssq(i["x"], i["w"], i["bias"]))
    case("gemm_ssq", _lin(), lambda o, i: o.gemm_ssq(i["x"], i["w"], i["bias"]), ll_gemm_ssq_planes=2)
    case("gemm_ssq/out,tag", _lin(out=lambda: Z(4, 256)), lambda o, i: o.gemm_ssq(i["x"], i["w"], i["bias"], out=i["out"], tag="t"), ll_gemm_ssq_planes=2)
    case("gemm_ssq/w shape", _lin(), lambda o, i: o.gemm_ssq(i["x"], i["w"][:, :64], i["bias"]), ll_gemm_ssq_planes=2)
    case("gemm_ssq/bias dtype", _lin(), lambda o, i: o.gemm_ssq(i["x"], i["w"], i["bias"].float()), ll_gemm_ssq_planes=2)
    case("ksplit_workspace", dict, lambda o, i: o.ksplit_workspace(torch.device("cpu"), 4, 256, 128))
    case("linear_small/19 rows", _lin(M=19), lambda o, i: o.linear_small(i["x"], i["w"], i["bias"], act_in=1, act_out=1))
    case("linear_small", _lin(M=2), lambda o, i: o.linear_small(i["x"], i["w"], i["bias"]))
    case("linear_small/bias size", _lin(M=2), lambda o, i: o.linear_small(i["x"], i["w"], i["bias"][:3]))
    case("linear_small/x dtype", _lin(M=2), lambda o, i: o.linear_small(i["x"].float(), i["w"], i["bias"]))
    t5 = dict(res=lambda: Z(4, 256), norm_w=lambda: Z(256))
    case("gemm_res_t5norm", _lin(**t5), lambda o, i: o.gemm_res_t5norm(i["x"], i["w"], i["bias"], i["res"], i["norm_w"]))
    case("gemm_res_t5norm/ksplit,eps,tag", _lin(**t5), lambda o, i: o.gemm_res_t5norm(i["x"], i["w"], i["bias"], i["res"], i["norm_w"], eps=1e-5, tag="t"),
         ll_gemm_ksplit_plan=4)
    case("gemm_res_t5norm/norm_w size", _lin(**t5), lambda o, i: o.gemm_res_t5norm(i["x"], i["w"], i["bias"], i["res"], i["norm_w"][:8]))
    case("gemm_res_t5norm/res strided", _lin(**t5), lambda o, i: o.gemm_res_t5norm(i["x"], i["w"], i["bias"], i["res"].t(), i["norm_w"]))

    def qkv(K=256):
        return lambda: dict(x=Z(1, 4, K), w=Z(768, K), bias=Z(768), cache_v=Z(1, 12, 2, 128), xi=Z(1, 4, K, dtype=i8), sx=Z(4, dtype=f32),
                            wq=Z(768, K, dtype=i8), sw=Z(768, dtype=f32))
    case("gemm_qkv_v_insert", qkv(), lambda o, i: o.gemm_qkv_v_insert(i["x"], i["w"], i["bias"], i["cache_v"], 8, 0, 4))
    case("gemm_qkv_v_insert/int8,tag", qkv(), lambda o, i: o.gemm_qkv_v_insert(None, (i["wq"], i["sw"]), i["bias"], i["cache_v"], 4, 1, 3,
                                                                              xq=(i["xi"], i["sx"]), tag="t"))
    added("gemm_w8a8_qkv_v_insert", "gemm_qkv_v_insert/int8,tag", lambda o, i: o.gemm_w8a8_qkv_v_insert(
        (i["xi"], i["sx"]), (i["wq"], i["sw"]), i["bias"], i["cache_v"], 4, 1, 3, 1, 4, tag="t"))
    case("gemm_qkv_v_insert/cache shape", qkv(), lambda o, i: o.gemm_qkv_v_insert(i["x"], i["w"], i["bias"], i["cache_v"][:, :, :1], 8, 0, 4))
    case("gemm_qkv_v_insert/w shape", qkv(), lambda o, i: o.gemm_qkv_v_insert(i["x"], i["w"][:, :128], i["bias"], i["cache_v"], 8, 0, 4))
    case("gemm_qkv_v_insert/int8 sx size", qkv(), lambda o, i: o.gemm_qkv_v_insert(None, (i["wq"], i["sw"]), i["bias"], i["cache_v"], 4, 1, 3,
                                                                                  xq=(i["xi"], i["sx"][:3])))
    case("gemm_qkv_v_insert/int8 wq dtype", qkv(), lambda o, i: o.gemm_qkv_v_insert(None, (i["w"], i["sw"]), i["bias"], i["cache_v"], 4, 1, 3,
                                                                                   xq=(i["xi"], i["sx"])))
    case("gemm_qkv_v_insert/cpu bias", qkv(), lambda o, i: o.gemm_qkv_v_insert(i["x"], i["w"], cpu(i["bias"]), i["cache_v"], 8, 0, 4))

    def qops(g, M=4, N=256, K=256):
        a, w = GEMMS[g]

        def make():
            from longlive_amd import ops as o
            xq, sx = _pair(o, a, (M, K))
            wq, sw = _pair(o, w, (N, K))
            return dict(xq=xq.zero_(), sx=sx.zero_(), wq=wq.zero_(), sw=sw.zero_(), bias=Z(N), res=Z(M, N), e=Z(1, 2, 6, N), mod=Z(6, N), out=Z(M, N),
                        cache_v=Z(1, 12, N // 384 or 1, 128))
        return make
    for g in GEMMS:
        row = g in ("w8a8", "f8")
        fn = (lambda o, i, g=g: lambda *a, **k: getattr(o, "gemm_" + g)(i["xq"], i["sx"], i["wq"], i["sw"], *a, **k)) if row else \
             (lambda o, i, g=g: lambda *a, **k: getattr(o, "gemm_" + g)((i["xq"], i["sx"]), (i["wq"], i["sw"]), *a, **k))
        case(f"gemm_{g}", qops(g), lambda o, i, fn=fn: fn(o, i)(i["bias"]))
        case(f"gemm_{g}/gelu,out,tag", qops(g), lambda o, i, fn=fn: fn(o, i)(i["bias"], o.EPI_BIAS_GELU, out=i["out"], tag="t"))
        case(f"gemm_{g}/res", qops(g), lambda o, i, fn=fn: fn(o, i)(i["bias"], o.EPI_BIAS_RES, res=i["res"]))
        case(f"gemm_{g}/gate", qops(g), lambda o, i, fn=fn: fn(o, i)(i["bias"], o.EPI_BIAS_GATE_RES, out=i["res"], res=i["res"], e=i["e"], mod=i["mod"],
                                                                    gate_idx=2, rows_per_batch=4, frame_len=2))
        case(f"gemm_{g}/gate,premod", qops(g), lambda o, i, fn=fn: fn(o, i)(i["bias"], o.EPI_BIAS_GATE_RES, res=i["res"], e=i["e"], gate_idx=5,
                                                                           rows_per_batch=4, frame_len=2))
        case(f"gemm_{g}/res missing", qops(g), lambda o, i, fn=fn: fn(o, i)(i["bias"], o.EPI_BIAS_RES))
        case(f"gemm_{g}/e shape", qops(g), lambda o, i, fn=fn: fn(o, i)(i["bias"], o.EPI_BIAS_GATE_RES, res=i["res"], e=i["e"], frame_len=4))
        case(f"gemm_{g}/bias size", qops(g), lambda o, i, fn=fn: fn(o, i)(i["bias"][:8]))
        if not row:
            case(f"gemm_{g}/mx_out", qops(g), lambda o, i, fn=fn: fn(o, i)(i["bias"], o.EPI_BIAS_GELU, mx_out=True))
            case(f"gemm_{g}/mx_out without gelu", qops(g), lambda o, i, fn=fn: fn(o, i)(i["bias"], mx_out=True))
            case(f"gemm_plan_{g}", dict, lambda o, i, g=g: getattr(o, "gemm_plan_" + g)(4, 256, 256))
        if g == "f8":
            case("gemm_plan_f8", dict, lambda o, i: o.gemm_plan_f8(4, 256, 256))
        if g != "w8a8":
            case(f"gemm_{g}_qkv_v_insert", qops(g, N=768), lambda o, i, g=g: getattr(o, f"gemm_{g}_qkv_v_insert")(
                (i["xq"], i["sx"]), (i["wq"], i["sw"]), i["bias"], i["cache_v"], 8, 0, 4, 1, 4))
            case(f"gemm_{g}_qkv_v_insert/rows,tag", qops(g, N=768), lambda o, i, g=g: getattr(o, f"gemm_{g}_qkv_v_insert")(
                (i["xq"], i["sx"]), (i["wq"], i["sw"]), i["bias"], i["cache_v"], 8, 0, 4, 2, 4, tag="t"))
    case("gemm_mx/x codes dtype", qops("mx"), lambda o, i: o.gemm_mx((i["xq"].view(u8), i["sx"]), (i["wq"], i["sw"]), i["bias"]))
    case("gemm_mx/K differs", qops("mx"), lambda o, i: o.gemm_mx((i["xq"][:, :128].contiguous(), i["sx"][:, :4].contiguous()), (i["wq"], i["sw"]), i["bias"]))
    case("gemm_mx6/packed width", qops("mx6"), lambda o, i: o.gemm_mx6((i["xq"][:, :96].contiguous(), i["sx"]), (i["wq"], i["sw"]), i["bias"]))
    case("gemm_w8a8/scales size", qops("w8a8"), lambda o, i: o.gemm_w8a8(i["xq"], i["sx"][:3], i["wq"], i["sw"], i["bias"]))


def _attention():
    def qkv(H=2, Lq=4, Sk=40):
        return lambda: dict(q=Z(1, Lq, H, 128), k=Z(1, Sk, H, 128), v=Z(1, Sk, H, 128), out=Z(1, Lq, H, 128), ssq=Z(H, Lq, dtype=f32), norm_w=Z(H * 128))
    case("flash_attn/one range", qkv(), lambda o, i: o.flash_attn(i["q"], i["k"], i["v"], [(0, 40)]))
    case("flash_attn/two ranges,out,scale,tag", qkv(), lambda o, i: o.flash_attn(i["q"], i["k"], i["v"], [(0, 8), (16, 40)], out=i["out"], scale=0.25, tag="t"))
    case("flash_attn/an empty range dropped", qkv(), lambda o, i: o.flash_attn(i["q"], i["k"], i["v"], [(8, 8), (16, 40)]))
    case("flash_attn/three ranges", qkv(), lambda o, i: o.flash_attn(i["q"], i["k"], i["v"], [(0, 8), (16, 24), (32, 40)]))
    case("flash_attn/no range", qkv(), lambda o, i: o.flash_attn(i["q"], i["k"], i["v"], [(8, 8)]))
    case("flash_attn/range past the keys", qkv(), lambda o, i: o.flash_attn(i["q"], i["k"], i["v"], [(0, 41)]))
    case("flash_attn/head_dim", lambda: dict(q=Z(1, 4, 2, 64), k=Z(1, 8, 2, 64), v=Z(1, 8, 2, 64)), lambda o, i: o.flash_attn(i["q"], i["k"], i["v"], [(0, 8)]))
    case("flash_attn/v shape", qkv(), lambda o, i: o.flash_attn(i["q"], i["k"], i["v"][:, :39], [(0, 8)]))
    case("flash_attn/q strided", qkv(), lambda o, i: o.flash_attn(i["q"].transpose(1, 2), i["k"], i["v"], [(0, 8)]))
    case("flash_attn/k dtype", qkv(), lambda o, i: o.flash_attn(i["q"], i["k"].float(), i["v"], [(0, 8)]))
    case("flash_attn/cpu", qkv(), lambda o, i: o.flash_attn(i["q"], i["k"], cpu(i["v"]), [(0, 8)]))
    case("flash_attn/out shape", qkv(), lambda o, i: o.flash_attn(i["q"], i["k"], i["v"], [(0, 8)], out=i["out"][:, :3]))
    for f in ("MX", "MX6", "MX4"):
        case(f"flash_attn/out_fmt {f}, kernel", qkv(), lambda o, i, f=f: o.flash_attn(i["q"], i["k"], i["v"], [(0, 8), (16, 40)], out_fmt=getattr(o, f), tag="t"),
             ll_flash_attn_q_ok=1)
        case(f"flash_attn/out_fmt {f}, two launches", qkv(), lambda o, i, f=f: o.flash_attn(i["q"], i["k"], i["v"], [(0, 40)], out_fmt=getattr(o, f)))
        case(f"flash_attn_q_ok/{f}", dict, lambda o, i, f=f: o.flash_attn_q_ok(getattr(o, f), 12, [(0, 8), (8, 8), (16, 40)]), ll_flash_attn_q_ok=1)
        case(f"flash_attn_q_plan/{f}", dict, lambda o, i, f=f: o.flash_attn_q_plan(getattr(o, f), 4680, 12, 1, [(0, 18720)]))
        for H in (1, 2):
            case(f"flash_attn_mx/out_fmt {f}, H={H}", lambda H=H: _shadow(H), lambda o, i, f=f: o.flash_attn_mx(i["q"], _sh(i), [(0, 8), (16, 40)], out_fmt=getattr(o, f)))
    case("flash_attn/out_fmt Q8", qkv(), lambda o, i: o.flash_attn(i["q"], i["k"], i["v"], [(0, 40)], out_fmt=o.Q8))
    case("flash_attn/out_fmt MX, kernel, k shape", qkv(), lambda o, i: o.flash_attn(i["q"], i["k"][:, :39], i["v"], [(0, 8)], out_fmt=o.MX), ll_flash_attn_q_ok=1)
    case("flash_attn/out_fmt MX, kernel, range past the keys", qkv(), lambda o, i: o.flash_attn(i["q"], i["k"], i["v"], [(0, 41)], out_fmt=o.MX), ll_flash_attn_q_ok=1)
    case("flash_attn_qnorm_ok", dict, lambda o, i: o.flash_attn_qnorm_ok(12, 512), ll_flash_attn_qnorm_ok=1)
    case("flash_attn_qnorm", qkv(), lambda o, i: o.flash_attn_qnorm(i["q"], i["ssq"], i["norm_w"], 1e-6, i["k"], i["v"], 16))
    case("flash_attn_qnorm/out,scale,tag", qkv(), lambda o, i: o.flash_attn_qnorm(i["q"], i["ssq"], i["norm_w"], 1e-6, i["k"], i["v"], 40, out=i["out"], scale=0.5, tag="t"))
    case("flash_attn_qnorm/keys past", qkv(), lambda o, i: o.flash_attn_qnorm(i["q"], i["ssq"], i["norm_w"], 1e-6, i["k"], i["v"], 41))
    case("flash_attn_qnorm/ssq shape", qkv(), lambda o, i: o.flash_attn_qnorm(i["q"], i["ssq"][:1], i["norm_w"], 1e-6, i["k"], i["v"], 16))
    case("flash_attn_qnorm/ssq dtype", qkv(), lambda o, i: o.flash_attn_qnorm(i["q"], i["ssq"].to(bf16), i["norm_w"], 1e-6, i["k"], i["v"], 16))
    case("flash_attn_qnorm/head_dim", lambda: dict(q=Z(1, 4, 2, 64), k=Z(1, 8, 2, 64), v=Z(1, 8, 2, 64), ssq=Z(2, 4, dtype=f32), norm_w=Z(128)),
         lambda o, i: o.flash_attn_qnorm(i["q"], i["ssq"], i["norm_w"], 1e-6, i["k"], i["v"], 8))
    case("flash_attn_qnorm/v shape", qkv(), lambda o, i: o.flash_attn_qnorm(i["q"], i["ssq"], i["norm_w"], 1e-6, i["k"], i["v"][:, :8], 4))

    def _shadow(H=2, S=40):
        return dict(q=Z(1, 4, H, 128), out=Z(1, 4, H, 128), cache_k=Z(1, S, H, 128), cache_v=Z(1, S, H, 128), kq=Z(1, 64, H, 128, dtype=u8), ks=Z(1, 64, H, 4, dtype=u8),
                    vq=Z(1, H, 2, 128, 32, dtype=u8), vs=Z(1, H, 2, 128, dtype=u8))

    def _sh(i, S=40):
        return dict(kq=i["kq"].view(torch.float8_e4m3fn), ks=i["ks"], vq=i["vq"].view(torch.float8_e4m3fn), vs=i["vs"], S=S)
    case("kv_shadow_mx_alloc", _shadow, lambda o, i: o.kv_shadow_mx_alloc(i["cache_k"]))
    case("kv_shadow_mx_alloc/head_dim", lambda: dict(cache_k=Z(1, 40, 2, 64)), lambda o, i: o.kv_shadow_mx_alloc(i["cache_k"]))
    case("kv_shadow_mx", _shadow, lambda o, i: o.kv_shadow_mx(i["cache_k"], i["cache_v"], _sh(i), 5, 37))
    case("kv_shadow_mx/tag", _shadow, lambda o, i: o.kv_shadow_mx(i["cache_k"], i["cache_v"], _sh(i), 32, 40, tag="t"))
    case("kv_shadow_mx/other cache", _shadow, lambda o, i: o.kv_shadow_mx(i["cache_k"], i["cache_v"], _sh(i, S=48), 0, 8))
    case("flash_attn_mx", _shadow, lambda o, i: o.flash_attn_mx(i["q"], _sh(i), [(0, 8), (16, 40)]))
    case("flash_attn_mx/one range,out,scale,tag", _shadow, lambda o, i: o.flash_attn_mx(i["q"], _sh(i), [(3, 3), (0, 40)], out=i["out"], scale=0.125, tag="t"))
    case("flash_attn_mx/range past the cache", _shadow, lambda o, i: o.flash_attn_mx(i["q"], _sh(i), [(0, 41)]))
    case("flash_attn_mx/shadow shape", _shadow, lambda o, i: o.flash_attn_mx(i["q"][:, :, :1].contiguous(), _sh(i), [(0, 40)]))
    case("flash_attn_mx/q dtype", _shadow, lambda o, i: o.flash_attn_mx(i["q"].float(), _sh(i), [(0, 40)]))
    case("flash_attn_mx/out_fmt F8", _shadow, lambda o, i: o.flash_attn_mx(i["q"], _sh(i), [(0, 40)], out_fmt=o.F8))
    case("flash_attn_mx_plan", dict, lambda o, i: o.flash_attn_mx_plan(4680, 12, 1, [(0, 4680), (9360, 18720)]))
    rope = lambda: dict(qkv=Z(1, 4, 768), wq=Z(256), wk=Z(256), rope_f=Z(1024, 22, 2, dtype=f32), rope_hw=Z(2, 42, 2, dtype=f32), q_out=Z(1, 4, 256),  # noqa: E731
                        cache_k=Z(1, 12, 2, 128), cache_v=Z(1, 12, 2, 128))
    args = lambda i, v: (i["qkv"], i["wq"], i["wk"], i["rope_f"], i["rope_hw"], i["q_out"], i["cache_k"], v, 128, 2, 3, 8, 0, 4, 1e-6)  # noqa: E731
    case("qk_norm_rope_kv_store", rope, lambda o, i: o.qk_norm_rope_kv_store(*args(i, i["cache_v"])))
    case("qk_norm_rope_kv_store/v inserted", rope, lambda o, i: o.qk_norm_rope_kv_store(*args(i, None)))
    case("qk_norm_rope_kv_store/rope_f dtype", rope, lambda o, i: o.qk_norm_rope_kv_store(*args(dict(i, rope_f=i["rope_f"].to(bf16)), None)))
    case("qk_norm_rope_kv_store/rope_hw shape", rope, lambda o, i: o.qk_norm_rope_kv_store(*args(dict(i, rope_hw=i["rope_hw"][:1]), None)))
    case("kv_roll", rope, lambda o, i: o.kv_roll(i["cache_k"], i["cache_v"], 2, 4, 6))
    case("kv_roll/v shape", rope, lambda o, i: o.kv_roll(i["cache_k"], i["cache_v"][:, :8], 2, 4, 6))


def _vae():
    geo3, geo2, geo1 = (8, 16, 256, 3, 3), (8, 16, 128, 1, 3), (8, 16, 64, 1, 1)

    def conv(geo, T=2, **more):
        return lambda: dict(x=Z(T + (2 if geo[3] > 1 else 0), 4, 6, geo[0]), w=Z(geo[1], geo[2]), bias=Z(geo[1]), gamma=Z(geo[1]), res=Z(T, 4, 6, geo[1]),
                            out=Z(T, 4, 6, geo[1]), res_up=Z(T, 8, 12, geo[1]), out_up=Z(T, 8, 12, geo[1]), **{k: v() for k, v in more.items()})
    for nm, geo in (("temporal", geo3), ("spatial", geo2), ("1x1", geo1)):
        case(f"conv_cl/{nm}", conv(geo), lambda o, i, geo=geo: o.conv_cl(i["x"], i["w"], i["bias"], geo))
        case(f"conv_cl/{nm},upsample,res,out", conv(geo), lambda o, i, geo=geo: o.conv_cl(i["x"], i["w"], i["bias"], geo, upsample=True, res=i["res_up"], out=i["out_up"]))
        case(f"conv_cl_rms/{nm}", conv(geo), lambda o, i, geo=geo: o.conv_cl_rms(i["x"], i["w"], i["bias"], geo, i["gamma"], i["out"]))
        case(f"conv_cl_rms/{nm},no silu,upsample,res,want_raw", conv(geo), lambda o, i, geo=geo: o.conv_cl_rms(
            i["x"], i["w"], i["bias"], geo, i["gamma"], i["out_up"], silu=False, upsample=True, res=i["res_up"], want_raw=True))
    case("conv_cl/res", conv(geo3), lambda o, i: o.conv_cl(i["x"], i["w"], i["bias"], geo3, res=i["res"]))
    case("conv_cl/too few frames", conv(geo3, T=0), lambda o, i: o.conv_cl(i["x"], i["w"], i["bias"], geo3))
    case("conv_cl/channels", conv(geo3), lambda o, i: o.conv_cl(i["x"], i["w"], i["bias"], (16,) + geo3[1:]))
    case("conv_cl/w shape", conv(geo3), lambda o, i: o.conv_cl(i["x"], i["w"][:, :64], i["bias"], geo3))
    case("conv_cl/out shape", conv(geo3), lambda o, i: o.conv_cl(i["x"], i["w"], i["bias"], geo3, out=i["out_up"]))
    case("conv_cl/res shape", conv(geo3), lambda o, i: o.conv_cl(i["x"], i["w"], i["bias"], geo3, res=i["res_up"]))
    case("conv_cl/x dtype", conv(geo3), lambda o, i: o.conv_cl(i["x"].float(), i["w"], i["bias"], geo3))
    case("conv_cl/cpu", conv(geo3), lambda o, i: o.conv_cl(i["x"], cpu(i["w"]), i["bias"], geo3))
    case("conv_cl_rms/too few frames", conv(geo3, T=0), lambda o, i: o.conv_cl_rms(i["x"], i["w"], i["bias"], geo3, i["gamma"], i["out"]))
    case("conv_cl_rms/channels", conv(geo3), lambda o, i: o.conv_cl_rms(i["x"], i["w"], i["bias"], (16,) + geo3[1:], i["gamma"], i["out"]))
    case("conv_cl_rms/w shape", conv(geo3), lambda o, i: o.conv_cl_rms(i["x"], i["w"][:8], i["bias"], geo3, i["gamma"], i["out"]))
    case("conv_cl_rms/gamma size", conv(geo3), lambda o, i: o.conv_cl_rms(i["x"], i["w"], i["bias"], geo3, i["gamma"][:8], i["out"]))
    case("conv_cl_rms/out_rms shape", conv(geo3), lambda o, i: o.conv_cl_rms(i["x"], i["w"], i["bias"], geo3, i["gamma"], i["out_up"]))
    case("conv_cl_rms/res shape", conv(geo3), lambda o, i: o.conv_cl_rms(i["x"], i["w"], i["bias"], geo3, i["gamma"], i["out"], res=i["res_up"]))
    case("conv_cl_rms/out_rms strided", conv(geo3), lambda o, i: o.conv_cl_rms(i["x"], i["w"], i["bias"], geo3, i["gamma"], i["out_up"][:, ::2, ::2]))
    case("conv_cl_rms_ok", dict, lambda o, i: [o.conv_cl_rms_ok(geo3, 60, 104), o.conv_cl_rms_ok(geo2, 30, 52, upsample=True)], ll_conv_cl_rms_ok=1)
    case("conv_plan", dict, lambda o, i: [o.conv_plan(2, 60, 104, geo3), o.conv_plan(2, 60, 104, geo2, upsample=True, res=True, rms=True)])
    case("conv_down_plan", dict, lambda o, i: [o.conv_down_plan(0, 4, 60, 104, 96, 96), o.conv_down_plan(1, 4, 60, 104, 96, 96)])
    gd, gt = (8, 16, 128, 1, 3), (8, 16, 64, 3, 1)
    down = lambda: dict(x=Z(4, 4, 6, 8), xt=Z(5, 4, 6, 8), w=Z(16, 128), wt=Z(16, 64), bias=Z(16), out=Z(4, 2, 3, 24), outt=Z(2, 4, 6, 16))  # noqa: E731
    case("conv_cl_down", down, lambda o, i: o.conv_cl_down(i["x"], i["w"], i["bias"], gd))
    case("conv_cl_down/wider out", down, lambda o, i: o.conv_cl_down(i["x"], i["w"], i["bias"], gd, out=i["out"]))
    case("conv_cl_down/temporal weights", down, lambda o, i: o.conv_cl_down(i["x"], i["wt"], i["bias"], gt))
    case("conv_cl_down/channels", down, lambda o, i: o.conv_cl_down(i["x"], i["w"], i["bias"], (4,) + gd[1:]))
    case("conv_cl_down/out shape", down, lambda o, i: o.conv_cl_down(i["x"], i["w"], i["bias"], gd, out=i["outt"]))
    case("conv_cl_tdown", down, lambda o, i: o.conv_cl_tdown(i["xt"], i["wt"], i["bias"], gt))
    case("conv_cl_tdown/out", down, lambda o, i: o.conv_cl_tdown(i["xt"], i["wt"], i["bias"], gt, out=i["outt"]))
    case("conv_cl_tdown/one frame", down, lambda o, i: o.conv_cl_tdown(i["xt"][:1], i["wt"], i["bias"], gt))
    case("conv_cl_tdown/x dtype", down, lambda o, i: o.conv_cl_tdown(i["xt"].float(), i["wt"], i["bias"], gt))
    case("zero_row", dict, lambda o, i: [o.zero_row(torch.device("cpu")), o.zero_row(torch.device("cpu"))])
    row = lambda: dict(x=Z(2, 4, 6, 16), gamma=Z(16), out=Z(2, 4, 6, 16), s=Z(6, 32), z=Z(2, 16, 4, 6), mean=Z(16), inv_std=Z(16))  # noqa: E731
    case("rms_silu_cl", row, lambda o, i: o.rms_silu_cl(i["x"], i["gamma"]))
    case("rms_silu_cl/no silu,out", row, lambda o, i: o.rms_silu_cl(i["x"], i["gamma"], silu=False, out=i["out"]))
    case("rms_silu_cl/gamma size", row, lambda o, i: o.rms_silu_cl(i["x"], i["gamma"][:8]))
    case("softmax_rows", row, lambda o, i: o.softmax_rows(i["s"], 0.5))
    case("softmax_rows/n_valid,out", row, lambda o, i: o.softmax_rows(i["s"], 2, n_valid=20, out=i["s"]))
    case("vae_unscale_cl", row, lambda o, i: o.vae_unscale_cl(i["z"], i["mean"], i["inv_std"]))
    case("vae_unscale_cl/mean size", row, lambda o, i: o.vae_unscale_cl(i["z"], i["mean"][:8], i["inv_std"]))
    case("vae_scale_tchw", row, lambda o, i: o.vae_scale_tchw(i["x"], i["mean"][:12].contiguous(), i["inv_std"][:12].contiguous()))
    case("vae_scale_tchw/too narrow", row, lambda o, i: o.vae_scale_tchw(i["x"][..., :8].contiguous(), i["mean"], i["inv_std"]))
    case("cl_to_tchw_clamp", row, lambda o, i: o.cl_to_tchw_clamp(i["x"]))
    case("cl_to_tchw_clamp/x strided", row, lambda o, i: o.cl_to_tchw_clamp(i["x"][..., :8]))
    px = lambda: dict(p0=Z(3, 2, 4, 6, dtype=f32), p1=Z(2, 3, 4, 6), out=Z(2, 4, 6, 8), u=Z(3, 4, 6, 3, dtype=u8), wide=Z(2, 4, 6, 6, dtype=u8))  # noqa: E731
    case("pixels_to_cl/channels first, fp32", px, lambda o, i: o.pixels_to_cl(i["p0"], 0))
    case("pixels_to_cl/frames first, bf16, out", px, lambda o, i: o.pixels_to_cl(i["p1"], 1, out=i["out"]))
    case("pixels_to_cl/frame view", px, lambda o, i: o.pixels_to_cl(i["p0"][:, 1:], 0, cpad=16))
    case("pixels_to_cl/copied", px, lambda o, i: o.pixels_to_cl(i["p0"][..., ::2], 0))
    case("pixels_to_cl/dtype", px, lambda o, i: o.pixels_to_cl(i["p0"].half(), 0))
    case("pixels_to_cl/shape", px, lambda o, i: o.pixels_to_cl(i["p0"], 1))
    case("pixels_to_cl/cpu", px, lambda o, i: o.pixels_to_cl(cpu(i["p0"]), 0))
    case("pixels_u8_to_cl", px, lambda o, i: o.pixels_u8_to_cl(i["u"]))
    case("pixels_u8_to_cl/frame view, out", px, lambda o, i: o.pixels_u8_to_cl(i["u"][::2], cpad=8, out=i["out"]))
    case("pixels_u8_to_cl/one frame of a view", px, lambda o, i: o.pixels_u8_to_cl(i["u"][1:2]))
    case("pixels_u8_to_cl/copied", px, lambda o, i: o.pixels_u8_to_cl(i["wide"][..., :3]))
    case("pixels_u8_to_cl/dtype", px, lambda o, i: o.pixels_u8_to_cl(i["u"].float()))
    case("pixels_u8_to_cl/shape", px, lambda o, i: o.pixels_u8_to_cl(i["wide"]))
    case("pixels_u8_to_cl/cpu", px, lambda o, i: o.pixels_u8_to_cl(cpu(i["u"])))
    case("pixels_u8_to_cl/out shape", px, lambda o, i: o.pixels_u8_to_cl(i["u"], out=i["out"]))


def _frames():
    fr = lambda: dict(x=Z(3, 4, 6, 8), u=Z(3, 4, 6, 3, dtype=u8), wide=Z(3, 4, 6, 6, dtype=u8), big=Z(6, 4, 6, 3, dtype=u8), out=Z(3, 4, 6, 3, dtype=u8),  # noqa: E731
                      yuv=Z(3, 36, dtype=u8), yuv2=Z(6, 36, dtype=u8), rows=Z(3, 40, dtype=u8), rows2=Z(3, 80, dtype=u8))
    case("cl_to_frames_u8", fr, lambda o, i: o.cl_to_frames_u8(i["x"]))
    case("cl_to_frames_u8/out view", fr, lambda o, i: o.cl_to_frames_u8(i["x"], out=i["big"][::2]))
    case("cl_to_frames_u8/one frame into a view", fr, lambda o, i: o.cl_to_frames_u8(i["x"][:1], out=i["big"][4:5]))
    case("cl_to_frames_u8/out dtype", fr, lambda o, i: o.cl_to_frames_u8(i["x"], out=i["out"].float()))
    case("cl_to_frames_u8/out cpu", fr, lambda o, i: o.cl_to_frames_u8(i["x"], out=cpu(i["out"])))
    case("cl_to_frames_u8/out pixels strided", fr, lambda o, i: o.cl_to_frames_u8(i["x"], out=i["wide"][..., :3]))
    case("cl_to_frames_u8/out shape", fr, lambda o, i: o.cl_to_frames_u8(i["x"], out=i["big"]))
    case("cl_to_frames_u8/out frames overlap", fr, lambda o, i: o.cl_to_frames_u8(i["x"], out=i["out"][:1].expand(3, 4, 6, 3)))
    for nm, fn in (("jpeg_encode", lambda o, f: o.jpeg_encode(f, 75)), ("jpeg_coefficients", lambda o, f: o.jpeg_coefficients(f)),
                   ("png_encode", lambda o, f: o.png_encode(f)), ("png_filter", lambda o, f: o.png_filter(f)),
                   ("frames_u8_to_yuv420", lambda o, f: o.frames_u8_to_yuv420(f)), ("resize_u8", lambda o, f: o.resize_u8(f, (2, 3)))):
        case(nm, fr, lambda o, i, fn=fn: fn(o, i["u"]))
        case(nm + "/frame view", fr, lambda o, i, fn=fn: fn(o, i["big"][1::2]))
        case(nm + "/one frame of a view", fr, lambda o, i, fn=fn: fn(o, i["big"][3:4]))
        case(nm + "/copied", fr, lambda o, i, fn=fn: fn(o, i["wide"][..., :3]))
        case(nm + "/dtype", fr, lambda o, i, fn=fn: fn(o, i["u"].to(torch.int16)))
        case(nm + "/shape", fr, lambda o, i, fn=fn: fn(o, i["wide"]))
        case(nm + "/cpu", fr, lambda o, i, fn=fn: fn(o, cpu(i["u"])))
    case("jpeg_sizes", dict, lambda o, i: o.jpeg_sizes(3, 480, 832))
    case("png_sizes", dict, lambda o, i: o.png_sizes(3, 480, 832))
    case("zlib_sizes", dict, lambda o, i: o.zlib_sizes(3, 1 << 33))
    case("zlib_compress", fr, lambda o, i: o.zlib_compress(i["rows"]))
    case("zlib_compress/row view", fr, lambda o, i: o.zlib_compress(i["rows2"][:, 8:48]))
    case("zlib_compress/one row of a view", fr, lambda o, i: o.zlib_compress(i["rows2"][1:2, 8:48]))
    case("zlib_compress/copied", fr, lambda o, i: o.zlib_compress(i["rows2"][:, ::2]))
    case("zlib_compress/dtype", fr, lambda o, i: o.zlib_compress(i["rows"].to(i8)))
    case("zlib_compress/shape", fr, lambda o, i: o.zlib_compress(i["u"]))
    case("zlib_compress/cpu", fr, lambda o, i: o.zlib_compress(cpu(i["rows"])))
    case("frames_u8_to_yuv420/full,out view", fr, lambda o, i: o.frames_u8_to_yuv420(i["u"], range="full", out=i["yuv2"][::2]))
    case("frames_u8_to_yuv420/range", fr, lambda o, i: o.frames_u8_to_yuv420(i["u"], range="tv"))
    case("frames_u8_to_yuv420/out shape", fr, lambda o, i: o.frames_u8_to_yuv420(i["u"], out=i["rows"]))
    case("frames_u8_to_yuv420/out dtype", fr, lambda o, i: o.frames_u8_to_yuv420(i["u"], out=i["yuv"].to(i8)))
    case("cl_to_yuv420", fr, lambda o, i: o.cl_to_yuv420(i["x"]))
    case("cl_to_yuv420/full,out", fr, lambda o, i: o.cl_to_yuv420(i["x"], range="full", out=i["yuv"]))
    case("cl_to_yuv420/one frame into a view", fr, lambda o, i: o.cl_to_yuv420(i["x"][:1], out=i["yuv2"][2:3]))
    case("cl_to_yuv420/range", fr, lambda o, i: o.cl_to_yuv420(i["x"], range=None))
    case("cl_to_yuv420/x dtype", fr, lambda o, i: o.cl_to_yuv420(i["x"].float()))
    case("resize_u8/stretch,out view", fr, lambda o, i: o.resize_u8(i["u"], (4, 6), fit="stretch", out=i["big"][::2]))
    case("resize_u8/cover, tall target", fr, lambda o, i: o.resize_u8(i["u"], (6, 2)))
    case("resize_u8/fit", fr, lambda o, i: o.resize_u8(i["u"], (2, 3), fit="pad"))
    case("resize_u8/out shape", fr, lambda o, i: o.resize_u8(i["u"], (2, 3), out=i["out"]))
    case("resize_u8/out dtype", fr, lambda o, i: o.resize_u8(i["u"], (4, 6), out=i["out"].to(i8)))

    def planes(layout, H=4, W=6, T=2):
        def make():
            from longlive_amd import ops as o
            hc, wc = o.yuv_chroma_shape(layout, H, W)
            return dict(buf=Z(T, H * W + 2 * hc * wc + 5, dtype=u8), y=Z(T, H, W, dtype=u8), cb=Z(T, max(hc, 1), max(wc, 1), dtype=u8),
                        cr=Z(T, max(hc, 1), max(wc, 1), dtype=u8), cr2=Z(2 * T, max(hc, 1), max(wc, 1), dtype=u8), out=Z(2 * T, H, W, 3, dtype=u8), hw=(hc, wc))
        return make

    def packed(i, H=4, W=6):
        hc, wc = i["hw"]
        b = i["buf"]
        return (b[:, :H * W].unflatten(-1, (H, W)), b[:, H * W:H * W + hc * wc].unflatten(-1, (hc, wc)), b[:, H * W + hc * wc:H * W + 2 * hc * wc].unflatten(-1, (hc, wc)))
    for lay in ("420jpeg", "420mpeg2", "420paldv", "422", "444"):
        case(f"yuv_to_frames_u8/{lay}", planes(lay), lambda o, i, lay=lay: o.yuv_to_frames_u8(i["y"], i["cb"], i["cr"], layout=lay))
        case(f"yuv_to_frames_u8/{lay},packed payload,full,out view", planes(lay), lambda o, i, lay=lay: o.yuv_to_frames_u8(*packed(i), layout=lay, range="full", out=i["out"][::2]))
    case("yuv_to_frames_u8/mono", planes("mono"), lambda o, i: o.yuv_to_frames_u8(i["y"], layout="mono"))
    case("yuv_to_frames_u8/mono ignores chroma", planes("mono"), lambda o, i: o.yuv_to_frames_u8(i["y"], i["cb"], i["cr"], layout="mono"))
    case("yuv_to_frames_u8/cb and cr strides differ", planes("420jpeg"), lambda o, i: o.yuv_to_frames_u8(i["y"], i["cb"], i["cr2"][::2]))
    case("yuv_to_frames_u8/one frame", planes("420jpeg", T=1), lambda o, i: o.yuv_to_frames_u8(*packed(i)))
    case("yuv_to_frames_u8/y copied", planes("420jpeg"), lambda o, i: o.yuv_to_frames_u8(i["out"][:2, :, :, 0], i["cb"], i["cr"]))
    case("yuv_to_frames_u8/cr missing", planes("420jpeg"), lambda o, i: o.yuv_to_frames_u8(i["y"], i["cb"]))
    case("yuv_to_frames_u8/cb shape", planes("422"), lambda o, i: o.yuv_to_frames_u8(i["y"], i["cb"][:, :2], i["cr"], layout="422"))
    case("yuv_to_frames_u8/y dims", planes("444"), lambda o, i: o.yuv_to_frames_u8(i["y"][0], i["cb"], i["cr"], layout="444"))
    case("yuv_to_frames_u8/layout", planes("444"), lambda o, i: o.yuv_to_frames_u8(i["y"], i["cb"], i["cr"], layout="411"))
    case("yuv_to_frames_u8/range", planes("444"), lambda o, i: o.yuv_to_frames_u8(i["y"], i["cb"], i["cr"], layout="444", range="pc"))
    case("yuv_to_frames_u8/cr dtype", planes("444"), lambda o, i: o.yuv_to_frames_u8(i["y"], i["cb"], i["cr"].to(i8), layout="444"))
    case("yuv_to_frames_u8/y cpu", planes("444"), lambda o, i: o.yuv_to_frames_u8(cpu(i["y"]), i["cb"], i["cr"], layout="444"))
    case("yuv_to_frames_u8/out shape", planes("444"), lambda o, i: o.yuv_to_frames_u8(i["y"], i["cb"], i["cr"], layout="444", out=i["out"]))


@functools.lru_cache(maxsize=None)
def jpeg_files(n, H=16, W=32, noisy=False):
    """n baseline 4:2:0 files from the host encoder; `noisy`: frames whose one restart segment per MCU row is long enough to be cut."""
    import jpeg_ref
    return [jpeg_ref.encode((jpeg_ref.noise if noisy else jpeg_ref.smooth_noise)(H, W, t), 90) for t in range(n)]


def _jpeg():
    dec = lambda: dict(out=Z(4, 16, 32, 3, dtype=u8), info=Z(2, dtype=i32), coef=Z(2, 1, 2, 6, 64, dtype=torch.int16), planes=Z(4096, dtype=u8), work=Z(8192, dtype=u8))  # noqa: E731
    dev = torch.device("cuda", 0)
    for nm in ("jpeg_decode", "jpeg_decode_coefficients"):
        fn = lambda o, nm=nm: getattr(o, nm)  # noqa: E731
        case(nm, dec, lambda o, i, fn=fn: fn(o)(jpeg_files(2), dev))
        case(nm + "/no device named, unchecked", dec, lambda o, i, fn=fn: fn(o)(jpeg_files(2), check=False))
        case(nm + "/bad status", dec, lambda o, i, fn=fn: fn(o)(jpeg_files(2), dev), jpeg_status=[0, 7])
        case(nm + "/bad status, unchecked", dec, lambda o, i, fn=fn: fn(o)(jpeg_files(2), dev, check=False), jpeg_status=[3, 7])
        case(nm + "/split=8", dec, lambda o, i, fn=fn: fn(o)(jpeg_files(2), dev, split=8, return_info=True))
        case(nm + "/split=8, bad status", dec, lambda o, i, fn=fn: fn(o)(jpeg_files(2), dev, split=8), jpeg_status=[1, 0])
        case(nm + "/split=8,rounds,info", dec, lambda o, i, fn=fn: fn(o)(jpeg_files(2), dev, split=8, rounds=3, info=i["info"], return_info=True))
        case(nm + "/split too long to cut anything", dec, lambda o, i, fn=fn: fn(o)(jpeg_files(2), dev, split=1 << 20, return_info=True))
        case(nm + "/auto", dec, lambda o, i, fn=fn: fn(o)(jpeg_files(2, 16, 1024, True), dev, split="auto"))
        case(nm + "/auto, many segments", dec, lambda o, i, fn=fn: (setattr(o, "JPEG_SPLIT_AUTO_SEGMENTS", 2), fn(o)(jpeg_files(2, 16, 1024, True), dev, split="auto"))[1])
        case(nm + "/info without split", dec, lambda o, i, fn=fn: fn(o)(jpeg_files(2), dev, return_info=True))
        case(nm + "/split value", dec, lambda o, i, fn=fn: fn(o)(jpeg_files(2), dev, split=10))
        case(nm + "/rounds value", dec, lambda o, i, fn=fn: fn(o)(jpeg_files(2), dev, split=8, rounds=0))
        case(nm + "/cpu device", dec, lambda o, i, fn=fn: fn(o)(jpeg_files(2), "cpu"))
        case(nm + "/info shape", dec, lambda o, i, fn=fn: fn(o)(jpeg_files(2), dev, split=8, info=i["info"][:1]))
    case("jpeg_decode/out view,scratch", dec, lambda o, i: o.jpeg_decode(jpeg_files(2), dev, out=i["out"][::2], scratch=(i["coef"], i["planes"])))
    case("jpeg_decode/split,scratch with work", dec, lambda o, i: o.jpeg_decode(jpeg_files(2), dev, split=8, scratch=(i["coef"], i["planes"], i["work"])))
    case("jpeg_decode/one frame into a view", dec, lambda o, i: o.jpeg_decode(jpeg_files(1), dev, out=i["out"][2:3]))
    case("jpeg_decode/work without split", dec, lambda o, i: o.jpeg_decode(jpeg_files(2), dev, scratch=(None, None, i["work"])))
    case("jpeg_decode/out shape", dec, lambda o, i: o.jpeg_decode(jpeg_files(2), dev, out=i["out"]))
    case("jpeg_decode/out dtype", dec, lambda o, i: o.jpeg_decode(jpeg_files(2), dev, out=i["out"][:2].to(i8)))
    case("jpeg_decode/planes too small", dec, lambda o, i: o.jpeg_decode(jpeg_files(2), dev, scratch=(None, i["planes"][:100])))
    case("jpeg_decode/coef shape", dec, lambda o, i: o.jpeg_decode(jpeg_files(2), dev, scratch=(i["coef"][:1], None)))
    case("jpeg_decode_coefficients/out,work", dec, lambda o, i: o.jpeg_decode_coefficients(jpeg_files(2), dev, out=i["coef"], split=8, work=i["work"]))
    case("jpeg_decode_coefficients/work too small", dec, lambda o, i: o.jpeg_decode_coefficients(jpeg_files(2), dev, split=8, work=i["work"][:64]))
    case("jpeg_decode_sizes", dict, lambda o, i: [o.jpeg_decode_sizes(2, 16, 32, 3, 2, 2), o.jpeg_decode_sizes(2, 16, 32, 3, 2, 2, split=(2, 9), rounds=5)])
    case("jpeg_decode_sizes/rounds", dict, lambda o, i: o.jpeg_decode_sizes(2, 16, 32, 3, 2, 2, split=(2, 9), rounds=65))


def _t5():
    t = lambda: dict(x=Z(4, 256), w=Z(256), h=Z(4, 64), table=Z(100, 256), ids=Z(5, dtype=torch.int64), qk=Z(8, 256), vt=Z(128, 8), tab=Z(2, 15),  # noqa: E731
                     t=Z(3, dtype=f32), steps=Z(4, dtype=f32), sig=Z(4, dtype=f32), px=Z(1, 2, 16, 4, 6), head=Z(1, 12, 64), sigma=Z(2, dtype=f32))
    case("t5_rmsnorm", t, lambda o, i: o.t5_rmsnorm(i["x"], i["w"]))
    case("t5_rmsnorm/eps", t, lambda o, i: o.t5_rmsnorm(i["x"], i["w"], eps=1e-5))
    case("t5_rmsnorm/w size", t, lambda o, i: o.t5_rmsnorm(i["x"], i["w"][:8]))
    case("t5_gated_gelu", t, lambda o, i: o.t5_gated_gelu(i["h"]))
    case("t5_gated_gelu/width", t, lambda o, i: o.t5_gated_gelu(i["h"][:, :40].contiguous()))
    case("gather_rows", t, lambda o, i: o.gather_rows(i["table"], i["ids"]))
    case("gather_rows/ids dtype", t, lambda o, i: o.gather_rows(i["table"], i["ids"].int()))
    case("t5_attention", t, lambda o, i: o.t5_attention(i["qk"], i["vt"], i["tab"], 2, 5))
    case("t5_attention/seq_len", t, lambda o, i: o.t5_attention(i["qk"], i["vt"], i["tab"], 2, 9))
    case("t5_attention/bias_tab shape", t, lambda o, i: o.t5_attention(i["qk"], i["vt"], i["tab"][:, :14].contiguous(), 2, 5))
    case("patchify", t, lambda o, i: o.patchify(i["px"]))
    case("patchify/x dtype", t, lambda o, i: o.patchify(i["px"].float()))
    case("sinusoid", t, lambda o, i: o.sinusoid(i["t"], 256))
    case("sinusoid/t dtype", t, lambda o, i: o.sinusoid(i["t"].to(bf16), 256))
    case("unpatchify_x0", t, lambda o, i: o.unpatchify_x0(i["head"], i["px"], i["sigma"]))
    case("unpatchify_x0/head shape", t, lambda o, i: o.unpatchify_x0(i["head"][:, :6].contiguous(), i["px"], i["sigma"]))
    case("unpatchify_x0/sigma size", t, lambda o, i: o.unpatchify_x0(i["head"], i["px"], i["sigma"][:1]))
    case("add_noise", t, lambda o, i: o.add_noise(i["px"][0], i["px"][0], i["sigma"]))
    case("add_noise/noise shape", t, lambda o, i: o.add_noise(i["px"][0], i["px"][0, :1], i["sigma"]))
    case("sigma_lookup", t, lambda o, i: o.sigma_lookup(i["t"], i["steps"], i["sig"]))
    case("sigma_lookup/table sizes", t, lambda o, i: o.sigma_lookup(i["t"], i["steps"], i["sig"][:3]))


for _group in (_producers, _gemms, _attention, _vae, _frames, _jpeg, _t5):
    _group()


def run_case(name, timed=True, used=None):
    """{"rows": [...], "events": torch.cuda.Event objects made} of one wrapper case."""
    from longlive_amd import ops
    make, call, answers = (CASES.get(name) or ADDED[name])[:3]
    inputs = make()
    tr = Trace(inputs, answers)
    saved_auto = ops.JPEG_SPLIT_AUTO_SEGMENTS
    with host_only(tr, timed, used), tr:
        try:
            tr.rows.append(["returned", tr.describe(call(ops, inputs))])
        except (RuntimeError, ValueError, AssertionError, TypeError, AttributeError) as exc:
            tr.rows.append(["raises", type(exc).__name__, str(exc)])
        finally:
            ops.JPEG_SPLIT_AUTO_SEGMENTS = saved_auto
    return {"rows": canonical(tr.rows), "events": tr.events}


# ---- model cases -----------------------------------------------------------------------------------------------------------------
QUANTS = (None, "int8", "mxfp8", "fp8_rowwise", "mxfp6", "mxfp4_a6", "mxfp4_a4")
FLAGS = ("fuse_attn_quant", "fuse_v_insert", "use_modulation_f32", "use_modulation_table", "fuse_cross_qnorm")
QNORM_YES = dict(ll_gemm_ssq_planes=2, ll_flash_attn_qnorm_ok=1)      # the toy model has two heads


def model_cases():
    """name -> (quant, attn_quant, {flag: value}, answers): every mode with every attention mode under the defaults, then every switch
    thrown the other way in every mode, the code-emitting attention with the kernel saying yes and no."""
    out = {}
    for q in QUANTS:
        for aq in (None, "mxfp8"):
            out[f"{q}/{aq}"] = (q, aq, {}, QNORM_YES)
            out[f"{q}/{aq}/fuse_attn_quant, kernel"] = (q, aq, {"fuse_attn_quant": True}, dict(QNORM_YES, ll_flash_attn_q_ok=1))
        out[f"{q}/None/fuse_attn_quant, two launches"] = (q, None, {"fuse_attn_quant": True}, {})
        for flag in FLAGS[1:]:
            out[f"{q}/None/{flag} off"] = (q, None, {flag: False}, QNORM_YES)
        out[f"{q}/None/qnorm kernels say no"] = (q, None, {}, {})
    return out


def run_model(name, timed=True, used=None):
    """The rows of five forward_frames calls of a two-layer toy model: three one-frame chunks that fill the window, one that rolls it,
    then a kv_only pass with a uniform timestep."""
    from longlive_amd import ops, synth
    from longlive_amd.model import CausalWanModelHIP, _QUANT_MODES
    assert set(_QUANT_MODES) == set(QUANTS), "a quantisation mode without a model case"
    quant, attn_quant, flags, answers = model_cases()[name]
    cfg = synth.toy_config(local_attn_size=3, sink_size=1)
    assert cfg.dim % 256 == 0 and cfg.ffn_dim % 256 == 0 and cfg.head_dim == 128 and cfg.num_layers == 2
    fs, dev = cfg.frame_seqlen, torch.device("cpu")
    m = CausalWanModelHIP(cfg, device="cpu")
    S = 3 * fs
    for mod in m.modules():
        if hasattr(mod, "max_attention_size"):
            mod.max_attention_size = S
    m.set_quant(quant).set_attn_quant(attn_quant)
    for flag in FLAGS:
        assert isinstance(getattr(m, flag), bool), flag
    for flag, value in flags.items():
        setattr(m, flag, value)
    inputs = {n: p.data for n, p in m.named_parameters()}
    x, t, ctx, sigma = Z(1, 1, cfg.in_dim, cfg.lat_h, cfg.lat_w), Z(1, 1, dtype=f32), Z(1, cfg.text_len, cfg.text_dim), Z(1, dtype=f32)
    kv = [dict(k=Z(1, S, cfg.num_heads, 128), v=Z(1, S, cfg.num_heads, 128), global_end_index=0, local_end_index=0) for _ in range(cfg.num_layers)]
    ca = [dict(k=Z(1, cfg.text_len, cfg.num_heads, 128), v=Z(1, cfg.text_len, cfg.num_heads, 128), is_init=False) for _ in range(cfg.num_layers)]
    inputs.update(x=x, t=t, context=ctx, sigma=sigma)
    for i in range(cfg.num_layers):
        inputs.update({f"kv{i}.k": kv[i]["k"], f"kv{i}.v": kv[i]["v"], f"cross{i}.k": ca[i]["k"], f"cross{i}.v": ca[i]["v"]})
    tr = Trace(inputs, answers)
    with host_only(tr, timed, used), tr:
        for n in range(5):
            tr.rows.append(["forward", n])
            kw = dict(kv_only=True, t_uniform=0.0) if n == 4 else dict(sigma=sigma if n % 2 else None)
            out = m.forward_frames(x, t, ctx, kv, ca, current_start=n * fs, **kw)
            tr.rows.append(["returned", tr.describe(out), [int(kv[0]["global_end_index"]), int(kv[0]["local_end_index"])]])
    assert any(r[0] == "ll_kv_roll" for r in tr.rows), "no chunk rolled the window"
    return {"rows": canonical(tr.rows), "events": tr.events}


def canonical(doc):
    """`doc` as it comes back from a JSON file (tuples are lists there)."""
    return json.loads(json.dumps(doc))


def summary(run) -> dict:
    """What the golden keeps of a model case: how often each entry was called, and the SHA-256 of all its rows."""
    counts = {}
    for row in run["rows"]:
        if row[0].startswith("ll_"):
            counts[row[0]] = counts.get(row[0], 0) + 1
    text = json.dumps(run["rows"], sort_keys=True, separators=(",", ":"))
    return {"counts": dict(sorted(counts.items())), "rows": len(run["rows"]), "sha256": hashlib.sha256(text.encode()).hexdigest()}


def signatures() -> dict:
    from longlive_amd import ops
    return {n: str(inspect.signature(f)) for n, f in public_functions(ops).items()}


def record() -> dict:
    """Everything the golden file holds, from the package that is imported now."""
    return {"signatures": signatures(), "cases": {n: run_case(n)["rows"] for n in CASES}, "model": {n: summary(run_model(n)) for n in model_cases()}}


def main(argv):
    if "--source" in argv:
        print(f"longlive_amd from {use_package_source(argv[argv.index('--source') + 1]).__file__}")
    path = argv[argv.index("--dump") + 1]
    with open(path, "w") as f:
        for name in CASES:
            f.write(f"## {name}\n")
            f.writelines(json.dumps(row) + "\n" for row in run_case(name)["rows"])
        for name in model_cases():
            f.write(f"## model {name}\n")
            f.writelines(json.dumps(row) + "\n" for row in run_model(name)["rows"])
    print(f"{path}: written")


if __name__ == "__main__":
    main(sys.argv[1:])
