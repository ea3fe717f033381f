"""Tensor-level wrappers over the C ABI.  torch is plumbing here (device memory + the current HIP stream);
all arithmetic happens in liblonglive_hip.so.  Every wrapper checks operand shapes on the host before a launch:
a kernel that faults can take the whole 8-GPU host down.
"""
from __future__ import annotations

import ctypes
import functools
import math
from dataclasses import dataclass
from typing import Optional, Tuple

import torch

from . import _lib

bf16 = torch.bfloat16

EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_GATE_RES, EPI_BIAS_RES = 0, 1, 2, 3


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


class KernelTimer:
    """HIP-event timing of individual launches on the stream they are launched on (bench.py's roofline leg).
    `ops.timer = KernelTimer()` turns it on; wrappers call timer.around(tag, work) for tagged kernels."""

    def __init__(self, tags=None):
        self.tags = None if tags is None else set(tags)
        self.records = {}          # tag -> [(start_event, end_event, work)]
        self.base = torch.cuda.Event(enable_timing=True)      # origin of the wall-clock intervals of union_ms()
        self.base.record()

    def begin(self, tag):
        if self.tags is not None and tag not in self.tags:
            return None
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        return ev

    def end(self, tag, start, work):
        if start is None:
            return
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        self.records.setdefault(tag, []).append((start, ev, work))

    def summary(self):
        """tag -> dict(launches, avg_ms, total_ms, work_per_launch) (call after a device sync)."""
        out = {}
        for tag, recs in self.records.items():
            ms = [a.elapsed_time(b) for a, b, _ in recs]
            out[tag] = dict(launches=len(ms), total_ms=sum(ms), avg_ms=sum(ms) / len(ms),
                            work_per_launch=sum(w for _, _, w in recs) / len(recs))
        return out


    def union_ms(self, tags) -> float:
        """Wall time during which at least one launch of `tags` was in flight (launches on two HIP streams overlap: the sum of
        their durations counts the shared time twice).  Call after a device sync."""
        iv = sorted((self.base.elapsed_time(a), self.base.elapsed_time(b)) for t in tags for a, b, _ in self.records.get(t, []))
        total, cur0, cur1 = 0.0, None, None
        for a, b in iv:
            if cur1 is None or a > cur1:
                if cur1 is not None:
                    total += cur1 - cur0
                cur0, cur1 = a, b
            else:
                cur1 = max(cur1, b)
        return total + ((cur1 - cur0) if cur1 is not None else 0.0)


timer: Optional[KernelTimer] = None


def _call(entry: str, *args, tag: Optional[str] = None, work: float = 0.0):
    """One launch on the current stream: entry(*args, stream), its status checked, and under `tag` timed when a KernelTimer is on.
    work = the launch's ALGORITHMIC FLOPs (MFMA kernels) or bytes (HBM-bound row kernels), SURVEY.md section 8d."""
    lib = _lib.load()
    timed = timer is not None and tag is not None
    t0 = timer.begin(tag) if timed else None
    _lib.check(getattr(lib, entry)(*args, _stream()), entry)
    if timed:
        timer.end(tag, t0, work)


def _host(entry: str, *args):
    """A host-only entry (sizes, plans): no stream, nothing launched."""
    _lib.check(getattr(_lib.load(), entry)(*args), entry)


def _plan(entry: str, *args, size: int = 256) -> str:
    """The text a *_plan entry writes about the launch it would make."""
    buf = ctypes.create_string_buffer(size)
    _host(entry, *args, buf, size)
    return buf.value.decode()


def _sizes(entry: str, *args, n: int = 2):
    """The n byte counts a *_sizes entry writes through its trailing pointers."""
    out = [ctypes.c_longlong(0) for _ in range(n)]
    _host(entry, *args, *map(ctypes.byref, out))
    return tuple(int(v.value) for v in out)


def _chk(t: torch.Tensor, name: str, dtype=bf16) -> torch.Tensor:
    if not t.is_cuda:
        raise RuntimeError(f"{name}: expected a device tensor (longlive_amd has no CPU path)")
    if t.dtype != dtype:
        raise RuntimeError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise RuntimeError(f"{name}: expected a contiguous tensor, got strides {t.stride()}")
    return t


def _ptr(t: Optional[torch.Tensor]) -> int:
    return 0 if t is None else t.data_ptr()


def _ptrs(ts) -> tuple:
    return tuple(t.data_ptr() for t in ts)


# ---- the three producers of a block linear's input, in bf16 and emitting a format's codes + scales (QFormat, below) ---------------
def _produced(fmt, x, out=None) -> tuple:
    """What a producer writes for input x: the bf16 tensor (`out` or a new one), or with a format its (codes, scales)."""
    if fmt is not None:
        return fmt.empty(tuple(x.shape), x.device)
    out = torch.empty_like(x) if out is None else _chk(out, "out")
    assert out.shape == x.shape
    return (out,)


def _ln_modulate(fmt, x, e, mod, shift_idx: int, scale_idx: int, num_frames: int, eps: float, out, tag: str):
    """LN + modulate in bf16 (fmt None) or emitting fmt's codes + scales: the same checks, another allocation and entry."""
    _chk(x, "x"); _chk(e, "e")
    B, L, Cc = x.shape
    nmod = e.shape[-2]
    assert e.shape == (B, num_frames, nmod, Cc), (e.shape, (B, num_frames, nmod, Cc)) if fmt is None else ""
    if mod is not None:
        _chk(mod, "mod")
        assert mod.numel() == nmod * Cc
    outs = _produced(fmt, x, out)
    _call("ll_ln_modulate" + ("_" + fmt.name if fmt else ""), x.data_ptr(), *_ptrs(outs), e.data_ptr(), _ptr(mod), nmod, shift_idx, scale_idx,
          B, L, Cc, num_frames, eps, tag=tag, work=(fmt.prod_bytes if fmt else 4.0) * x.numel())      # bf16: read x, write out
    return outs if fmt else outs[0]


def ln_modulate(x, e, mod, shift_idx: int, scale_idx: int, num_frames: int, eps: float, out=None, tag: str = "ln_modulate"):
    """x [B,L,C]; e [B,F,nmod,C]; mod [nmod,C] (causal_model.py:445,463-464,506-507); mod=None: `e` is a layer's slice of
    modulation_table(), i.e. already bf16(mod + e)."""
    return _ln_modulate(None, x, e, mod, shift_idx, scale_idx, num_frames, eps, out, tag)


def _ln_modulate_q(fmt: "QFormat", x, e, mod, shift_idx: int, scale_idx: int, num_frames: int, eps: float, tag: str = "ln_modulate"):
    """ln_modulate emitting the fmt codes + scales of its bf16 output."""
    return _ln_modulate(fmt, x, e, mod, shift_idx, scale_idx, num_frames, eps, None, tag)


def _modulation_table(entry: str, dtype, e, mods, *mask):
    _chk(e, "e"); _chk(mods, "mods")
    B, F, nmod, Cc = e.shape
    NL = mods.shape[0]
    assert mods.shape == (NL, nmod, Cc), (mods.shape, e.shape)
    out = torch.empty(NL, B, F, nmod, Cc, dtype=dtype, device=e.device)
    _call(entry, e.data_ptr(), mods.data_ptr(), out.data_ptr(), NL, B * F, nmod, Cc, *mask)
    return out


def modulation_table_f32(e, mods, one_plus_mask: int):
    """The fp32 form for ln_modulate_tab: [NL,B,F,nmod,C] float32 = float(bf16(mods[l] + e)), chunks in one_plus_mask
    float(bf16(1 + bf16(mods[l] + e))) -- the `1 + e[1]` of causal_model.py:445,463 once per (layer, frame)."""
    return _modulation_table("ll_modulation_table_f32", torch.float32, e, mods, int(one_plus_mask))


def _ln_modulate_tab_q(fmt: Optional["QFormat"], x, tab, shift_idx: int, scale_idx: int, num_frames: int, eps: float, tag: str = "ln_modulate"):
    """ln_modulate_tab emitting the fmt codes + scales of its bf16 output (fmt None: the bf16 output itself)."""
    _chk(x, "x"); _chk(tab, "tab", torch.float32)
    B, L, Cc = x.shape
    nmod = tab.shape[2]
    assert tab.shape == (B, num_frames, nmod, Cc), (tab.shape, (B, num_frames, nmod, Cc))
    outs = _produced(fmt, x)
    if fmt is None or fmt is Q8:      # one entry writes bf16 or int8 codes + scales, and takes a null for the other
        entry, ptrs = "ll_ln_modulate_tab", (*_ptrs(outs), 0, 0) if fmt is None else (0, *_ptrs(outs))
    else:
        entry, ptrs = "ll_ln_modulate_tab_" + fmt.name, _ptrs(outs)
    _call(entry, x.data_ptr(), *ptrs, tab.data_ptr(), nmod, shift_idx, scale_idx, B, L, Cc, num_frames, eps,
          tag=tag, work=(fmt.prod_bytes if fmt else 4.0) * B * L * Cc)
    return outs if fmt else outs[0]


def ln_modulate_tab(x, tab, shift_idx: int, scale_idx: int, num_frames: int, eps: float, q8: bool = False, tag: str = "ln_modulate"):
    """ln_modulate / ln_modulate_q8 from a layer's slice tab [B,F,nmod,C] (float32) of modulation_table_f32, whose scale chunk
    already holds 1 + scale: same bits.  Returns bf16 [B,L,C], or (int8 [B,L,C], float32 scale [B*L]) when q8 (ln_modulate_tab_q8)."""
    return _ln_modulate_tab_q(Q8 if q8 else None, x, tab, shift_idx, scale_idx, num_frames, eps, tag)


def modulation_table(e, mods):
    """e [B,F,nmod,C] (per forward), mods [NL,nmod,C] (per layer) -> [NL,B,F,nmod,C] = bf16(mods[l] + e): what every block
    computes as `self.modulation.unsqueeze(1) + e` (causal_model.py:440), for all layers in one launch."""
    return _modulation_table("ll_modulation_table", bf16, e, mods)


def _layernorm_affine(fmt, x, w, b, eps: float, out=None):
    """LayerNorm with weight and bias in bf16 (fmt None) or emitting fmt's codes + scales."""
    _chk(x, "x"); _chk(w, "w"); _chk(b, "b")
    Cc = x.shape[-1]
    assert w.numel() == Cc and b.numel() == Cc
    outs = _produced(fmt, x, out)
    _call("ll_layernorm_affine" + ("_" + fmt.name if fmt else ""), x.data_ptr(), w.data_ptr(), b.data_ptr(), *_ptrs(outs), x.numel() // Cc, Cc,
          eps, tag="layernorm_affine", work=(fmt.prod_bytes if fmt else 4.0) * x.numel())
    return outs if fmt else outs[0]


def layernorm_affine(x, w, b, eps: float, out=None):
    return _layernorm_affine(None, x, w, b, eps, out)


def _layernorm_affine_q(fmt: "QFormat", x, w, b, eps: float):
    """layernorm_affine emitting the fmt codes + scales of its bf16 output."""
    return _layernorm_affine(fmt, x, w, b, eps)


def rmsnorm(x, w, eps: float, out=None, C: Optional[int] = None):
    """RMSNorm over the first C columns of each row of a 2-D (or flattened) row-major view.  x may be a column
    slice of a wider buffer as long as its last-dim stride is 1 and rows are evenly strided."""
    assert x.dtype == bf16 and x.is_cuda and x.stride(-1) == 1
    Cc = x.shape[-1] if C is None else C
    x2 = x.flatten(0, -2) if x.dim() > 2 else x
    assert x2.dim() == 2 and x2.data_ptr() == x.data_ptr(), "rows of x must be evenly strided"
    rows, ldx = x2.shape[0], x2.stride(0)
    _chk(w, "w")
    assert w.numel() == Cc
    if out is None:
        out = torch.empty(rows, Cc, dtype=bf16, device=x.device)
    assert out.dtype == bf16 and out.is_cuda and out.stride(-1) == 1
    o2 = out.flatten(0, -2) if out.dim() > 2 else out
    assert o2.dim() == 2 and o2.data_ptr() == out.data_ptr() and o2.shape[0] == rows and o2.shape[1] >= Cc
    _call("ll_rmsnorm", x2.data_ptr(), w.data_ptr(), o2.data_ptr(), rows, Cc, ldx, o2.stride(0), eps, tag="rmsnorm", work=4.0 * rows * Cc)
    return out


def qk_norm_rope_kv_store(qkv, wq, wk, rope_f, rope_hw, q_out, cache_k, cache_v, head_dim: int, frame_len: int,
                          start_frame: int, write_start: int, roped_offset: int, write_len: int, eps: float):
    """qkv [B,L,3C] -> q_out [B,L,C]; cache_k/v [B,S,H,D] rows [write_start, +write_len) updated in place.  cache_v=None: V
    was inserted by gemm_qkv_v_insert and the v third of qkv is not read."""
    _chk(qkv, "qkv"); _chk(wq, "wq"); _chk(wk, "wk"); _chk(q_out, "q_out"); _chk(cache_k, "cache_k")
    if cache_v is not None:
        _chk(cache_v, "cache_v")
    _chk(rope_f, "rope_f", torch.float32); _chk(rope_hw, "rope_hw", torch.float32)
    B, L, C3 = qkv.shape
    Cc = C3 // 3
    assert C3 == 3 * Cc and q_out.shape == (B, L, Cc)
    S = cache_k.shape[1]
    assert cache_k.shape[0] == B and cache_k.numel() == B * S * Cc and (cache_v is None or cache_v.shape == cache_k.shape)
    half = head_dim // 2
    nf = half - 2 * (half // 3)
    assert rope_f.shape == (1024, nf, 2), rope_f.shape
    assert rope_hw.shape == (frame_len, half - nf, 2), rope_hw.shape
    nv = 1 if cache_v is not None else 0
    _call("ll_qk_norm_rope_kv_store", qkv.data_ptr(), wq.data_ptr(), wk.data_ptr(), rope_f.data_ptr(), rope_hw.data_ptr(), q_out.data_ptr(),
          cache_k.data_ptr(), _ptr(cache_v), B, L, Cc, head_dim, frame_len, start_frame, S, write_start, roped_offset, write_len, eps,
          tag="qk_norm_rope_kv_store",
          work=2.0 * ((2 + nv) * B * L * Cc + B * L * Cc + (1 + nv) * B * write_len * Cc))   # q,k(,v) in; q out; k(,v) -> cache
    return q_out


def kv_roll(cache_k, cache_v, dst: int, src: int, n: int):
    _chk(cache_k, "cache_k"); _chk(cache_v, "cache_v")
    B, S = cache_k.shape[:2]
    Cc = cache_k.numel() // (B * S)
    assert cache_v.shape == cache_k.shape
    _call("ll_kv_roll", cache_k.data_ptr(), cache_v.data_ptr(), B, S, Cc, dst, src, n,
          tag="kv_roll", work=2.0 * 2 * 2 * B * n * Cc)     # k and v, read + write, bf16


# ---- linears -----------------------------------------------------------------------------------------------------------------------
def _linear(x, w, bias, out=None, detail: bool = False):
    """Operands of out[M,N] = x[M,K] @ w[N,K]^T + bias, x any [..., K] contiguous tensor: (M, N, K, out), `out` new when None."""
    _chk(x, "x"); _chk(w, "w"); _chk(bias, "bias")
    K = x.shape[-1]
    M = x.numel() // K
    N = w.shape[0]
    assert w.shape == (N, K) and bias.numel() == N, (w.shape, bias.shape, K) if detail else ""
    if out is None:
        out = torch.empty(*x.shape[:-1], N, dtype=bf16, device=x.device)
    _chk(out, "out")
    assert out.numel() == M * N
    return M, N, K, out


def _epilogue(epilogue: int, M: int, N: int, res, e, mod, frame_len: int, detail: bool = False) -> int:
    """The operands gemm()'s epilogues read, checked: res [M,N] (EPI_BIAS_RES, EPI_BIAS_GATE_RES), e [.., nmod, N] per frame and
    mod [nmod, N] (EPI_BIAS_GATE_RES).  Returns nmod (0 without a gate)."""
    nmod = 0
    if epilogue in (EPI_BIAS_GATE_RES, EPI_BIAS_RES):
        _chk(res, "res")
        assert res.numel() == M * N
    if epilogue == EPI_BIAS_GATE_RES:
        _chk(e, "e")
        nmod = e.shape[-2]
        assert e.shape[-1] == N and e.numel() == (M // frame_len) * nmod * N, (e.shape, M, frame_len) if detail else ""
        if mod is not None:         # None: e already holds bf16(mod + e) (modulation_table)
            _chk(mod, "mod")
            assert mod.numel() == nmod * N
    return nmod


def gemm(x, w, bias, epilogue: int = EPI_BIAS, out=None, res=None, e=None, mod=None, gate_idx: int = 0,
         rows_per_batch: int = 0, frame_len: int = 0, tag: str = "gemm"):
    """out[M,N] = epilogue(x[M,K] @ w[N,K]^T + bias).  x may be any [..., K] contiguous tensor."""
    M, N, K, out = _linear(x, w, bias, out, detail=True)
    nmod = _epilogue(epilogue, M, N, res, e, mod, frame_len, detail=True)
    if M <= 1024 and M * N <= (1 << 22) and epilogue in (EPI_BIAS, EPI_BIAS_RES) and _ksplit_plan(M, N, K):
        # few rows (the text side: umT5 at 512 tokens, text K / V projections): K cut into ranges so that the grid fills the device.
        # Taken by itself only up to 1024 rows: the DiT's own linears (a 1-frame chunk has M = 1560) never come here, so the order
        # of a row's fp32 sum there does not depend on M or on the device's CU count.  Inside this region the number of ranges
        # depends on N and K only (gemm_ksplit_splits); WHETHER the path is taken still depends on M and the CU count.
        ws = ksplit_workspace(x.device, M, N, K)
        _call("ll_gemm_bf16_ksplit", x.data_ptr(), w.data_ptr(), bias.data_ptr(), out.data_ptr(), M, N, K, K, N, epilogue, _ptr(res),
              ws.data_ptr(), ws.numel(), tag=tag, work=2.0 * M * N * K)
    else:
        _call("ll_gemm_bf16", x.data_ptr(), w.data_ptr(), bias.data_ptr(), out.data_ptr(), M, N, K, K, N, epilogue, _ptr(res), _ptr(e),
              _ptr(mod), nmod, gate_idx, rows_per_batch, frame_len, tag=tag, work=2.0 * M * N * K)
    return out


def gemm_ssq_planes(M: int, N: int, K: int) -> int:
    """128-column planes ll_gemm_bf16_ssq would write for this shape under the current tuning (0 = not covered)."""
    return int(_lib.load().ll_gemm_ssq_planes(M, N, K))


def gemm_ssq(x, w, bias, out=None, tag: str = "gemm"):
    """(x @ w^T + bias [.., N] bf16, ssq [N / 128, M] fp32): the bias GEMM whose epilogue also leaves, per row and 128-column n-tile,
    the sum of squares of its bf16 outputs -- the statistics of the RMSNorm that follows a q projection (model.py:172), consumed by
    flash_attn_qnorm.  Only for shapes gemm_ssq_planes() accepts."""
    M, N, K, out = _linear(x, w, bias, out)
    planes = gemm_ssq_planes(M, N, K)
    if planes == 0:
        raise RuntimeError(f"gemm_ssq: {M} x {N} x {K} is not covered by the generated kernel (use gemm + rmsnorm)")
    ssq = torch.empty(planes, M, dtype=torch.float32, device=x.device)
    _call("ll_gemm_bf16_ssq", x.data_ptr(), w.data_ptr(), bias.data_ptr(), out.data_ptr(), ssq.data_ptr(), M, N, K, K, N,
          tag=tag, work=2.0 * M * N * K)
    return out, ssq


_ksplit_ws = {}


def _ksplit_plan(M: int, N: int, K: int) -> int:
    """K-ranges the small-M path would use (0 = not taken).  Asked per call: the answer follows the library's tuning, and only
    calls with few rows get here (the DiT's block linears do not)."""
    return int(_lib.load().ll_gemm_ksplit_plan(M, N, K))


def _dev_index(device) -> int:
    return torch.cuda.current_device() if device.index is None else device.index


def ksplit_workspace(device, M: int, N: int, K: int) -> torch.Tensor:
    """Scratch for ll_gemm_bf16_ksplit ([splits][M][N] fp32 tile sums; needs no initialisation), one buffer per (device, stream)."""
    need = int(_lib.load().ll_gemm_ksplit_workspace_bytes(M, N, K))
    key = (device.type, _dev_index(device), int(_stream() or 0))
    buf = _ksplit_ws.get(key)
    if buf is None or buf.numel() < need:
        buf = torch.empty(max(need, 16), dtype=torch.uint8, device=device)
        _ksplit_ws[key] = buf
    return buf


def _v_cache(cache_v, B: int, N: int) -> int:
    """cache_v [B, S, H, D] for the V third of a [.., N = 3C] projection: S."""
    S = cache_v.shape[1]
    assert cache_v.shape[0] == B and cache_v.numel() == B * S * (N // 3), (cache_v.shape, B, S, N)
    return S


def gemm_qkv_v_insert(x, w, bias, cache_v, write_start: int, roped_offset: int, write_len: int, xq=None, tag: str = "gemm_qkv"):
    """The fused q|k|v projection x [B,L,K] @ w [3C,K]^T + bias with the V third inserted into cache_v [B,S,H,D] by the GEMM
    epilogue (token t -> slot write_start + t - roped_offset for 0 <= t - roped_offset < write_len).  Returns the [B,L,3C]
    buffer whose q and k thirds are valid (the v third is unwritten).  xq = (int8 [B,L,K], scale [B*L]) with int8 w = (wq, sw):
    the W8A8 form (gemm_w8a8_qkv_v_insert)."""
    if xq is not None:
        B, L, _ = xq[0].shape
        assert xq[1].numel() == B * L
        return gemm_w8a8_qkv_v_insert(xq, w, bias, cache_v, write_start, roped_offset, write_len, B, L, tag=tag)
    _chk(cache_v, "cache_v")
    M, N, K, out = _linear(x, w, bias)
    B, L, _ = x.shape
    assert N % 3 == 0
    S = _v_cache(cache_v, B, N)
    _call("ll_gemm_bf16_qkv", x.data_ptr(), w.data_ptr(), bias.data_ptr(), out.data_ptr(), B * L, N, K, K, N, cache_v.data_ptr(), B, L, S,
          write_start, roped_offset, write_len, tag=tag, work=2.0 * B * L * N * K)
    return out


def quantize_rows(x, q=None, scale=None):
    """Per-row symmetric int8 quantisation of a [..., K] bf16 tensor -> (int8 [..., K], float32 scale [rows])."""
    _chk(x, "x")
    K = x.shape[-1]
    rows = x.numel() // K
    if q is None:
        q = torch.empty(x.shape, dtype=torch.int8, device=x.device)
    if scale is None:
        scale = torch.empty(rows, dtype=torch.float32, device=x.device)
    _chk(q, "q", torch.int8); _chk(scale, "scale", torch.float32)
    assert q.numel() == x.numel() and scale.numel() == rows
    _call("ll_quantize_rows", x.data_ptr(), q.data_ptr(), scale.data_ptr(), rows, K, K, tag="quantize_rows", work=3.0 * x.numel())
    return q, scale


def linear_small(x, w, bias, act_in: int = 0, act_out: int = 0):
    """Few-row linear (time embedding); rows are processed 8 at a time."""
    M, N, K, out = _linear(x, w, bias)
    x2, o2 = x.view(M, K), out.view(M, N)
    for m0 in range(0, M, 8):
        _call("ll_linear_small", x2[m0:].data_ptr(), w.data_ptr(), bias.data_ptr(), o2[m0:].data_ptr(), min(8, M - m0), N, K, act_in, act_out)
    return out


# ---- attention ---------------------------------------------------------------------------------------------------------------------
def _segs2(segments, S):
    """Up to two key ranges [(start, end), ...] within [0, S), empty ones dropped: (s0, e0, s1, e1), the second (0, 0) when absent."""
    segs = [(int(a), int(b)) for a, b in segments if b > a]
    assert 1 <= len(segs) <= 2, segments
    for a, b_ in segs:
        assert 0 <= a < b_ <= S, (segments, S)
    (s0, e0) = segs[0]
    (s1, e1) = segs[1] if len(segs) == 2 else (0, 0)
    return s0, e0, s1, e1


def _attn_q(q):
    _chk(q, "q")
    B, Lq, H, D = q.shape
    assert D == 128, "kernel is specialised for head_dim 128"
    return B, Lq, H, D


def _attn_qkv(q, k, v):
    """q [B,Lq,H,128], k and v [B,Sk,H,128], all contiguous: (B, Lq, H, D, Sk)."""
    B, Lq, H, D = _attn_q(q)
    _chk(k, "k"); _chk(v, "v")
    Sk = k.shape[1]
    assert k.shape == (B, Sk, H, D) and v.shape == k.shape
    return B, Lq, H, D, Sk


def _attn_flops(B: int, H: int, Lq: int, nkeys: int, D: int) -> float:
    return 4.0 * B * H * Lq * nkeys * D      # algorithmic FLOPs: QK^T + PV


def _attn_scale(scale, D: int) -> float:
    return 1.0 / math.sqrt(D) if scale is None else scale


def flash_attn(q, k, v, segments, out=None, scale: Optional[float] = None, tag: Optional[str] = None, out_fmt: Optional["QFormat"] = None):
    """q [B,Lq,H,128] (contiguous); k,v [B,Sk,H,128]; keys = concatenation of up to two row ranges
    [(start, end), ...] of k/v.  Returns [B,Lq,H,128], or with out_fmt (MX, MX6, MX4) the (codes, scales) of those rows as
    out_fmt.empty((B, Lq, H*128)) shapes them: the bytes quantize_<fmt>(flash_attn(...)) gives, written by the attention kernel's
    epilogue where flash_attn_q_ok says so and by the two launches otherwise."""
    if out_fmt is not None:
        return _flash_attn_q(out_fmt, q, k, v, segments, scale, tag)
    B, Lq, H, D, Sk = _attn_qkv(q, k, v)
    s0, e0, s1, e1 = _segs2(segments, Sk)
    out = torch.empty_like(q) if out is None else _chk(out, "out")
    assert out.shape == q.shape
    _call("ll_flash_attn", q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), B, Lq, H, H * D, H * D, H * D, Sk * H * D,
          s0, e0 - s0, s1, e1 - s1, _attn_scale(scale, D), tag=tag or "flash_attn", work=_attn_flops(B, H, Lq, (e0 - s0) + (e1 - s1), D))
    return out


def flash_attn_qnorm_ok(H: int, nkeys: int) -> bool:
    return bool(_lib.load().ll_flash_attn_qnorm_ok(H, nkeys))


_QFMT_ID = {"mx": 1, "mx6": 2, "mx4": 3}      # include/longlive_hip.h: enum ll_qfmt


def _qfmt_id(fmt) -> int:
    assert fmt.name in _QFMT_ID, f"attention emits the block-scaled formats only (MX, MX6, MX4), not {fmt.name}"
    return _QFMT_ID[fmt.name]


def flash_attn_q_ok(fmt, H: int, segments) -> bool:
    """Does the generated attention kernel write fmt's codes + scales itself for these key ranges (under the current tuning)?"""
    s0, e0, s1, e1 = _segs2(segments, 1 << 30)
    return bool(_lib.load().ll_flash_attn_q_ok(_qfmt_id(fmt), H, s0, e0 - s0, s1, e1 - s1))


def flash_attn_q_plan(fmt, Lq: int, H: int, B: int, segments) -> str:
    """Kernel and grid of a flash_attn(..., out_fmt=fmt) call, or that it takes two launches (host only)."""
    s0, e0, s1, e1 = _segs2(segments, 1 << 30)
    return _plan("ll_flash_attn_q_plan", _qfmt_id(fmt), Lq, H, B, s0, e0 - s0, s1, e1 - s1, size=512)


def _flash_attn_q(fmt, q, k, v, segments, scale, tag):
    B, Lq, H, D = q.shape
    if not flash_attn_q_ok(fmt, H, segments):
        return _quantize(fmt, flash_attn(q, k, v, segments, scale=scale, tag=tag).view(B, Lq, H * D))
    B, Lq, H, D, Sk = _attn_qkv(q, k, v)
    s0, e0, s1, e1 = _segs2(segments, Sk)
    codes, scales = fmt.empty((B, Lq, H * D), q.device)
    _call("ll_flash_attn_q", _qfmt_id(fmt), q.data_ptr(), k.data_ptr(), v.data_ptr(), codes.data_ptr(), scales.data_ptr(), B, Lq, H, H * D,
          codes.shape[-1], scales.shape[-1], H * D, Sk * H * D, s0, e0 - s0, s1, e1 - s1, _attn_scale(scale, D),
          tag=tag or "flash_attn", work=_attn_flops(B, H, Lq, (e0 - s0) + (e1 - s1), D))
    return codes, scales


def flash_attn_qnorm(q, ssq, norm_w, eps: float, k, v, nkeys: int, out=None, scale: Optional[float] = None, tag: Optional[str] = None):
    """Attention over keys [0, nkeys) of k / v with WanRMSNorm(q; norm_w) applied inside the kernel: q [B,Lq,H,128] is the RAW
    projection output and ssq [H, B*Lq] its per-plane row sums of squares (gemm_ssq).  model.py:172,189 in two launches."""
    _chk(q, "q"); _chk(k, "k"); _chk(v, "v"); _chk(norm_w, "norm_w"); _chk(ssq, "ssq", torch.float32)
    B, Lq, H, D = q.shape
    assert D == 128 and norm_w.numel() == H * D and ssq.shape == (H, B * Lq), (q.shape, ssq.shape, norm_w.shape)
    Sk = _attn_qkv(q, k, v)[4]
    assert 0 < nkeys <= Sk
    out = torch.empty_like(q) if out is None else _chk(out, "out")
    assert out.shape == q.shape
    _call("ll_flash_attn_qnorm", q.data_ptr(), ssq.data_ptr(), norm_w.data_ptr(), eps, k.data_ptr(), v.data_ptr(), out.data_ptr(),
          B, Lq, H, H * D, H * D, H * D, Sk * H * D, 0, nkeys, _attn_scale(scale, D),
          tag=tag or "flash_attn", work=_attn_flops(B, H, Lq, nkeys, D))
    return out


def patchify(x):
    """x [B,F,Cin,H,W] -> [B, F*(H/2)*(W/2), Cin*4]."""
    _chk(x, "x")
    B, F, Cin, H, W = x.shape
    out = torch.empty(B, F * (H // 2) * (W // 2), Cin * 4, dtype=bf16, device=x.device)
    _call("ll_patchify", x.data_ptr(), out.data_ptr(), B, F, Cin, H, W)
    return out


def sinusoid(t, dim: int):
    """t float32 [n] -> bf16 [n, dim]."""
    _chk(t, "t", torch.float32)
    n = t.numel()
    out = torch.empty(n, dim, dtype=bf16, device=t.device)
    _call("ll_sinusoid", t.data_ptr(), out.data_ptr(), n, dim)
    return out


def unpatchify_x0(head, xt, sigma) -> Tuple[torch.Tensor, torch.Tensor]:
    """head [B, F*h*w, 4*Cout]; xt [B,F,Cout,H,W]; sigma float32 [B*F] -> (flow, x0) [B,F,Cout,H,W]."""
    _chk(head, "head"); _chk(xt, "xt"); _chk(sigma, "sigma", torch.float32)
    B, F, Cout, H, W = xt.shape
    assert head.shape == (B, F * (H // 2) * (W // 2), 4 * Cout), head.shape
    assert sigma.numel() == B * F
    flow, x0 = torch.empty_like(xt), torch.empty_like(xt)
    _call("ll_unpatchify_x0", head.data_ptr(), xt.data_ptr(), sigma.data_ptr(), flow.data_ptr(), x0.data_ptr(), B, F, Cout, H, W)
    return flow, x0


def add_noise(x0, noise, sigma):
    """x0, noise [N, ...]; sigma float32 [N] -> bf16((1-sigma) x0 + sigma noise)."""
    _chk(x0, "x0"); _chk(noise, "noise"); _chk(sigma, "sigma", torch.float32)
    N = x0.shape[0]
    assert noise.shape == x0.shape and sigma.numel() == N
    out = torch.empty_like(x0)
    _call("ll_add_noise", x0.data_ptr(), noise.data_ptr(), sigma.data_ptr(), out.data_ptr(), N, x0.numel() // N)
    return out


def sigma_lookup(t, timesteps, sigmas):
    """t float32 [n] (device) -> sigmas[argmin |timesteps - t|] float32 [n]."""
    _chk(t, "t", torch.float32); _chk(timesteps, "timesteps", torch.float32); _chk(sigmas, "sigmas", torch.float32)
    assert timesteps.numel() == sigmas.numel()
    out = torch.empty(t.numel(), dtype=torch.float32, device=t.device)
    _call("ll_sigma_lookup", t.data_ptr(), timesteps.data_ptr(), sigmas.data_ptr(), out.data_ptr(), t.numel(), timesteps.numel())
    return out


# ---- VAE decoder (channels-last) -------------------------------------------------------------------------------------
_zero16 = {}


def zero_row(device) -> torch.Tensor:
    """64 zero bytes on `device`: the source of every padding chunk of the implicit-GEMM convolution."""
    key = str(device)
    if key not in _zero16:
        _zero16[key] = torch.zeros(32, dtype=bf16, device=device)
    return _zero16[key]


def pack_conv_weight(w: torch.Tensor, bias: torch.Tensor):
    """Reference conv weight [Cout, Cin, (kt,) kh, kw] -> the kernel's [Cout8, Kpad] bf16 with k = (tap, ci), rows padded
    to a multiple of 8 output channels and K to a multiple of 64 (zeros), plus the padded bias.  One-time, at load."""
    if w.dim() == 4:
        w = w.unsqueeze(2)
    cout, cin, kt, kh, kw = w.shape
    assert kh == kw
    k = kt * kh * kw * cin
    kpad = (k + 63) // 64 * 64
    cout8 = (cout + 7) // 8 * 8
    packed = torch.zeros(cout8, kpad, dtype=bf16, device=w.device)
    packed[:cout, :k] = w.permute(0, 2, 3, 4, 1).reshape(cout, k).to(bf16)
    b = torch.zeros(cout8, dtype=bf16, device=w.device)
    b[:cout] = bias.to(bf16)
    return packed.contiguous(), b, (cin, cout8, kpad, kt, kh)


def _conv_in(x, packed, bias, geo, hist: int, name: Optional[str] = None, takes: str = ""):
    """Input, weights and bias of a channels-last convolution against its pack_conv_weight geometry: x is [hist + T, H, W, Cin], the
    stream's previous `hist` input frames first.  Returns (T, H, W).  `name`: the wrapper the refusals speak for."""
    cin, cout, kpad, kt, kh = geo
    _chk(x, "x"); _chk(packed, "w"); _chk(bias, "bias")
    T, H, W, C = x.shape[0] - hist, x.shape[1], x.shape[2], x.shape[3]
    assert T >= 1, f"{name}: {takes}" if name else ""
    assert C == cin, f"{name}: input has {C} channels, weights expect {cin}" if name else ""
    assert packed.shape == (cout, kpad) and bias.numel() == cout
    return T, H, W


def conv_cl(x, packed, bias, geo, upsample: bool = False, res=None, out=None):
    """Channels-last convolution.  Temporal kernels (kt == 3): x is [2 + T, H, W, Cin] -- the stream's previous two input
    frames (zeros at its start) followed by the T new ones; otherwise x is [T, H, W, Cin].  packed/bias/geo from
    pack_conv_weight.  Returns [T, H<<up, W<<up, Cout8]."""
    cin, cout, kpad, kt, kh = geo
    hist = 2 if kt > 1 else 0
    T, H, W = _conv_in(x, packed, bias, geo, hist, "conv_cl", "a temporal convolution takes [2 + T, H, W, Cin] (two history frames first)")
    Ho, Wo = (2 * H, 2 * W) if upsample else (H, W)
    if out is None:
        out = torch.empty(T, Ho, Wo, cout, dtype=bf16, device=x.device)
    assert out.shape == (T, Ho, Wo, cout) and out.is_contiguous() and out.dtype == bf16
    if res is not None:
        _chk(res, "res")
        assert res.shape == out.shape
    _call("ll_conv_cl", x[hist:].data_ptr(), zero_row(x.device).data_ptr(), packed.data_ptr(), bias.data_ptr(), _ptr(res), out.data_ptr(),
          T, H, W, cin, cout, kpad, kt, kh, 1 if upsample else 0, cout, tag="conv", work=2.0 * T * Ho * Wo * cout * (kt * kh * kh * cin))
    return out


def conv_cl_rms_ok(geo, H: int, W: int, upsample: bool = False) -> bool:
    """conv_cl_rms covers this convolution (the halo-tile kernel with every channel of a pixel in one workgroup: Cout = 96)."""
    cin, cout, kpad, kt, kh = geo
    return bool(_lib.load().ll_conv_cl_rms_ok(H, W, cin, cout, kt, kh, 1 if upsample else 0))


def conv_cl_rms(x, packed, bias, geo, gamma, out_rms, silu: bool = True, upsample: bool = False, res=None, want_raw: bool = False):
    """conv_cl + the RMS_norm (+ SiLU) of its result in ONE launch: out_rms [T, Ho, Wo, Cout] = rms_silu(conv(x) [+ res]) -- what
    ResidualBlock feeds its next convolution (vae.py:193-220).  want_raw: also return the un-normalised tensor (the next block's
    shortcut), else None.  Only where conv_cl_rms_ok(...)."""
    cin, cout, kpad, kt, kh = geo
    hist = 2 if kt > 1 else 0
    T, H, W = _conv_in(x, packed, bias, geo, hist)
    _chk(gamma, "gamma"); _chk(out_rms, "out_rms")
    assert gamma.numel() == cout
    Ho, Wo = (2 * H, 2 * W) if upsample else (H, W)
    assert out_rms.shape == (T, Ho, Wo, cout) and out_rms.is_contiguous()
    out = torch.empty(T, Ho, Wo, cout, dtype=bf16, device=x.device) if want_raw else None
    if res is not None:
        _chk(res, "res")
        assert res.shape == out_rms.shape
    _call("ll_conv_cl_rms", x[hist:].data_ptr(), zero_row(x.device).data_ptr(), packed.data_ptr(), bias.data_ptr(), _ptr(res), _ptr(out),
          gamma.data_ptr(), out_rms.data_ptr(), 1 if silu else 0, T, H, W, cin, cout, kpad, kt, kh, 1 if upsample else 0, cout,
          tag="conv", work=2.0 * T * Ho * Wo * cout * (kt * kh * kh * cin))
    return out


def rms_silu_cl(x, gamma, silu: bool = True, out=None):
    _chk(x, "x"); _chk(gamma, "gamma")
    C = x.shape[-1]
    assert gamma.numel() == C
    if out is None:
        out = torch.empty_like(x)
    _call("ll_rms_silu_cl", x.data_ptr(), gamma.data_ptr(), out.data_ptr(), x.numel() // C, C, 1 if silu else 0)
    return out


def softmax_rows(s, scale: float, n_valid: Optional[int] = None, out=None):
    """softmax(scale * s[:, :n_valid]) along the last dim; columns >= n_valid come out as zeros."""
    _chk(s, "s")
    ld = s.shape[-1]
    N = ld if n_valid is None else n_valid
    if out is None:
        out = torch.empty_like(s)
    _call("ll_softmax_rows", s.data_ptr(), out.data_ptr(), s.numel() // ld, N, ld, float(scale))
    return out


def vae_unscale_cl(z, mean, inv_std):
    """z [T, C, h, w] bf16 -> bf16(bf16(z / inv_std) + mean) as channels-last [T, h, w, C]."""
    _chk(z, "z"); _chk(mean, "mean"); _chk(inv_std, "inv_std")
    T, C, h, w = z.shape
    assert mean.numel() == C and inv_std.numel() == C
    out = torch.empty(T, h, w, C, dtype=bf16, device=z.device)
    _call("ll_vae_unscale_cl", z.data_ptr(), mean.data_ptr(), inv_std.data_ptr(), out.data_ptr(), T, C, h, w)
    return out


def cl_to_tchw_clamp(x):
    """[T,H,W,C>=3] bf16 channels-last -> fp32 [T,3,H,W] clamped to [-1,1]."""
    _chk(x, "x")
    T, H, W, C = x.shape
    out = torch.empty(T, 3, H, W, dtype=torch.float32, device=x.device)
    _call("ll_cl_to_tchw_clamp", x.data_ptr(), out.data_ptr(), T, H, W, C)
    return out


# ---- frames out: uint8 frames from the decoder, baseline JPEG ----------------------------------------------------------
def _u8_items(t, name: str, shape_ok: bool, shape: str):
    """A uint8 device tensor [T, ...] of the stated shape -- frames [H, W, 3], planes [h, w], rows [n] -- with each item contiguous and
    the items not overlapping (copied when they are not), and its item stride in bytes.  The stride of a single item is its size:
    torch leaves the stride of a dimension of one undefined."""
    if not t.is_cuda:
        raise RuntimeError(f"{name}: expected a device tensor (longlive_amd has no CPU path)")
    if t.dtype != torch.uint8:
        raise RuntimeError(f"{name}: expected uint8, got {t.dtype}")
    assert shape_ok, f"{name}: {tuple(t.shape)} is not {shape}"
    T, n = t.shape[0], math.prod(t.shape[1:])
    if t.stride()[1:] != _item_strides(t) or (T > 1 and t.stride(0) < n):
        t = t.contiguous()
    return t, (t.stride(0) if T > 1 else n)


def _item_strides(t) -> tuple:
    strides, n = [], 1
    for d in reversed(t.shape[1:]):
        strides.append(n)
        n *= d
    return tuple(reversed(strides))


def _frames_u8(frames, what: str):
    """uint8 [T, H, W, 3] on the device with contiguous frames (copied when they are not) and its frame stride in bytes."""
    return _u8_items(frames, what, frames.dim() == 4 and frames.shape[3] == 3, "[T, H, W, 3]")


def _u8_out(out, shape: tuple, device, what: str):
    """`out` (new when None): a uint8 device tensor of `shape` = [T, ...] whose items -- frames [H, W, 3], I420 frames [n] -- are
    contiguous and do not overlap, at any stride; and that stride in bytes."""
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=device)
    if not out.is_cuda or out.dtype != torch.uint8:
        raise RuntimeError("out: expected a uint8 device tensor")
    assert out.shape == shape and out.stride()[1:] == _item_strides(out), f"out: {tuple(out.shape)} strides {out.stride()} is not {what} with contiguous frames"
    n = math.prod(shape[1:])
    stride = out.stride(0) if shape[0] > 1 else n
    assert stride >= n
    return out, stride


def _frames_out(out, T: int, H: int, W: int, device):
    return _u8_out(out, (T, H, W, 3), device, "[T, H, W, 3]")


def cl_to_frames_u8(x, out=None):
    """[T,H,W,C>=3] bf16 channels-last -> uint8 [T,H,W,3]: `(255.0 * (cl_to_tchw_clamp(x) * 0.5 + 0.5).clamp(0, 1)).to(uint8)` laid out
    frame by frame, bit for bit, in one pass.  `out`: a uint8 [T,H,W,3] view whose frames are contiguous (any frame stride)."""
    _chk(x, "x")
    T, H, W, C = x.shape
    out, stride_t = _frames_out(out, T, H, W, x.device)
    _call("ll_cl_to_frames_u8", x.data_ptr(), out.data_ptr(), stride_t, T, H, W, C)
    return out


def _encode(entry: str, sizes, src, *head):
    """The body of the three encoders: entry(src, *head, buf, out_stride, sizes, scratch, scratch_bytes) for T = src.shape[0] items,
    with `sizes` = (out_stride, scratch_bytes) as the encoder's *_sizes entry gives them.  Returns (buf uint8 [T, out_stride], sizes
    int32 [T])."""
    out_stride, scratch_bytes = sizes
    T = src.shape[0]
    buf = torch.empty(T, out_stride, dtype=torch.uint8, device=src.device)
    used = torch.empty(T, dtype=torch.int32, device=src.device)
    scratch = torch.empty(scratch_bytes, dtype=torch.uint8, device=src.device)
    _call(entry, src.data_ptr(), *head, buf.data_ptr(), out_stride, used.data_ptr(), scratch.data_ptr(), scratch_bytes)
    return buf, used


def jpeg_sizes(T: int, H: int, W: int):
    """(out_stride, scratch_bytes) of ll_jpeg_encode_u8 for T frames of H x W (host only)."""
    return _sizes("ll_jpeg_sizes", T, H, W)


def jpeg_encode(frames, quality: int = 90):
    """uint8 frames [T, H, W, 3] RGB (or a view with contiguous frames) -> (buf uint8 [T, out_stride], sizes int32 [T]): frame t's
    baseline JPEG file (4:2:0, one restart interval per MCU row) is buf[t, :sizes[t]].  Stream-ordered: nothing is read back."""
    frames, stride_t = _frames_u8(frames, "frames")
    T, H, W, _ = frames.shape
    return _encode("ll_jpeg_encode_u8", jpeg_sizes(T, H, W), frames, stride_t, T, H, W, int(quality))


def jpeg_bytes(buf, sizes) -> list:
    """The files of jpeg_encode on the host: one copy of `sizes`, then one of the bytes in use."""
    n = sizes.cpu().tolist()
    if not n:
        return []
    width = max(n)
    host = buf[:, :width].cpu().numpy()
    return [host[t, :k].tobytes() for t, k in enumerate(n)]


def jpeg_coefficients(frames, quality: int = 90):
    """The encoder's first stage alone: int16 [T, ceil(H/16), ceil(W/16), 6, 64], blocks Y00 Y01 Y10 Y11 Cb Cr in zigzag order."""
    frames, stride_t = _frames_u8(frames, "frames")
    T, H, W, _ = frames.shape
    coef = torch.empty(T, (H + 15) // 16, (W + 15) // 16, 6, 64, dtype=torch.int16, device=frames.device)
    _call("ll_jpeg_coefficients_u8", frames.data_ptr(), stride_t, T, H, W, int(quality), coef.data_ptr())
    return coef


# ---- lossless frames out: PNG files and the zlib compressor inside them ("Lossless frames: PNG") ----
def png_sizes(T: int, H: int, W: int):
    """(out_stride, scratch_bytes) of ll_png_encode_u8 for T frames of H x W (host only)."""
    return _sizes("ll_png_sizes", T, H, W)


def png_encode(frames):
    """uint8 frames [T, H, W, 3] RGB (or a view with contiguous frames) -> (buf uint8 [T, out_stride], sizes int32 [T]): frame t's PNG
    file (8-bit RGB, lossless) is buf[t, :sizes[t]].  Stream-ordered: nothing is read back."""
    frames, stride_t = _frames_u8(frames, "frames")
    T, H, W, _ = frames.shape
    return _encode("ll_png_encode_u8", png_sizes(T, H, W), frames, stride_t, T, H, W)


png_bytes = jpeg_bytes      # the files of png_encode on the host: the same one read


def png_filter(frames):
    """The encoder's first stage alone: uint8 [T, H, 1 + 3W], each row's filter type and its filtered bytes."""
    frames, stride_t = _frames_u8(frames, "frames")
    T, H, W, _ = frames.shape
    out = torch.empty(T, H, 1 + 3 * W, dtype=torch.uint8, device=frames.device)
    _call("ll_png_filter_u8", frames.data_ptr(), stride_t, T, H, W, out.data_ptr())
    return out


def zlib_sizes(T: int, n: int):
    """(out_stride, scratch_bytes) of ll_zlib_compress_u8 for T rows of n bytes (host only)."""
    return _sizes("ll_zlib_sizes", T, n)


def zlib_compress(rows):
    """uint8 rows [T, n] (unit stride along n, any row stride) -> (buf uint8 [T, out_stride], sizes int32 [T]): row t's zlib stream
    (the PNG encoder's deterministic DEFLATE, which zlib.decompress reads) is buf[t, :sizes[t]].  Stream-ordered."""
    rows, stride = _u8_items(rows, "rows", rows.dim() == 2, "[T, n]")
    T, n = rows.shape
    return _encode("ll_zlib_compress_u8", zlib_sizes(T, n), rows, stride, T, n)


# ---- planar YUV: I420 frames out, planes of six layouts in ("Planar YUV and Y4M") -----------------
YUV_RANGES = ("limited", "full")
YUV_LAYOUTS = ("420jpeg", "420mpeg2", "420paldv", "422", "444", "mono")     # the index is ll_yuv_to_frames_u8's `layout`


def _yuv_full(range) -> int:
    if range not in YUV_RANGES:
        raise ValueError(f"range: {range!r} is not one of {', '.join(YUV_RANGES)}")
    return int(range == "full")


def yuv420_bytes(H: int, W: int) -> int:
    """Bytes of one I420 frame: the Y plane, then Cb and Cr of ceil(H/2) x ceil(W/2)."""
    return int(H) * int(W) + 2 * ((int(H) + 1) // 2) * ((int(W) + 1) // 2)


def yuv_chroma_shape(layout: str, H: int, W: int):
    """(Hc, Wc) of a layout's chroma planes; (0, 0) for mono."""
    if layout not in YUV_LAYOUTS:
        raise ValueError(f"layout: {layout!r} is not one of {', '.join(YUV_LAYOUTS)}")
    if layout == "mono":
        return 0, 0
    return (H if layout in ("422", "444") else (H + 1) // 2), (W if layout == "444" else (W + 1) // 2)


def _yuv420_out(out, T: int, H: int, W: int, device):
    n = yuv420_bytes(H, W)
    return _u8_out(out, (T, n), device, f"[T, {n}]")


def frames_u8_to_yuv420(frames, range: str = "limited", out=None):
    """uint8 frames [T, H, W, 3] RGB -> uint8 [T, yuv420_bytes(H, W)]: I420 frames (BT.601, chroma at the centre of its 2 x 2 pixels,
    `range` limited or full), the integer arithmetic of csrc/yuv.h.  `out`: a uint8 [T, yuv420_bytes] view with contiguous frames."""
    full = _yuv_full(range)
    frames, stride_t = _frames_u8(frames, "frames")
    T, H, W, _ = frames.shape
    out, ost = _yuv420_out(out, T, H, W, frames.device)
    _call("ll_frames_u8_to_yuv420", frames.data_ptr(), stride_t, T, H, W, full, out.data_ptr(), ost)
    return out


def cl_to_yuv420(x, range: str = "limited", out=None):
    """[T,H,W,C>=3] bf16 channels-last -> uint8 [T, yuv420_bytes(H, W)]: frames_u8_to_yuv420(cl_to_frames_u8(x)) bit for bit, in one
    pass without the RGB bytes touching memory."""
    full = _yuv_full(range)
    _chk(x, "x")
    T, H, W, C = x.shape
    out, ost = _yuv420_out(out, T, H, W, x.device)
    _call("ll_cl_to_yuv420", x.data_ptr(), T, H, W, C, full, out.data_ptr(), ost)
    return out


def yuv420_planes(buf, H: int, W: int):
    """Views (y [..., H, W], cb [..., Hc, Wc], cr [..., Hc, Wc]) of I420 frames buf [..., yuv420_bytes(H, W)]."""
    hc, wc = (H + 1) // 2, (W + 1) // 2
    assert buf.shape[-1] == yuv420_bytes(H, W), f"buf: {tuple(buf.shape)} does not hold {H} x {W} I420 frames"
    return (buf[..., :H * W].unflatten(-1, (H, W)), buf[..., H * W:H * W + hc * wc].unflatten(-1, (hc, wc)),
            buf[..., H * W + hc * wc:].unflatten(-1, (hc, wc)))


def _yuv_plane(p, name: str, T: int, h: int, w: int):
    """A [T, h, w] uint8 device plane stack with contiguous planes (copied when they are not) and its plane stride in bytes."""
    return _u8_items(p, name, tuple(p.shape) == (T, h, w), f"[{T}, {h}, {w}]")


def yuv_to_frames_u8(y, cb=None, cr=None, layout: str = "420jpeg", range: str = "limited", out=None):
    """Planes y [T, H, W], cb / cr [T, Hc, Wc] (yuv_chroma_shape; None for mono) -> uint8 frames [T, H, W, 3] RGB: BT.601, chroma
    interpolated to luma resolution as the layout sites it (csrc/yuv.h).  The planes may be views of packed payloads (any plane
    stride); cb and cr must share one.  `out`: a uint8 [T, H, W, 3] view with contiguous frames."""
    full = _yuv_full(range)
    if y.dim() != 3:
        raise RuntimeError(f"y: {tuple(y.shape)} is not [T, H, W]")
    T, H, W = y.shape
    hc, wc = yuv_chroma_shape(layout, H, W)
    y, sty = _yuv_plane(y, "y", T, H, W)
    stc = 0
    if layout == "mono":
        cb = cr = None
    else:
        if cb is None or cr is None:
            raise RuntimeError(f"cb, cr: layout {layout} needs both chroma planes")
        cb, stc = _yuv_plane(cb, "cb", T, hc, wc)
        cr, stc_r = _yuv_plane(cr, "cr", T, hc, wc)
        if stc_r != stc:
            cb, cr = cb.contiguous(), cr.contiguous()
            stc = hc * wc
    out, ost = _frames_out(out, T, H, W, y.device)
    _call("ll_yuv_to_frames_u8", y.data_ptr(), _ptr(cb), _ptr(cr), sty, stc, T, H, W, YUV_LAYOUTS.index(layout), full, out.data_ptr(), ost)
    return out


# ---- clip intake: baseline JPEG decoder, antialiased resize ------------------------------------------------------------
# split="auto" (profiles/clip_intake.md): 1024 bytes per subsequence, so only segments of 4 KiB and more are
# cut, and only in a clip of fewer than 1024 segments: the split route decodes every byte about three times (pass 0, the rescan, the
# emit), which pays when a clip offers a few dozen lanes (81 no-DRI frames: 7.8 times faster) and loses when its restart intervals
# already fill the device (2430 segments: the serial route is 1.8 to 3.7 times faster).  Between 81 and 2430 nothing is measured;
# 1024 segments are four one-lane waves per CU.  12 rounds: the longest settle round measured at 256 bytes and more is 7.
JPEG_SPLIT_AUTO = 1024
JPEG_SPLIT_AUTO_SEGMENTS = 1024
JPEG_SPLIT_ROUNDS = 12


def jpeg_decode_sizes(T: int, H: int, W: int, components: int, hs: int, vs: int, split=None, rounds=None):
    """(coef_bytes, scratch_bytes) of ll_jpeg_decode_u8 (host only); with split=(segments, subsequences), the shape of the split table,
    also the work bytes of ll_jpeg_decode_u8_split: (coef_bytes, scratch_bytes, work_bytes).  `rounds` is checked, it changes no size."""
    sizes = _sizes("ll_jpeg_decode_sizes", T, H, W, components, hs, vs)
    if split is None:
        return sizes
    _jpeg_rounds(rounds)
    return sizes + _sizes("ll_jpeg_decode_split_sizes", int(split[0]), int(split[1]), n=1)


def _jpeg_rounds(rounds) -> int:
    if rounds is None:
        return JPEG_SPLIT_ROUNDS
    if isinstance(rounds, bool) or not isinstance(rounds, int) or not 1 <= rounds <= 64:
        raise ValueError(f"rounds: {rounds!r} must be an integer 1..64")
    return rounds


def _jpeg_split_bytes(split):
    """split=None -> None (the serial route), "auto" -> JPEG_SPLIT_AUTO, an int -> that many bytes per subsequence."""
    if split is None:
        return None
    if isinstance(split, str) and split.strip().lower() == "auto":
        return JPEG_SPLIT_AUTO
    if isinstance(split, bool) or not isinstance(split, int) or split < 8 or split % 4:
        raise ValueError(f"split: {split!r} must be None, 'auto' or a multiple of 4 bytes, at least 8")
    return split


def _jpeg_upload(files, device, split=None, auto=False):
    """pack_jpegs(files) and its arrays on the device, sent as ONE buffer: (packed, {name: device view}); with `split` (bytes per
    subsequence) the split table goes along as "subs" (absent when no segment is long enough to be cut, and under `auto` when the
    clip has JPEG_SPLIT_AUTO_SEGMENTS segments or more)."""
    import numpy as np
    from . import jpeg_files
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device())
    if torch.device(device).type != "cuda":
        raise RuntimeError("jpeg_decode: expected a device (longlive_amd has no CPU path)")
    pk = jpeg_files.pack_jpegs(files)
    parts = {"segs": pk.segs, "qt": pk.qt, "huff": pk.huff, "sel": pk.sel, "data": pk.data}
    if split is not None and not (auto and pk.segs.shape[0] >= JPEG_SPLIT_AUTO_SEGMENTS):
        subs = jpeg_files.split_segments(pk, split)
        if subs.shape[0]:
            parts["subs"] = subs
    offs, n = {}, 0
    for k, a in parts.items():
        offs[k] = n
        n += (a.nbytes + 15) // 16 * 16
    blob = np.zeros(max(n, 16), dtype=np.uint8)
    for k, a in parts.items():
        blob[offs[k]:offs[k] + a.nbytes] = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    dev = torch.from_numpy(blob).to(device)
    return pk, {k: dev[offs[k]:offs[k] + max(a.nbytes, 1)] for k, a in parts.items()}


def _jpeg_status(status, pk):
    bad = {}
    for s, code in enumerate(status.cpu().tolist()):
        if code:
            bad.setdefault(int(pk.segs[s, 2]), code)
    if bad:
        raise ValueError("jpeg_decode: malformed entropy-coded data in frame" + ("s " if len(bad) > 1 else " ") +
                         ", ".join(f"{t} (code {c})" for t, c in sorted(bad.items())))


def _jpeg_coef_out(pk, device, coef):
    rows, cols, bpm = pk.grid
    shape = (pk.frames, rows, cols, bpm, 64)
    if coef is None:
        coef = torch.empty(shape, dtype=torch.int16, device=device)
    assert coef.is_cuda and coef.dtype == torch.int16 and tuple(coef.shape) == shape and coef.is_contiguous(), \
        f"coef: expected a contiguous int16 device tensor {shape}"
    return coef


def _jpeg_split_args(pk, d, device, rounds, info, work):
    """(status, info, the split entry points' trailing arguments or None when the clip has no subsequence).  Without an `info` of the
    caller's, status and info are the two rows of one tensor, so that `check` reads both back in one copy."""
    nseg = pk.segs.shape[0]
    if info is None:
        both = torch.zeros(2, nseg, dtype=torch.int32, device=device)
        status, info = both[0], both[1]
    else:
        assert info.is_cuda and info.dtype == torch.int32 and info.shape == (nseg,) and info.is_contiguous(), \
            f"info: expected a contiguous int32 device tensor [{nseg}]"
        status = torch.empty(nseg, dtype=torch.int32, device=device)
    if "subs" not in d:                                 # every segment is too short to cut: the serial route, info 0 throughout
        info.zero_()
        return status, info, None
    nsub = d["subs"].numel() // 12
    work_bytes = jpeg_decode_sizes(pk.frames, pk.height, pk.width, pk.components, pk.hs, pk.vs, split=(nseg, nsub), rounds=rounds)[2]
    if work is None:
        work = torch.empty(work_bytes, dtype=torch.uint8, device=device)
    assert work.is_cuda and work.dtype == torch.uint8 and work.numel() >= work_bytes and work.is_contiguous()
    return status, info, (d["subs"].data_ptr(), nsub, rounds, info.data_ptr(), work.data_ptr(), work.numel())


def _jpeg_checked(status, info, pk):
    """One read-back of status and info where they share a tensor."""
    if status._base is not None and status._base is info._base:
        host = status._base.cpu()
        _jpeg_status(host[0], pk)
    else:
        _jpeg_status(status, pk)


def _jpeg_launch(entry: str, head, mid, pk, d, device, sub, rounds, check: bool, return_info: bool, info, work, refusal: str):
    """entry(*head, status, *mid) on the serial route (sub None, or no segment long enough to cut), entry_split(.., *tail) on the split
    route; the status read back once under `check`.  Returns info (None on the serial route)."""
    if sub is None:
        if return_info or info is not None or work is not None:
            raise ValueError(refusal)
        status = torch.empty(pk.segs.shape[0], dtype=torch.int32, device=device)
        _call(entry, *head, status.data_ptr(), *mid)
        if check:
            _jpeg_status(status, pk)
        return None
    status, info, tail = _jpeg_split_args(pk, d, device, _jpeg_rounds(rounds), info, work)
    if tail is None:
        _call(entry, *head, status.data_ptr(), *mid)
    else:
        _call(entry + "_split", *head, status.data_ptr(), *mid, *tail)
    if check:
        _jpeg_checked(status, info, pk)
    return info


def jpeg_decode_coefficients(files, device=None, out=None, check: bool = True, split=None, rounds=None, return_info: bool = False,
                             info=None, work=None):
    """Baseline JPEG files (bytes, same size and sampling) -> int16 [T, rows, cols, bpm, 64] on the device: the entropy stage alone, in
    zigzag order, blocks in scan order (for 4:2:0 the layout of jpeg_coefficients).  `check` reads the segments' status back once and
    raises ValueError naming the frames whose data is malformed.  split / rounds / return_info / info / work: as in jpeg_decode."""
    sub = _jpeg_split_bytes(split)
    pk, d = _jpeg_upload(files, device, sub, auto=isinstance(split, str))
    coef = _jpeg_coef_out(pk, d["data"].device, out)
    head = (d["data"].data_ptr(), pk.data.nbytes, d["segs"].data_ptr(), pk.segs.shape[0], d["huff"].data_ptr(), d["sel"].data_ptr(),
            pk.frames, pk.height, pk.width, pk.components, pk.hs, pk.vs, coef.data_ptr())
    info = _jpeg_launch("ll_jpeg_decode_coefficients", head, (), pk, d, coef.device, sub, rounds, check, return_info, info, work,
                        "return_info, info and work belong to the split route: pass split=")
    return (coef, info) if return_info else coef


def jpeg_decode(files, device=None, check: bool = True, out=None, scratch=None, split=None, rounds=None, return_info: bool = False,
                info=None):
    """Baseline JPEG files (bytes; grey, 4:4:4, 4:2:2 or 4:2:0, all of one size and sampling) -> uint8 [T, H, W, 3] RGB on the device.
    One host-to-device copy of the packed bytes and tables, three launches.  `check` reads the segments' status back once and raises
    ValueError naming the frames whose entropy data is malformed.  `out`: a uint8 [T, H, W, 3] view with contiguous frames (any
    frame stride); `scratch`: (coef int16, planes uint8) to decode into, any content.

    split: None = one lane per restart segment, as ever; an int = the entropy stage decodes subsequences of that many bytes side by
    side (csrc/jpeg_dec.hip's split route: the same coefficients and status, bit for bit; rounds + 6 launches in its place);
    "auto" = JPEG_SPLIT_AUTO bytes where the clip has fewer than JPEG_SPLIT_AUTO_SEGMENTS segments, else the serial route.  rounds (default JPEG_SPLIT_ROUNDS): resynchronisation rounds; a segment that needs more is
    decoded serially.  The split table rides in the same one copy, `check` still reads back once (status and info together), and
    return_info=True returns (frames, info): per segment 0 = serial by table, r >= 1 = settled in round r, -1 / -2 = fell back
    unsettled / flagged.  `info`: an int32 [segments] tensor to write it to; `scratch` may carry the work buffer as a third entry."""
    sub = _jpeg_split_bytes(split)
    pk, d = _jpeg_upload(files, device, sub, auto=isinstance(split, str))
    device = d["data"].device
    T, H, W = pk.frames, pk.height, pk.width
    coef_bytes, scratch_bytes = jpeg_decode_sizes(T, H, W, pk.components, pk.hs, pk.vs)
    coef, planes, work = (tuple(scratch) + (None,))[:3] if scratch is not None else (None, None, None)
    coef = _jpeg_coef_out(pk, device, coef)
    if planes is None:
        planes = torch.empty(scratch_bytes, dtype=torch.uint8, device=device)
    assert planes.is_cuda and planes.dtype == torch.uint8 and planes.numel() >= scratch_bytes and planes.is_contiguous()
    out, stride_t = _frames_out(out, T, H, W, device)
    head = (d["data"].data_ptr(), pk.data.nbytes, d["segs"].data_ptr(), pk.segs.shape[0], d["huff"].data_ptr(), d["sel"].data_ptr(),
            d["qt"].data_ptr(), T, H, W, pk.components, pk.hs, pk.vs, coef.data_ptr())
    mid = (out.data_ptr(), stride_t, planes.data_ptr(), planes.numel())
    info = _jpeg_launch("ll_jpeg_decode_u8", head, mid, pk, d, device, sub, rounds, check, return_info, info, work,
                        "return_info, info and a work buffer belong to the split route: pass split=")
    return (out, info) if return_info else out


def resize_taps(n_in: int, n_out: int):
    """Antialiased triangle filter of one axis as host arrays (start int32 [n_out], count int32 [n_out], weights fp32 [n_out, k]): with
    scale = in / out, s = max(scale, 1), c = (o + 0.5) scale the taps are i in [max(int(c - s + 0.5), 0), min(int(c + s + 0.5), in))
    with weights max(0, 1 - |(i + 0.5 - c) / s|), normalised in fp64, then rounded to fp32."""
    import numpy as np
    scale = n_in / n_out
    s = max(scale, 1.0)
    c = (np.arange(n_out, dtype=np.float64) + 0.5) * scale
    lo = np.maximum((c - s + 0.5).astype(np.int64), 0)
    hi = np.minimum((c + s + 0.5).astype(np.int64), n_in)
    k = int((hi - lo).max())
    i = lo[:, None] + np.arange(k)[None, :]
    w = np.maximum(0.0, 1.0 - np.abs((i + 0.5 - c[:, None]) / s)) * (i < hi[:, None])
    w = w / w.sum(axis=1, keepdims=True)
    return lo.astype(np.int32), (hi - lo).astype(np.int32), w.astype(np.float32)


@functools.lru_cache(maxsize=16)
def _resize_tables(n_in: int, n_out: int, dev_index: int):
    start, count, w = resize_taps(n_in, n_out)
    dev = torch.device("cuda", dev_index)
    return torch.from_numpy(start).to(dev), torch.from_numpy(count).to(dev), torch.from_numpy(w).to(dev)


RESIZE_FITS = ("cover", "stretch")


def cover_window(Hs: int, Ws: int, Hd: int, Wd: int):
    """(y0, x0, Hc, Wc): the centred integer crop window of an Hs x Ws frame that has the target's aspect."""
    if Ws * Hd >= Wd * Hs:
        Wc = min(Ws, max(1, int(math.floor(Hs * Wd / Hd + 0.5))))
        return 0, (Ws - Wc) // 2, Hs, Wc
    Hc = min(Hs, max(1, int(math.floor(Ws * Hd / Wd + 0.5))))
    return (Hs - Hc) // 2, 0, Hc, Ws


def resize_u8(frames, size, fit: str = "cover", out=None):
    """uint8 frames [T, Hs, Ws, 3] -> [T, Hd, Wd, 3] (size = (Hd, Wd)) by a separable antialiased triangle filter, what
    F.interpolate(mode="bilinear", antialias=True) computes, rounded once at the end.  fit "cover": a centred crop window of the
    target's aspect (cover_window) is resized; "stretch": the whole frame.  Equal sizes return the input's bytes."""
    if fit not in RESIZE_FITS:
        raise ValueError(f"fit: {fit!r} is not one of {', '.join(RESIZE_FITS)}")
    frames, stride_t = _frames_u8(frames, "frames")
    T, Hs, Ws, _ = frames.shape
    Hd, Wd = int(size[0]), int(size[1])
    assert T >= 1 and Hd >= 1 and Wd >= 1
    y0, x0, Hc, Wc = cover_window(Hs, Ws, Hd, Wd) if fit == "cover" else (0, 0, Hs, Ws)
    out, ost = _frames_out(out, T, Hd, Wd, frames.device)
    idx = _dev_index(frames.device)
    ys, yn, yw = _resize_tables(Hc, Hd, idx)
    xs, xn, xw = _resize_tables(Wc, Wd, idx)
    _call("ll_resize_u8", frames.data_ptr(), stride_t, Hs, Ws, y0, x0, Hc, Wc, out.data_ptr(), ost, Hd, Wd, T, ys.data_ptr(), yn.data_ptr(),
          yw.data_ptr(), yw.shape[1], xs.data_ptr(), xn.data_ptr(), xw.data_ptr(), xw.shape[1])
    return out


# ---- VAE encoder: strided gathers, pixel intake, latent scaling ------------------------------------------------------
def _conv_down(kind: int, x, packed, bias, geo, out):
    cin, cout, kpad, kt, kh = geo
    name = "conv_cl_tdown" if kind else "conv_cl_down"
    assert (kt, kh) == ((3, 1) if kind else (1, 3)), f"{name}: weights are {kt}x{kh}x{kh}"
    hist = 1 if kind else 0
    T, H, W = _conv_in(x, packed, bias, geo, hist, name, "takes [1 + T, H, W, Cin] (the stream's previous frame first)")
    To, Ho, Wo = (T // 2, H, W) if kind else (T, H // 2, W // 2)
    if out is None:
        out = torch.empty(To, Ho, Wo, cout, dtype=bf16, device=x.device)
    _chk(out, "out")
    assert out.shape[:3] == (To, Ho, Wo) and out.shape[3] >= cout, f"{name}: out {tuple(out.shape)} for {(To, Ho, Wo, cout)}"
    _call("ll_" + name, x[hist:].data_ptr(), zero_row(x.device).data_ptr(), packed.data_ptr(), bias.data_ptr(), out.data_ptr(), T, H, W, cin,
          cout, kpad, out.shape[3], tag=name, work=2.0 * To * Ho * Wo * cout * (kt * kh * kh * cin))
    return out


def conv_cl_down(x, packed, bias, geo, out=None):
    """ZeroPad2d((0,1,0,1)) + Conv2d(3, stride 2) per frame (Resample 'downsample2d/3d', vae.py:87-94): x [T, H, W, Cin] ->
    [T, H // 2, W // 2, Cout]; `out` may have rows wider than Cout (columns >= Cout are left alone)."""
    return _conv_down(0, x, packed, bias, geo, out)


def conv_cl_tdown(x, packed, bias, geo, out=None):
    """The (3,1,1) stride-(2,1,1) time_conv of 'downsample3d' (vae.py:95-96, 156-157): x [1 + T, H, W, Cin] -- the stream's previous
    frame, then T (even) new ones -> [T // 2, H, W, Cout]."""
    return _conv_down(1, x, packed, bias, geo, out)


def conv_down_plan(kind: int, T: int, H: int, W: int, cin: int, cout: int) -> str:
    """Kernel instance, tile, grid and k-steps conv_cl_down (kind 0) / conv_cl_tdown (kind 1) launch for this shape (host only)."""
    return _plan("ll_conv_down_plan", kind, T, H, W, cin, cout)


def conv_plan(T: int, H: int, W: int, geo, upsample: bool = False, res: bool = False, rms: bool = False) -> str:
    """ll_conv_plan's text for a pack_conv_weight geometry."""
    cin, cout, kpad, kt, kh = geo
    return _plan("ll_conv_plan", T, H, W, cin, cout, kt, kh, 1 if upsample else 0, 1 if res else 0, 1 if rms else 0)


def _cl_out(out, T: int, H: int, W: int, cpad: int, device):
    if out is None:
        out = torch.empty(T, H, W, cpad, dtype=bf16, device=device)
    _chk(out, "out")
    assert out.shape == (T, H, W, cpad)
    return out


def pixels_to_cl(px, channel_dim: int, cpad: int = 8, out=None):
    """Pixels [3, T, H, W] (channel_dim 0) or [T, 3, H, W] (channel_dim 1), fp32 or bf16, any view whose frames are contiguous ->
    channels-last bf16 [T, H, W, cpad], channels >= 3 zero; fp32 is rounded to bf16 once."""
    if not px.is_cuda:
        raise RuntimeError("pixels: expected a device tensor (longlive_amd has no CPU path)")
    if px.dtype not in (torch.float32, bf16):
        raise RuntimeError(f"pixels: expected float32 or bfloat16, got {px.dtype}")
    assert channel_dim in (0, 1) and px.dim() == 4 and px.shape[channel_dim] == 3, f"pixels: {tuple(px.shape)}, channel_dim {channel_dim}"
    T, H, W = px.shape[1 - channel_dim], px.shape[2], px.shape[3]
    if px.stride(3) != 1 or px.stride(2) != W:
        px = px.contiguous()
    out = _cl_out(out, T, H, W, cpad, px.device)
    _call("ll_pixels_to_cl", px.data_ptr(), 1 if px.dtype == torch.float32 else 0, px.stride(channel_dim), px.stride(1 - channel_dim),
          out.data_ptr(), T, H, W, cpad)
    return out


def pixels_u8_to_cl(frames, cpad: int = 8, out=None):
    """Video frames uint8 [T, H, W, 3] (any view whose frames are contiguous) -> channels-last bf16 [T, H, W, cpad], channels >= 3
    zero, values `(u.float() / 127.5 - 1).to(bfloat16)` bit for bit."""
    frames, stride_t = _frames_u8(frames, "frames")          # uint8: elements are bytes
    T, H, W, _ = frames.shape
    out = _cl_out(out, T, H, W, cpad, frames.device)
    _call("ll_pixels_u8_to_cl", frames.data_ptr(), stride_t, out.data_ptr(), T, H, W, cpad)
    return out


def vae_scale_tchw(mu, mean, inv_std):
    """Channels-last mu [T, h, w, ld] (first z channels) -> fp32 [T, z, h, w] = float(bf16(bf16(mu - mean) * inv_std))."""
    _chk(mu, "mu"); _chk(mean, "mean"); _chk(inv_std, "inv_std")
    T, h, w, ld = mu.shape
    z = mean.numel()
    assert inv_std.numel() == z and ld >= z
    out = torch.empty(T, z, h, w, dtype=torch.float32, device=mu.device)
    _call("ll_vae_scale_tchw", mu.data_ptr(), mean.data_ptr(), inv_std.data_ptr(), out.data_ptr(), T, z, h, w, ld)
    return out


# ---- umT5 text encoder -----------------------------------------------------------------------------------------------
def t5_rmsnorm(x, w, eps: float = 1e-6):
    _chk(x, "x"); _chk(w, "w")
    C = x.shape[-1]
    assert w.numel() == C
    out = torch.empty_like(x)
    _call("ll_t5_rmsnorm", x.data_ptr(), w.data_ptr(), out.data_ptr(), x.numel() // C, C, float(eps))
    return out


def gemm_res_t5norm(x, w, bias, res, norm_w, eps: float = 1e-6, tag: str = "gemm"):
    """(x_new, h) = (res + (x @ w^T + bias), T5LayerNorm(x_new; norm_w)): umT5's `x = x + linear(.)` and the norm that follows it
    (t5.py:119-160) -- on the small-M path one pass over the rows does the K-range sum, bias, residual and norm."""
    M, N, K, out = _linear(x, w, bias)
    _chk(res, "res"); _chk(norm_w, "norm_w")
    assert res.numel() == M * N and norm_w.numel() == N
    h = torch.empty_like(out)
    ws = ksplit_workspace(x.device, M, N, K) if _ksplit_plan(M, N, K) else None
    _call("ll_gemm_bf16_ksplit_t5norm", x.data_ptr(), w.data_ptr(), bias.data_ptr(), out.data_ptr(), M, N, K, K, N, res.data_ptr(),
          norm_w.data_ptr(), float(eps), h.data_ptr(), _ptr(ws), ws.numel() if ws is not None else 0, tag=tag, work=2.0 * M * N * K)
    return out, h


def t5_gated_gelu(h):
    """h [M, 2F] = [gate | fc1] -> bf16(fc1 * GELU_py(gate)) [M, F]."""
    _chk(h, "h")
    M, F2 = h.numel() // h.shape[-1], h.shape[-1]
    assert F2 % 16 == 0
    out = torch.empty(*h.shape[:-1], F2 // 2, dtype=bf16, device=h.device)
    _call("ll_t5_gated_gelu", h.data_ptr(), out.data_ptr(), M, F2 // 2)
    return out


def gather_rows(table, ids):
    """table [V, C] bf16, ids int64 [n] on the device with 0 <= id < V (checked by the caller on the host copy)."""
    _chk(table, "table"); _chk(ids, "ids", torch.int64)
    V, C = table.shape
    out = torch.empty(ids.numel(), C, dtype=bf16, device=table.device)
    _call("ll_gather_rows", table.data_ptr(), ids.data_ptr(), out.data_ptr(), ids.numel(), C, V)
    return out


def t5_attention(qk, vt, bias_tab, num_heads: int, seq_len: int):
    """qk [L, 2*H*64] = [q | k] rows; vt [H*64, L]; bias_tab [H, 2L-1] -> [L, H*64]."""
    _chk(qk, "qk"); _chk(vt, "vt"); _chk(bias_tab, "bias_tab")
    L, two_c = qk.shape
    C = num_heads * 64
    assert two_c == 2 * C and vt.shape == (C, L) and bias_tab.shape == (num_heads, 2 * L - 1)
    assert 1 <= seq_len <= L
    out = torch.empty(L, C, dtype=bf16, device=qk.device)
    _call("ll_t5_attention", qk.data_ptr(), qk[:, C:].data_ptr(), vt.data_ptr(), bias_tab.data_ptr(), out.data_ptr(), L, num_heads, two_c, C,
          int(seq_len))
    return out


# ---- quantisation formats of the block linears: what a format is, stated once (include/longlive_hip.h ll_quantize_*) --------------
fp8 = torch.float8_e4m3fn
u8 = torch.uint8


@dataclass(frozen=True)
class QFormat:
    """A row [.., K] of bf16 as codes + scales.  Codes are `bits` wide, packed along K into `code` elements [.., K * bits / 8];
    scales are E8M0 bytes [rows, K / 32] (block) or one float32 per row.  K must be a multiple of `granule`; `label` is set where
    the wrappers refuse another K themselves (the packed formats: a wrong K would size the code tensor wrongly)."""
    name: str              # suffix of the producers' and GEMMs' C entry points
    code: torch.dtype
    bits: int
    block: bool
    granule: int
    quantizer: str         # the quantiser's C entry point
    quant_bytes: float     # bytes per element moved by the quantiser / by a producer, as the KernelTimer tags report them
    prod_bytes: float
    label: Optional[str] = None

    def empty(self, shape, device):
        K = shape[-1]
        if self.label:
            assert K % self.granule == 0, f"{self.label} rows need K % {self.granule} == 0, got {K}"
        rows = math.prod(shape) // K
        scales = torch.empty(rows, K // 32, dtype=u8, device=device) if self.block else torch.empty(rows, dtype=torch.float32, device=device)
        return torch.empty(*shape[:-1], K * self.bits // 8, dtype=self.code, device=device), scales

    def pair(self, xm, name: str):
        """(codes, scales, rows, K) of an operand (codes, scales), checked."""
        q, s = xm
        _chk(q, name, self.code); _chk(s, name + " scales", u8 if self.block else torch.float32)
        width = q.shape[-1]
        assert width % (self.granule * self.bits // 8) == 0, q.shape
        K = width * 8 // self.bits
        rows = q.numel() // width
        assert s.numel() == (rows * (K // 32) if self.block else rows), (q.shape, s.shape)
        return q, s, rows, K


Q8 = QFormat("q8", torch.int8, 8, False, 1, "ll_quantize_rows", 3.0, 3.0)
F8 = QFormat("f8", u8, 8, False, 1, "ll_quantize_rows_f8", 3.0, 3.0)
MX = QFormat("mx", fp8, 8, True, 32, "ll_quantize_mx", 3.0, 3.0)
MX6 = QFormat("mx6", u8, 6, True, 256, "ll_quantize_mx6", 2.75, 3.0, "MXFP6")
MX4 = QFormat("mx4", u8, 4, True, 256, "ll_quantize_mx4", 2.53, 2.53, "MXFP4")


def _bind(fn, *fixed):
    """A public name for a shared implementation with its leading arguments (C entry point, formats) fixed."""
    f = functools.partial(fn, *fixed)
    f.__doc__ = fn.__doc__
    return f


def _quantize(fmt: QFormat, x, tag: Optional[str] = None):
    """Quantise a [..., K] bf16 tensor along K -> (codes [..., K packed], scales) in fmt."""
    _chk(x, "x")
    K = x.shape[-1]
    q, s = fmt.empty(tuple(x.shape), x.device)
    _call(fmt.quantizer, x.data_ptr(), q.data_ptr(), s.data_ptr(), x.numel() // K, K, K,
          tag=tag or fmt.quantizer[3:], work=fmt.quant_bytes * x.numel())
    return q, s


def _qgemm(entry: str, afmt: QFormat, wfmt: QFormat, xm, wm, bias, epilogue: int = EPI_BIAS, out=None, res=None, e=None, mod=None,
           gate_idx: int = 0, rows_per_batch: int = 0, frame_len: int = 0, mx_out: bool = False, tag: str = "gemm"):
    """out[M,N] = epilogue(x @ w^T + bias) with gemm()'s epilogues for operands xm = (codes [..., K packed], scales) in afmt and
    wm = (codes [N, K packed], scales) in wfmt.  mx_out (block-scaled formats, GELU only): returns the afmt codes + scales of the
    bf16 result instead of it."""
    xq, sx, M, K = afmt.pair(xm, "xq")
    wq, sw, N, Kw = wfmt.pair(wm, "wq")
    _chk(bias, "bias")
    assert Kw == K and wq.dim() == 2 and bias.numel() == N, (wq.shape, K, bias.shape)
    nmod = _epilogue(epilogue, M, N, res, e, mod, frame_len)
    if mx_out:
        assert afmt.block and epilogue == EPI_BIAS_GELU and out is None
        qo, so = afmt.empty((*xq.shape[:-1], N), xq.device)
    else:
        qo = so = None
        if out is None:
            out = torch.empty(*xq.shape[:-1], N, dtype=bf16, device=xq.device)
        _chk(out, "out")
        assert out.numel() == M * N
    outs = (_ptr(out), _ptr(qo), _ptr(so)) if afmt.block else (out.data_ptr(),)      # only the block-scaled entries can write codes
    _call(entry, xq.data_ptr(), sx.data_ptr(), wq.data_ptr(), sw.data_ptr(), bias.data_ptr(), *outs, M, N, K, N, epilogue, _ptr(res), _ptr(e),
          _ptr(mod), nmod, gate_idx, rows_per_batch, frame_len, tag=tag, work=2.0 * M * N * K)
    return (qo, so) if mx_out else out


def _qgemm_rowwise(entry: str, fmt: QFormat):
    """The per-row-scale GEMMs take codes and scales as separate arguments."""
    def f(xq, sx, wq, sw, bias, epilogue: int = EPI_BIAS, out=None, res=None, e=None, mod=None, gate_idx: int = 0,
          rows_per_batch: int = 0, frame_len: int = 0, tag: str = "gemm"):
        return _qgemm(entry, fmt, fmt, (xq, sx), (wq, sw), bias, epilogue, out, res, e, mod, gate_idx, rows_per_batch, frame_len, tag=tag)
    return f


def _qgemm_qkv(entry: str, afmt: QFormat, wfmt: QFormat, xm, wm, bias, cache_v, write_start: int, roped_offset: int, write_len: int,
               B: int, L: int, tag: str = "gemm_qkv"):
    """gemm_qkv_v_insert on quantised operands: xm = (codes [B*L or B,L, K packed], scales) in afmt, wm = (codes [3C, K packed],
    scales) in wfmt.  Returns [B, L, 3C] with the q and k thirds valid; the V third went into cache_v [B, S, H, D]."""
    xq, sx, M, K = afmt.pair(xm, "xq")
    wq, sw, N, Kw = wfmt.pair(wm, "wq")
    _chk(bias, "bias"); _chk(cache_v, "cache_v")
    assert Kw == K and M == B * L and bias.numel() == N and N % 3 == 0
    S = _v_cache(cache_v, B, N)
    out = torch.empty(B, L, N, dtype=bf16, device=xq.device)
    _call(entry, xq.data_ptr(), sx.data_ptr(), wq.data_ptr(), sw.data_ptr(), bias.data_ptr(), out.data_ptr(), M, N, K, N, cache_v.data_ptr(),
          B, L, S, write_start, roped_offset, write_len, tag=tag, work=2.0 * M * N * K)
    return out


def _gemm_plan(entry: str, M: int, N: int, K: int) -> str:
    """Kernel instance, tile and grid of the GEMM (and its QKV V-insert form) behind a ll_gemm_plan_* entry (host only)."""
    return _plan(entry, M, N, K)


# The public names.  Per format: the quantiser and the three producers, each returning (codes, scales) equal bit for bit to the
# quantiser applied to the bf16 form's output (int8: quantize_rows above, and ln_modulate_tab_q8 shares its C entry point with the
# bf16 form).  Per activation x weight pairing: the GEMM, its QKV V-insert form and its plan string.
quantize_rows_f8, quantize_mx, quantize_mx6, quantize_mx4 = (_bind(_quantize, f) for f in (F8, MX, MX6, MX4))
ln_modulate_q8, ln_modulate_f8, ln_modulate_mx, ln_modulate_mx6, ln_modulate_mx4 = (_bind(_ln_modulate_q, f) for f in (Q8, F8, MX, MX6, MX4))
ln_modulate_tab_q8, ln_modulate_tab_f8, ln_modulate_tab_mx, ln_modulate_tab_mx6, ln_modulate_tab_mx4 = (
    _bind(_ln_modulate_tab_q, f) for f in (Q8, F8, MX, MX6, MX4))
layernorm_affine_q8, layernorm_affine_f8, layernorm_affine_mx, layernorm_affine_mx6, layernorm_affine_mx4 = (
    _bind(_layernorm_affine_q, f) for f in (Q8, F8, MX, MX6, MX4))

gemm_w8a8 = _qgemm_rowwise("ll_gemm_w8a8", Q8)       # int8 codes, int32 accumulation
gemm_f8 = _qgemm_rowwise("ll_gemm_f8", F8)           # e4m3fn codes (uint8), fp32 accumulation
gemm_mx = _bind(_qgemm, "ll_gemm_mx", MX, MX)
gemm_mx6 = _bind(_qgemm, "ll_gemm_mx6", MX6, MX6)
gemm_mx4w6 = _bind(_qgemm, "ll_gemm_mx4w6", MX6, MX4)      # MXFP4 weights over MXFP6 activations
gemm_mx4 = _bind(_qgemm, "ll_gemm_mx4", MX4, MX4)
gemm_w8a8_qkv_v_insert = _bind(_qgemm_qkv, "ll_gemm_w8a8_qkv", Q8, Q8)
gemm_f8_qkv_v_insert = _bind(_qgemm_qkv, "ll_gemm_f8_qkv", F8, F8)
gemm_mx_qkv_v_insert = _bind(_qgemm_qkv, "ll_gemm_mx_qkv", MX, MX)
gemm_mx6_qkv_v_insert = _bind(_qgemm_qkv, "ll_gemm_mx6_qkv", MX6, MX6)
gemm_mx4w6_qkv_v_insert = _bind(_qgemm_qkv, "ll_gemm_mx4w6_qkv", MX6, MX4)
gemm_mx4_qkv_v_insert = _bind(_qgemm_qkv, "ll_gemm_mx4_qkv", MX4, MX4)
gemm_plan_f8, gemm_plan_mx, gemm_plan_mx6, gemm_plan_mx4w6, gemm_plan_mx4 = (
    _bind(_gemm_plan, "ll_gemm_plan_" + n) for n in ("f8", "mx", "mx6", "mx4w6", "mx4"))


# ---- MXFP8 self-attention over a block-scaled shadow of the KV cache (attention_mx.hip) ------------------------------------------
def kv_shadow_mx_alloc(cache_k) -> dict:
    """Zero-filled MX shadow of one layer's cache k (or v) [B, S, H, 128]: K^ codes [B, S32, H, 128] + scales [B, S32, H, 4],
    V^ codes [B, H, S32 / 32, 128, 32] + scales [B, H, S32 / 32, 128] (include/longlive_hip.h ll_kv_shadow_mx).  Zero, not empty: a
    key tile stages two 32-slot blocks, and the second may be one no refresh has derived yet; its keys are masked (P^ = 0), but its
    V^ bytes still enter the MFMA, where a NaN code or scale byte times 0 is NaN (ll_flash_attn_mx's precondition)."""
    _chk(cache_k, "cache_k")
    B, S, H, D = cache_k.shape
    assert D == 128, "the shadow is specialised for head_dim 128"
    S32 = (S + 31) // 32 * 32
    dev = cache_k.device
    return dict(kq=torch.zeros(B, S32, H, D, dtype=u8, device=dev).view(fp8), ks=torch.zeros(B, S32, H, 4, dtype=u8, device=dev),
                vq=torch.zeros(B, H, S32 // 32, D, 32, dtype=u8, device=dev).view(fp8),
                vs=torch.zeros(B, H, S32 // 32, D, dtype=u8, device=dev), S=S)


def _shadow_ptrs(shadow: dict) -> tuple:
    return _ptrs(shadow[k] for k in ("kq", "ks", "vq", "vs"))


def kv_shadow_mx(cache_k, cache_v, shadow: dict, lo: int, hi: int, tag: str = "kv_shadow_mx"):
    """Re-derive the shadow of cache slots [lo, hi) (widened to whole 32-slot blocks) from the bf16 cache.  Replaces nothing in
    the reference: it follows the cache writes of causal_model.py:257-311 in MX attention mode."""
    _chk(cache_k, "cache_k"); _chk(cache_v, "cache_v")
    B, S, H, D = cache_k.shape
    assert cache_v.shape == cache_k.shape and shadow["S"] == S and shadow["kq"].shape[:1] == (B,), (cache_k.shape, shadow["kq"].shape)
    S32 = shadow["kq"].shape[1]
    n = ((int(hi) + 31) // 32 - int(lo) // 32) * 32
    _call("ll_kv_shadow_mx", cache_k.data_ptr(), cache_v.data_ptr(), *_shadow_ptrs(shadow), B, S, S32, H, D, int(lo), int(hi),
          tag=tag, work=2.0 * B * n * H * D * (2 + 1))         # bytes: k and v read (bf16), codes written


def flash_attn_mx(q, shadow: dict, segments, out=None, scale: Optional[float] = None, tag: Optional[str] = None,
                  out_fmt: Optional[QFormat] = None):
    """flash_attn over the MX shadow of the cache: q [B,Lq,H,128] bf16 (quantised per row in the kernel), keys = up to two slot
    ranges [(start, end), ...].  Returns [B,Lq,H,128] bf16, or with out_fmt (MX, MX6, MX4) the (codes, scales) of those rows: the
    bytes quantize_<fmt>(flash_attn_mx(...)) gives, from the kernel's epilogue (two launches for a packed format over an odd H)."""
    B, Lq, H, D = _attn_q(q)
    S, S32 = shadow["S"], shadow["kq"].shape[1]
    assert shadow["kq"].shape == (B, S32, H, D) and shadow["vq"].shape == (B, H, S32 // 32, D, 32), (q.shape, shadow["kq"].shape)
    s0, e0, s1, e1 = _segs2(segments, S)
    scale = _attn_scale(scale, D)
    tag = tag or "flash_attn_mx"
    work = _attn_flops(B, H, Lq, (e0 - s0) + (e1 - s1), D)
    if out_fmt is not None:
        if _qfmt_id(out_fmt) != 1 and H % 2:
            return _quantize(out_fmt, flash_attn_mx(q, shadow, segments, scale=scale, tag=tag).view(B, Lq, H * D))
        codes, scales = out_fmt.empty((B, Lq, H * D), q.device)
        _call("ll_flash_attn_mx_q", _qfmt_id(out_fmt), q.data_ptr(), *_shadow_ptrs(shadow), codes.data_ptr(), scales.data_ptr(), B, Lq, H, D,
              H * D, codes.shape[-1], scales.shape[-1], S, S32, s0, e0 - s0, s1, e1 - s1, scale, tag=tag, work=work)
        return codes, scales
    out = torch.empty_like(q) if out is None else _chk(out, "out")
    assert out.shape == q.shape
    _call("ll_flash_attn_mx", q.data_ptr(), *_shadow_ptrs(shadow), out.data_ptr(), B, Lq, H, D, H * D, H * D, S, S32, s0, e0 - s0, s1, e1 - s1,
          scale, tag=tag, work=work)
    return out


def flash_attn_mx_plan(Lq: int, H: int, B: int, segments) -> str:
    """Kernel, tile and grid of a flash_attn_mx call (host only)."""
    s0, e0, s1, e1 = _segs2(segments, 1 << 30)
    return _plan("ll_flash_attn_mx_plan", Lq, H, B, s0, e0 - s0, s1, e1 - s1)
