"""CausalWanModel on MI355X: the 30-block causal video DiT forward with KV cache, run entirely through
liblonglive_hip.so (hand-written gfx950 kernels).  Host-side mirror of
wan/modules/causal_model.py::CausalWanModel._forward_inference (:907-1068).

The module tree exists only to carry parameters under the reference's state-dict names
(`blocks.{i}.self_attn.q.weight`, `blocks.{i}.ffn.0.weight`, `head.head.weight`, ... causal_model.py:90-95,
395-411,491-495,599-619) so that reference checkpoints load with `load_state_dict`; no nn.Module.forward of a
child is ever called.
"""
from __future__ import annotations

import math
from typing import Callable, Dict, List, NamedTuple, Optional, Tuple

import torch
import torch.nn as nn

from . import ops
from .kv_cache import KVPlan, plan_update, shadow_refresh_ranges
from .synth import WanConfig

bf16 = torch.bfloat16


class _Lin(nn.Module):
    def __init__(self, out_f: int, in_f: int, device, dtype):
        super().__init__()
        self.weight = nn.Parameter(torch.zeros(out_f, in_f, device=device, dtype=dtype), requires_grad=False)
        self.bias = nn.Parameter(torch.zeros(out_f, device=device, dtype=dtype), requires_grad=False)


class _Norm(nn.Module):
    def __init__(self, dim: int, device, dtype, bias: bool = False):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(dim, device=device, dtype=dtype), requires_grad=False)
        if bias:
            self.bias = nn.Parameter(torch.zeros(dim, device=device, dtype=dtype), requires_grad=False)


class _Attn(nn.Module):
    def __init__(self, dim, device, dtype):
        super().__init__()
        self.q, self.k, self.v, self.o = (_Lin(dim, dim, device, dtype) for _ in range(4))
        self.norm_q, self.norm_k = _Norm(dim, device, dtype), _Norm(dim, device, dtype)
        # read by the reference pipeline's _set_all_modules_max_attention_size (causal_inference.py:319-329)
        self.max_attention_size = 32760


class _Block(nn.Module):
    def __init__(self, cfg: WanConfig, device, dtype):
        super().__init__()
        d = cfg.dim
        self.self_attn = _Attn(d, device, dtype)
        self.cross_attn = _Attn(d, device, dtype)
        del self.cross_attn.max_attention_size
        self.norm3 = _Norm(d, device, dtype, bias=True)
        self.ffn = nn.ModuleList([_Lin(cfg.ffn_dim, d, device, dtype), nn.Identity(), _Lin(d, cfg.ffn_dim, device, dtype)])
        self.modulation = nn.Parameter(torch.zeros(1, 6, d, device=device, dtype=dtype), requires_grad=False)


class _Head(nn.Module):
    def __init__(self, cfg: WanConfig, device, dtype):
        super().__init__()
        self.head = _Lin(math.prod(cfg.patch_size) * cfg.out_dim, cfg.dim, device, dtype)
        self.modulation = nn.Parameter(torch.zeros(1, 2, cfg.dim, device=device, dtype=dtype), requires_grad=False)


class _Conv(nn.Module):
    def __init__(self, cfg: WanConfig, device, dtype):
        super().__init__()
        self.weight = nn.Parameter(torch.zeros(cfg.dim, cfg.in_dim, *cfg.patch_size, device=device, dtype=dtype),
                                   requires_grad=False)
        self.bias = nn.Parameter(torch.zeros(cfg.dim, device=device, dtype=dtype), requires_grad=False)


class _QuantMode(NamedTuple):
    """What one mode of the block linears launches.  Every entry is looked up on `ops` when it is called."""
    quantize_w: Optional[Callable]     # weight [N, K] -> (codes, scales); None: bf16 weights as they are
    quantize_x: Optional[Callable]     # an activation no fused producer emitted
    ln_modulate: Callable              # the three producers, emitting what the GEMMs read
    ln_modulate_tab: Callable
    layernorm_affine: Callable
    gemm: Callable                     # (x, w, bias, epilogue, **kw), x and w as the quantisers / producers return them
    gemm_qkv: Callable                 # (x, w, bias, cache_v, write_start, roped_offset, write_len, B, L)
    mx_out: bool                       # FFN1's GELU epilogue writes the codes + scales FFN2 reads, never the bf16 hidden
    granule: int                       # dim and ffn_dim must be multiples of it
    afmt: Optional[ops.QFormat] = None  # the activations' block-scaled format (ops.MX, MX6, MX4: what the attention kernels can emit per
                                       # head); None for bf16 and for per-row scales, which span all heads of a row


def _op(name: str) -> Callable:
    return lambda *a, **kw: getattr(ops, name)(*a, **kw)


def _quant_mode(wq: str, xq: str, act: str, gemm: str, mx_out: bool, granule: int) -> _QuantMode:
    """The regular naming: weights by ops.<wq>, activations by ops.<xq> or the ops.*_<act> producers, ops.gemm_<gemm>[_qkv_v_insert]."""
    return _QuantMode(_op(wq), _op(xq), _op("ln_modulate_" + act), _op("ln_modulate_tab_" + act), _op("layernorm_affine_" + act),
                      _op("gemm_" + gemm), _op(f"gemm_{gemm}_qkv_v_insert"), mx_out, granule, getattr(ops, act.upper()) if act.startswith("mx") else None)


def _rowwise(gemm: str) -> Callable:       # the per-row-scale GEMMs take codes and scales as separate arguments
    return lambda x, w, *a, **kw: getattr(ops, gemm)(*x, *w, *a, **kw)


# None: bf16.  "int8": W8A8 (per-token activation scales, per-output-channel weight scales, int32 accumulation).  "mxfp8": e4m3 codes
# with per-32 E8M0 block scales on the scaled MFMA.  "fp8_rowwise": int8's scales with e4m3 codes.  "mxfp6": mxfp8's block scales with
# E2M3 codes packed 6 bits each.  "mxfp4_a6": mxfp6's activations with E2M1 weights packed 4 bits each (W4A6).  "mxfp4_a4": E2M1
# weights and activations.  The packed formats need whole 256-k super-blocks.
_QUANT_MODES = {
    None: _QuantMode(None, None, _op("ln_modulate"), _op("ln_modulate_tab"), _op("layernorm_affine"), _op("gemm"),
                     lambda x, w, b, cache_v, ws, ro, wl, B, L: ops.gemm_qkv_v_insert(x, w, b, cache_v, ws, ro, wl), False, 1),
    "int8": _quant_mode("quantize_rows", "quantize_rows", "q8", "w8a8", False, 128)._replace(gemm=_rowwise("gemm_w8a8")),
    "mxfp8": _quant_mode("quantize_mx", "quantize_mx", "mx", "mx", True, 128),
    "fp8_rowwise": _quant_mode("quantize_rows_f8", "quantize_rows_f8", "f8", "f8", False, 128)._replace(gemm=_rowwise("gemm_f8")),
    "mxfp6": _quant_mode("quantize_mx6", "quantize_mx6", "mx6", "mx6", True, 256),
    "mxfp4_a6": _quant_mode("quantize_mx4", "quantize_mx6", "mx6", "mx4w6", True, 256),
    "mxfp4_a4": _quant_mode("quantize_mx4", "quantize_mx4", "mx4", "mx4", True, 256),
}


_MX_SHADOW = "_ll_mx"      # a layer's cache dict in MX attention mode: the block-scaled shadow of k / v (ops.kv_shadow_mx_alloc)


def mx_shadow_key(k: torch.Tensor, v: torch.Tensor) -> tuple:
    """What the MX shadow of a layer's k / v was derived from: data pointers, shape and version counters.  An outside in-place write
    (zero_, copy_) bumps a version, a new tensor changes a pointer or the shape; the model's own writes go through the C ABI and
    change none of them."""
    return (k.data_ptr(), v.data_ptr(), tuple(k.shape), k._version, v._version)


def _idx_versions(cache: dict):
    g, e = cache.get("global_end_index"), cache.get("local_end_index")      # host ints: the value itself is the "version"
    return (g._version if torch.is_tensor(g) else ("int", g), e._version if torch.is_tensor(e) else ("int", e))


def _kv_state(cache: dict) -> Tuple[int, int]:
    """(global_end_index, local_end_index) as python ints.  Accepts the reference's cache dicts (int64[1] device tensors,
    pipeline/causal_inference.py:275-276): they are read back ONCE and shadowed under `_ll_idx`; afterwards the shadow is
    authoritative and the tensors are only written (async fill_) -- unless somebody ELSE writes them: the reference's training
    pipelines reset them in place (`blk["global_end_index"].zero_()`, pipeline/streaming_training.py:290-305).  Every in-place
    write bumps the tensor's version counter, so a version that is not the one left by our own last fill_ means an external
    write, and the tensors are read again (one sync, only then)."""
    st = cache.get("_ll_idx")
    if st is not None and len(st) == 4 and st[2:] != list(_idx_versions(cache)):
        st = None
    if st is None:
        g, e = cache["global_end_index"], cache["local_end_index"]
        st = [int(g.item()) if torch.is_tensor(g) else int(g), int(e.item()) if torch.is_tensor(e) else int(e),
              *_idx_versions(cache)]
        cache["_ll_idx"] = st
    return st[0], st[1]


def _kv_commit(cache: dict, G: int, E: int) -> None:
    for key, val in (("global_end_index", G), ("local_end_index", E)):
        cur = cache.get(key)
        if torch.is_tensor(cur):
            cur.fill_(val)
        else:
            cache[key] = val
    cache["_ll_idx"] = [G, E, *_idx_versions(cache)]


class CausalWanModelHIP(nn.Module):
    """Drop-in for the KV-cache inference branch of CausalWanModel."""

    rope_frames = 1024      # rows of the frame-axis RoPE table (model.py:29-36): the longest timeline, in latent frames

    def __init__(self, cfg: WanConfig, device="cuda", dtype=bf16):
        super().__init__()
        assert dtype == bf16, "the HIP path computes in bf16 (inference.py:134)"
        assert cfg.head_dim == 128, "kernels are specialised for head_dim 128 (Wan2.1-T2V-1.3B: 1536 / 12)"
        assert cfg.patch_size == (1, 2, 2)
        self.cfg = cfg
        d = cfg.dim
        self.patch_embedding = _Conv(cfg, device, dtype)
        self.text_embedding = nn.ModuleList([_Lin(d, cfg.text_dim, device, dtype), nn.Identity(), _Lin(d, d, device, dtype)])
        self.time_embedding = nn.ModuleList([_Lin(d, cfg.freq_dim, device, dtype), nn.Identity(), _Lin(d, d, device, dtype)])
        self.time_projection = nn.ModuleList([nn.Identity(), _Lin(6 * d, d, device, dtype)])
        self.blocks = nn.ModuleList([_Block(cfg, device, dtype) for _ in range(cfg.num_layers)])
        self.head = _Head(cfg, device, dtype)
        # attributes the reference pipelines read / write (causal_inference.py:54,135,310-329;
        # interactive_causal_inference.py:73-84)
        self.local_attn_size = cfg.local_attn_size
        self.sink_size = cfg.sink_size
        self.max_attention_size = 32760 if cfg.local_attn_size == -1 else cfg.local_attn_size * 1560
        for b in self.blocks:
            b.self_attn.max_attention_size = self.max_attention_size
        self.num_frame_per_block = 1
        self.block_mask = None
        # None: bf16 linears (the reference's precision).  "int8": W8A8 for the six per-token linears of every block
        # (BASELINE config 5; per-token activation scales, per-output-channel weight scales, int32 accumulation).  "mxfp8": the same
        # six on the block-scaled e4m3 MFMA (one power-of-two scale per 32 elements of K for activations and weights alike).
        # "fp8_rowwise": int8's per-token / per-output-channel scales with e4m3 codes, on the W8A8 kernels' structure.  "mxfp6": mxfp8's
        # per-32 block scales with E2M3 (FP6) codes packed 6 bits each, on the MFMA's FP4-rate form.  "mxfp4_a6": mxfp6's activations
        # with E2M1 (FP4) weights packed 4 bits each (W4A6).  "mxfp4_a4": those E2M1 weights over E2M1 activations in the same scheme
        # and layout (W4A4).
        self.quant: Optional[str] = None
        # None: bf16 self-attention.  "mxfp8": self-attention on the block-scaled e4m3 MFMA over an MX shadow of each layer's KV cache
        # (kept in the cache dict under _MX_SHADOW, re-derived after every write; orthogonal to `quant`).
        self.attn_quant: Optional[str] = None
        self.use_modulation_table = True      # modulation + e0 once per (layer, frame) instead of once per token row (A/B switch)
        self.fuse_v_insert = True             # the QKV projection's epilogue writes V into the KV cache (A/B switch)
        self.use_modulation_f32 = True        # LN + modulate from the fp32 table (1 + scale, shift: ops.modulation_table_f32) beside the
                                              # bf16 one the gate epilogues read: same bits, fewer instructions per row (A/B switch)
        self.fuse_attn_quant = False          # block-scaled modes: self- and cross-attention write the codes + scales their output
                                              # projections read (ops.flash_attn(..., out_fmt=)), no quantiser launch between: same bits.
                                              # Off by default: faster end to end in mxfp8 and mxfp4_a6, not in mxfp6 and mxfp4_a4
                                              # (profiles/attn_qout_fps.md)
        self.fuse_cross_qnorm = True          # cross-attention q: RMSNorm statistics from the projection's epilogue, applied in the attention
                                              # kernel's Q prologue (no RMSNorm launch) where both generated kernels cover the call (A/B switch)
        self._packed = None
        self._rope_f = None
        self._rope_hw: Dict[Tuple[int, int], torch.Tensor] = {}
        self._ctx_cache = None
        self._time_memo: Dict[tuple, tuple] = {}      # (t value, B, F, HIP stream) -> (parameter key, packed key, e, e0, etab): see forward_frames(t_uniform=)
        # nn.Module's recursive load (e.g. WanDiffusionWrapper.load_state_dict, as inference.py:87/94 loads) never calls a
        # child's load_state_dict override, only its _load_from_state_dict -- which runs these hooks.
        self._register_load_state_dict_pre_hook(self._invalidate_derived)

    # ---- parameter packing -------------------------------------------------------------------------------------
    def _apply(self, fn, *a, **k):
        self._packed = None
        self._rope_f = None
        self._rope_hw = {}
        self._ctx_cache = None
        self._time_memo = {}
        return super()._apply(fn, *a, **k)

    def _invalidate_derived(self, *unused_hook_args):
        """Drop everything derived from the parameters: the fused QKV / int8 copies and the memoised text embedding."""
        self._packed = None
        self._ctx_cache = None
        self._time_memo = {}

    def invalidate_packed(self):
        """Call after writing parameters through `.data` (which bypasses the version counter that `_pack` checks);
        load_state_dict (direct or through a parent), `.to()` and in-place ops under no_grad are detected automatically."""
        self._invalidate_derived()

    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        self._invalidate_derived()
        return super().load_state_dict(state_dict, strict=strict, **kw)

    @staticmethod
    def _prepare_blockwise_causal_attn_mask(*args, **kwargs):
        """The reference builds a flex-attention mask before recaching (interactive_causal_inference.py:73-84), but
        the KV-cache branch of self-attention never reads it (causal_model.py:205-360).  Kept for call compatibility."""
        return None

    def _param_key(self):
        """(address, version) of every parameter a packed copy is made from: an in-place update (EMA swap, LoRA re-fold,
        `param.copy_`) bumps `_version`, a re-assignment changes the address."""
        key = []
        for blk in self.blocks:
            sa = blk.self_attn
            ts = [sa.q.weight, sa.k.weight, sa.v.weight, sa.q.bias, sa.k.bias, sa.v.bias, blk.modulation]
            if self.quant is not None:
                ts += [sa.o.weight, blk.cross_attn.q.weight, blk.cross_attn.o.weight, blk.ffn[0].weight, blk.ffn[2].weight]
            key.extend((t.data_ptr(), t._version) for t in ts)
        return tuple(key)

    def _pack(self):
        if self._packed is not None:
            if self._packed_key == self._param_key():
                return self._packed
            self._invalidate_derived()
        P = []
        for blk in self.blocks:
            sa, ca = blk.self_attn, blk.cross_attn
            d = dict(
                wqkv=torch.cat([sa.q.weight, sa.k.weight, sa.v.weight], 0).contiguous(),
                bqkv=torch.cat([sa.q.bias, sa.k.bias, sa.v.bias], 0).contiguous(),
                mod=blk.modulation.detach().reshape(6, -1).contiguous(),
            )
            quantize = _QUANT_MODES[self.quant].quantize_w
            if quantize is not None:
                for name, w in (("qkv", d["wqkv"]), ("o", sa.o.weight), ("cq", ca.q.weight), ("co", ca.o.weight),
                                ("f1", blk.ffn[0].weight), ("f2", blk.ffn[2].weight)):
                    d["q_" + name], d["s_" + name] = quantize(w.detach().contiguous())
            P.append(d)
        self._packed = P
        self._mods = torch.stack([d["mod"] for d in P], 0).contiguous()      # [NL, 6, C] for ops.modulation_table
        self._packed_key = self._param_key()
        return P

    def set_quant(self, mode: Optional[str]):
        """A key of _QUANT_MODES: None (bf16), "int8", "mxfp8", "fp8_rowwise", "mxfp6", "mxfp4_a6" or "mxfp4_a4".  Weights are
        (re)quantised lazily at the next forward."""
        if mode not in _QUANT_MODES:
            raise ValueError(f"unknown quantisation mode {mode!r}")
        granule = _QUANT_MODES[mode].granule
        if granule >= 128 and (self.cfg.dim % 128 or self.cfg.ffn_dim % 128):
            raise ValueError(f"{mode} linears need dim and ffn_dim to be multiples of 128")
        if granule == 256 and (self.cfg.dim % 256 or self.cfg.ffn_dim % 256):
            raise ValueError(f"{mode} linears need dim and ffn_dim to be multiples of 256 (packed 256-k super-blocks)")
        self.quant = mode
        self._packed = None
        return self

    def set_attn_quant(self, mode: Optional[str]):
        """None (bf16 self-attention) or "mxfp8" (MXFP8 self-attention over a block-scaled shadow of the KV cache).
        Independent of set_quant; cross-attention stays bf16 in every mode."""
        if mode not in (None, "mxfp8"):
            raise ValueError(f"unknown attention quantisation mode {mode!r}")
        if mode is not None and self.cfg.head_dim != 128:
            raise ValueError("MX attention needs head_dim 128")
        self.attn_quant = mode
        return self

    @staticmethod
    def _mx_shadow(kvc: dict):
        """(shadow, stale) of a layer's cache: allocated at the first MX forward; stale when it is new or k / v changed outside the
        model since the last refresh (version counter, data pointer or shape: our own writes go through the C ABI and bump nothing)."""
        k = kvc["k"]
        sh = kvc.get(_MX_SHADOW)
        if sh is None or sh["kq"].shape[0] != k.shape[0] or sh["S"] != k.shape[1] or sh["kq"].shape[2] != k.shape[2]:
            sh = ops.kv_shadow_mx_alloc(k)
            sh["key"] = None
            kvc[_MX_SHADOW] = sh
        return sh, sh["key"] != mx_shadow_key(k, kvc["v"])

    def _lin(self, x, pk, key, w, b, epilogue=0, **kw):
        """One block linear in the current mode (same fused epilogues in every mode).  `x` is a bf16 tensor, quantised here per the
        mode, or the (codes, scales) pair a fused producer of the mode already emitted."""
        m = _QUANT_MODES[self.quant]
        if m.quantize_w is not None:
            w = (pk["q_" + key], pk["s_" + key])
            if not isinstance(x, tuple):
                x = m.quantize_x(x)
        return m.gemm(x, w, b, epilogue, tag="gemm_" + key, **kw)

    def _rope_tables(self, hp: int, wp: int, device):
        """fp32 (cos, sin) tables from the reference's fp64 angles (model.py:29-36; causal_model.py:622-629):
        rope_f [1024, nf, 2] for the frame axis, rope_hw [hp*wp, 2*c3, 2] = (h angles | w angles) per spatial token."""
        d = self.cfg.head_dim
        half = d // 2
        c3 = half // 3
        nf = half - 2 * c3

        def angles(n, dim):
            return torch.outer(torch.arange(n, dtype=torch.float64),
                               1.0 / torch.pow(10000.0, torch.arange(0, dim, 2, dtype=torch.float64).div(dim)))

        if self._rope_f is None:
            a = angles(self.rope_frames, d - 4 * (d // 6))
            assert a.shape[1] == nf
            self._rope_f = torch.stack([a.cos(), a.sin()], -1).float().contiguous().to(device)
        key = (hp, wp)
        if key not in self._rope_hw:
            ah = angles(1024, 2 * (d // 6))[:hp]          # [hp, c3]
            aw = angles(1024, 2 * (d // 6))[:wp]          # [wp, c3]
            a = torch.cat([ah.view(hp, 1, c3).expand(hp, wp, c3), aw.view(1, wp, c3).expand(hp, wp, c3)], -1)
            a = a.reshape(hp * wp, 2 * c3)
            self._rope_hw[key] = torch.stack([a.cos(), a.sin()], -1).float().contiguous().to(device)
        return self._rope_f, self._rope_hw[key]

    # ---- embeddings ---------------------------------------------------------------------------------------------
    def time_embed(self, t: torch.Tensor):
        """t [B,F] -> e [B*F, C], e0 [B,F,6,C]   (causal_model.py:976-979)."""
        c = self.cfg
        tf = t.reshape(-1).to(torch.float32).contiguous()
        emb = ops.sinusoid(tf, c.freq_dim)
        h = ops.linear_small(emb, self.time_embedding[0].weight, self.time_embedding[0].bias, act_out=1)
        e = ops.linear_small(h, self.time_embedding[2].weight, self.time_embedding[2].bias)
        e0 = ops.linear_small(e, self.time_projection[1].weight, self.time_projection[1].bias, act_in=1)
        return e, e0.view(*t.shape, 6, c.dim)

    def _time_param_key(self):
        ps = (self.time_embedding[0].weight, self.time_embedding[0].bias, self.time_embedding[2].weight, self.time_embedding[2].bias,
              self.time_projection[1].weight, self.time_projection[1].bias)
        return tuple((p.data_ptr(), p._version) for p in ps)

    def text_embed(self, context: torch.Tensor):
        """[B, text_len, text_dim] -> [B, text_len, C]   (causal_model.py:984-989).  The reference recomputes this
        every forward; its only consumer is the cross-attention K/V projection, which is cached per prompt
        (model.py:174-183), so it is evaluated lazily and memoised on the prompt tensor."""
        key = (context.data_ptr(), (context._version, torch.cuda.current_stream(context.device).cuda_stream if context.is_cuda else 0))
        if self._ctx_cache is not None and self._ctx_cache[:2] == key:      # (same prompt tensor AND same HIP stream: the memo was computed there)
            return self._ctx_cache[2]
        c = self.cfg
        ctx = context.to(bf16)
        if ctx.shape[1] < c.text_len:
            ctx = torch.cat([ctx, ctx.new_zeros(ctx.shape[0], c.text_len - ctx.shape[1], ctx.shape[2])], 1)
        ctx = ctx.contiguous()
        h = ops.gemm(ctx, self.text_embedding[0].weight, self.text_embedding[0].bias, ops.EPI_BIAS_GELU)
        out = ops.gemm(h, self.text_embedding[2].weight, self.text_embedding[2].bias)
        self._ctx_cache = (key[0], key[1], out, context)   # holding `context` keeps its address from being reused
        return out

    # ---- one block ---------------------------------------------------------------------------------------------
    @torch.no_grad()
    def block_forward(self, i: int, xs: torch.Tensor, e0: torch.Tensor, ctx: Optional[torch.Tensor], kvc: dict,
                      cac: dict, F: int, grid_hw: Tuple[int, int], current_start: int,
                      sink_recache_after_switch: bool = False, q_buf: Optional[torch.Tensor] = None,
                      kv_insert_only: bool = False, pk: Optional[dict] = None, premod: bool = False,
                      cache_done_event=None, co_running: bool = False, tab32: Optional[torch.Tensor] = None) -> KVPlan:
        """CausalWanAttentionBlock.forward (causal_model.py:413-477) for block `i`: updates the residual stream
        xs [B, L, C] IN PLACE (L = F * hp * wp tokens, grid_hw = (hp, wp) tokens per frame) and this layer's KV / cross
        caches, returns the layer's KV plan (the caller commits the end indices after all layers,
        causal_model.py:1061-1062).  e0 [B, F, 6, C]; ctx = embedded text [B, 512, C] (only read when the cross cache is
        not initialised).  kv_insert_only: stop after the K/V insert.  premod: `e0` is this layer's slice of
        ops.modulation_table (modulation already added), as forward_frames passes it.  cache_done_event: recorded on the
        current stream right after this layer's LAST access to its KV cache (the self-attention launch, or the insert when
        kv_insert_only) -- a forward on another stream may touch the layer's cache from then on.  tab32: this layer's slice
        [B, F, 6, C] of ops.modulation_table_f32 (chunks 1 and 4 hold 1 + scale): the two LN + modulate launches read it
        instead of e0."""
        c = self.cfg
        B, L, C = xs.shape
        Hh, D = c.num_heads, c.head_dim
        hp, wp = grid_hw
        fs = hp * wp
        if L != F * fs:
            raise ValueError(f"block_forward: {L} tokens are not {F} frames of {hp}x{wp}")
        rope_f, rope_hw = self._rope_tables(hp, wp, xs.device)
        if q_buf is None:
            q_buf = torch.empty(B, L, Hh, D, dtype=bf16, device=xs.device)
        blk = self.blocks[i]
        if pk is None:
            pk = self._pack()[i]
        mod = None if premod else pk["mod"]
        sa, ca = blk.self_attn, blk.cross_attn
        # --- self attention (causal_model.py:444-456) ---
        m = _QUANT_MODES[self.quant]
        G, E = _kv_state(kvc)
        S = kvc["k"].shape[1]
        plan = plan_update(current_start, L, G, E, S, self.sink_size * fs, self.local_attn_size,
                           sa.max_attention_size, sink_recache_after_switch)
        amx = self.attn_quant == "mxfp8"
        ofmt = m.afmt if self.fuse_attn_quant else None
        if amx:
            shadow, stale = self._mx_shadow(kvc)
        else:
            kvc.pop(_MX_SHADOW, None)      # bf16 writes from here on are not mirrored: a later MX forward starts from a new shadow
        if plan.roll is not None:          # before the projection: its epilogue writes V into the rolled window
            ops.kv_roll(kvc["k"], kvc["v"], *plan.roll)
        h1 = m.ln_modulate_tab(xs, tab32, 0, 1, F, c.eps) if tab32 is not None else m.ln_modulate(xs, e0, mod, 0, 1, F, c.eps)
        if self.fuse_v_insert:             # V third of the projection goes straight into its cache slots (GEMM epilogue)
            qkv = m.gemm_qkv(h1, pk["wqkv"] if m.quantize_w is None else (pk["q_qkv"], pk["s_qkv"]), pk["bqkv"], kvc["v"],
                             plan.write_start, plan.roped_offset, plan.write_len, B, L)
            v_dst = None
        else:
            qkv = self._lin(h1, pk, "qkv", pk["wqkv"], pk["bqkv"])
            v_dst = kvc["v"]
        ops.qk_norm_rope_kv_store(qkv, sa.norm_q.weight, sa.norm_k.weight, rope_f, rope_hw, q_buf.view(B, L, C),
                                  kvc["k"], v_dst, D, fs, current_start // fs, plan.write_start,
                                  plan.roped_offset, plan.write_len, c.eps)
        if amx:                            # the shadow follows the roll and the insert (or all of the cache after an outside change)
            for lo, hi in shadow_refresh_ranges(plan, stale, S):
                ops.kv_shadow_mx(kvc["k"], kvc["v"], shadow, lo, hi, tag="kv_shadow_mx_co" if co_running else "kv_shadow_mx")
            shadow["key"] = mx_shadow_key(kvc["k"], kvc["v"])
        if kv_insert_only:
            if cache_done_event is not None:
                cache_done_event.record(torch.cuda.current_stream())
            return plan
        # (a forward that runs beside another one on a second stream -- the pipelines' context-pass overlap -- times its launches
        #  under another tag: bench.py's roofline describes the kernel running alone on the device)
        if amx:
            att = ops.flash_attn_mx(q_buf, shadow, plan.segments, tag="flash_attn_self_mx_co" if co_running else "flash_attn_self_mx",
                                    out_fmt=ofmt)
        else:
            att = ops.flash_attn(q_buf, kvc["k"], kvc["v"], plan.segments, tag="flash_attn_self_co" if co_running else "flash_attn_self",
                                 out_fmt=ofmt)
        if cache_done_event is not None:
            cache_done_event.record(torch.cuda.current_stream())
        self._lin(att if ofmt is not None else att.view(B, L, C), pk, "o", sa.o.weight, sa.o.bias, ops.EPI_BIAS_GATE_RES, out=xs, res=xs, e=e0,
                  mod=mod, gate_idx=2, rows_per_batch=L, frame_len=fs)
        # --- cross attention (causal_model.py:460; model.py:159-194) ---
        xn = m.layernorm_affine(xs, blk.norm3.weight, blk.norm3.bias, c.eps)
        fuse_qn = (self.fuse_cross_qnorm and self.quant is None and ops.gemm_ssq_planes(B * L, C, C) == Hh and ops.flash_attn_qnorm_ok(Hh, c.text_len))
        if fuse_qn:
            qraw, ssq = ops.gemm_ssq(xn, ca.q.weight, ca.q.bias, tag="gemm_cq_ssq")
        else:
            qc = ops.rmsnorm(self._lin(xn, pk, "cq", ca.q.weight, ca.q.bias), ca.norm_q.weight, c.eps)
        if not cac["is_init"]:
            kc = ops.gemm(ctx, ca.k.weight, ca.k.bias)
            if cac["k"].shape != (B, c.text_len, Hh, D) or not cac["k"].is_contiguous():
                cac["k"] = torch.empty(B, c.text_len, Hh, D, dtype=bf16, device=xs.device)
                cac["v"] = torch.empty(B, c.text_len, Hh, D, dtype=bf16, device=xs.device)
            ops.rmsnorm(kc, ca.norm_k.weight, c.eps, out=cac["k"].view(B, c.text_len, C))
            ops.gemm(ctx, ca.v.weight, ca.v.bias, out=cac["v"].view(B, c.text_len, C))
            cac["is_init"] = True
        if fuse_qn:
            atc = ops.flash_attn_qnorm(qraw.view(B, L, Hh, D), ssq, ca.norm_q.weight, c.eps, cac["k"], cac["v"], c.text_len, tag="flash_attn_cross_qn")
        else:
            atc = ops.flash_attn(qc.view(B, L, Hh, D), cac["k"], cac["v"], [(0, c.text_len)], tag="flash_attn_cross", out_fmt=ofmt)
        self._lin(atc if isinstance(atc, tuple) else atc.view(B, L, C), pk, "co", ca.o.weight, ca.o.bias, ops.EPI_BIAS_RES, out=xs, res=xs)
        # --- FFN (causal_model.py:462-468) ---
        h2 = m.ln_modulate_tab(xs, tab32, 3, 4, F, c.eps) if tab32 is not None else m.ln_modulate(xs, e0, mod, 3, 4, F, c.eps)
        ff = self._lin(h2, pk, "f1", blk.ffn[0].weight, blk.ffn[0].bias, ops.EPI_BIAS_GELU,
                       **(dict(mx_out=True) if m.mx_out else {}))
        self._lin(ff, pk, "f2", blk.ffn[2].weight, blk.ffn[2].bias, ops.EPI_BIAS_GATE_RES, out=xs, res=xs, e=e0,
                  mod=mod, gate_idx=5, rows_per_batch=L, frame_len=fs)
        return plan

    # ---- forward -----------------------------------------------------------------------------------------------
    @torch.no_grad()
    def forward_frames(self, x: torch.Tensor, t: torch.Tensor, context: torch.Tensor, kv_cache: List[dict],
                       crossattn_cache: List[dict], current_start: int = 0,
                       sink_recache_after_switch: bool = False, sigma: Optional[torch.Tensor] = None,
                       kv_only: bool = False, layer_wait=None, layer_record=None, t_uniform: Optional[float] = None):
        """x [B,F,Cin,H,W] (the wrapper's layout); t [B,F]; context [B,text_len,text_dim].
        t_uniform: the caller KNOWS that every entry of t equals this host value (the pipelines build their timestep tensors from
        the four denoising steps + the context step): the time embedding, its projection and the modulation table of all layers
        depend on nothing else, so they are computed once per (value, B, F, HIP stream) and reused while the parameters they
        were made from are unchanged -- six launches per forward less, same bits.
        Returns the head output [B, L, 4*Cout] (pre-unpatchify), or (flow, x0) in [B,F,C,H,W] when `sigma`
        (float32 [B*F]) is given.  kv_only: the caller discards the output and only wants the KV caches updated (the
        clean-context pass and the recache pass, causal_inference.py:192-200, interactive_causal_inference.py:34-106):
        everything after the last layer's K/V insert -- its attention, cross-attention, FFN and the head -- is skipped and
        None is returned; the caches end up bit-identical.
        layer_wait / layer_record: per-layer HIP events for running TWO forwards on two streams one layer apart (the pipelines
        overlap a block's clean-context pass with the next block's first denoising forward): before touching layer i's caches
        this forward waits for layer_wait[i]; right after layer i's last cache access (its self-attention launch) it records
        layer_record[i] on its stream."""
        c = self.cfg
        B, F, Cin, H, W = x.shape
        hp, wp = H // 2, W // 2
        fs = hp * wp
        L = F * fs
        Hh, D, C = c.num_heads, c.head_dim, c.dim
        assert current_start % fs == 0, "current_start must sit on a frame boundary"
        x = x.to(bf16).contiguous()
        pe = self.patch_embedding
        xs = ops.gemm(ops.patchify(x), pe.weight.view(C, -1), pe.bias)                      # [B, L, C]
        need_ctx = any(not cc["is_init"] for cc in crossattn_cache)
        ctx = self.text_embed(context) if need_ctx else None

        q_buf = torch.empty(B, L, Hh, D, dtype=bf16, device=x.device)
        plans: List[KVPlan] = []
        last = len(self.blocks) - 1
        P = self._pack()       # validated against the live parameters once per forward
        premod = self.use_modulation_table
        tab_f32 = premod and self.use_modulation_f32 and x.is_cuda
        memo_key = None
        if t_uniform is not None and x.is_cuda and tuple(t.shape) == (B, F):
            memo_key = (float(t_uniform), B, F, premod, tab_f32, torch.cuda.current_stream(x.device).cuda_stream)
            hit = self._time_memo.get(memo_key)
            if hit is not None and hit[0] == self._time_param_key() and hit[1] is self._packed_key:
                e, e0, etab, etab32 = hit[2:]
            else:
                hit = None
        if memo_key is None or hit is None:
            e, e0 = self.time_embed(t)
            etab = ops.modulation_table(e0, self._mods) if premod else None   # [NL, B, F, 6, C] = modulation + e0, one launch
            etab32 = ops.modulation_table_f32(e0, self._mods, 0b010010) if tab_f32 else None     # fp32, chunks 1 and 4 = 1 + scale
            if memo_key is not None:
                if len(self._time_memo) >= 64:       # (a caller sweeping many timestep values: start over rather than grow)
                    self._time_memo = {}
                self._time_memo[memo_key] = (self._time_param_key(), self._packed_key, e, e0, etab, etab32)
        cur_stream = torch.cuda.current_stream() if (layer_wait is not None or layer_record is not None) else None
        for i in range(len(self.blocks)):
            if layer_wait is not None:
                cur_stream.wait_event(layer_wait[i])
            plans.append(self.block_forward(i, xs, etab[i] if premod else e0, ctx, kv_cache[i], crossattn_cache[i], F, (hp, wp),
                                            current_start, sink_recache_after_switch, q_buf,
                                            kv_insert_only=kv_only and i == last, pk=P[i], premod=premod,
                                            cache_done_event=layer_record[i] if layer_record is not None else None,
                                            co_running=cur_stream is not None, tab32=etab32[i] if tab_f32 else None))
        # commit end indices once all layers have planned with the old values (causal_model.py:1061-1062, 901-904)
        for kvc, plan in zip(kv_cache, plans):
            _kv_commit(kvc, plan.G_new, plan.E_new)
        if kv_only:
            return (None, None) if sigma is not None else None
        # --- head (causal_model.py:497-508,1065) ---
        eh = e.view(B, F, 1, C).expand(B, F, 2, C).contiguous()
        hd = ops.ln_modulate(xs, eh, self.head.modulation.view(2, C), 0, 1, F, c.eps)
        ho = ops.gemm(hd, self.head.head.weight, self.head.head.bias)                       # [B, L, 4*Cout]
        if sigma is None:
            return ho
        return ops.unpatchify_x0(ho, x, sigma)

    def forward(self, x, t=None, context=None, seq_len=None, kv_cache=None, crossattn_cache=None,
                current_start: int = 0, cache_start=None, sink_recache_after_switch: bool = False, **unused):
        """Reference-compatible call (causal_model.py:1230-1238): x [B,C,F,H,W] -> flow [B,C,F,H,W]."""
        if kv_cache is None:
            raise NotImplementedError("only the KV-cache inference branch exists (the reference's training branch "
                                      "is itself a stub: causal_model.py:1102-1103)")
        xf = x.permute(0, 2, 1, 3, 4).contiguous()
        B, F = xf.shape[:2]
        zero = torch.zeros(B * F, dtype=torch.float32, device=xf.device)
        flow, _ = self.forward_frames(xf, t, context, kv_cache, crossattn_cache, current_start,
                                      sink_recache_after_switch, sigma=zero)
        return flow.permute(0, 2, 1, 3, 4)
