"""Host restatement of MXFP8 self-attention over the block-scaled shadow of the KV cache (include/longlive_hip.h ll_kv_shadow_mx /
ll_flash_attn_mx).  The MX rule is tests/mx_ref.py's.

  * Q^: every query row (bf16, after RMSNorm + RoPE) quantised in blocks of 32 channels (= ll_quantize_mx of the row);
  * K^ shadow: every cache slot's K row the same way: codes [B, S32, H, 128], scales [B, S32, H, 4] (S32 = S rounded up to 32);
  * V^ shadow: per (head, channel d, slot block j = slots 32 j .. 32 j + 31) the MX rule over V[32 j + i, head, d], slots >= S read
    as 0; codes [B, H, S32 / 32, 128, 32] with position 16 hh + jj holding slot 32 j + frag(jj, hh), scales [B, H, S32 / 32, 128];
  * scores s = sum_b 2^(eq + ek) sum q^ k^ in fp32; key tiles of 64 slots start at each range's start rounded down to 32 (adjacent
    ranges merged first); slots outside the ranges are masked to -inf;
  * lazy max per query: M = c m_ref moves to a tile's c * max only when that exceeds M by more than THR = 8; O and l are rescaled by
    exp2(M_old - M_new) then;
  * P^ = e4m3fn(RNE(exp2(c s - M))) (unit scale: P <= 2^8 < 448), l = sum P^, O = sum P^ V^, output bf16(O / l).

The kernel and this restatement differ only by the fp32 summation order and v_exp_f32's ulp.
MXAttnRefModel is the oracle's RefModel (optionally with tests/quant_ref.py's quantised block linears) with self-attention on this
scheme."""
import math
from typing import List, Optional, Tuple

import torch
from torch import Tensor

import mx_ref
from oracle import ref_ops as R
from quant_ref import QuantRefModel

FP8 = torch.float8_e4m3fn
KT = 64
THR = 8.0
LOG2E = 1.4426950408889634


def frag_slot(p: int) -> int:
    """Slot (within its 32-block) of code position p of a V^ row: the key order of a score tile's accumulator registers."""
    jj, hh = p & 15, p >> 4
    return (jj & 3) + 8 * (jj >> 2) + 4 * hh


FRAG = torch.tensor([frag_slot(p) for p in range(32)])


def shadow_k(k: Tensor) -> Tuple[Tensor, Tensor]:
    """bf16 cache k [B, S, H, 128] -> (codes [B, S32, H, 128] e4m3fn, scales [B, S32, H, 4] uint8)."""
    B, S, H, D = k.shape
    S32 = (S + 31) // 32 * 32
    kp = torch.zeros(B, S32, H, D, dtype=torch.bfloat16, device=k.device)
    kp[:, :S] = k
    q, s = mx_ref.quantize(kp.reshape(-1, D))
    return q.reshape(B, S32, H, D), s.reshape(B, S32, H, D // 32)


def shadow_v(v: Tensor) -> Tuple[Tensor, Tensor]:
    """bf16 cache v [B, S, H, 128] -> (codes [B, H, S32/32, 128, 32] in fragment order, scales [B, H, S32/32, 128] uint8)."""
    B, S, H, D = v.shape
    S32 = (S + 31) // 32 * 32
    vp = torch.zeros(B, S32, H, D, dtype=torch.bfloat16, device=v.device)
    vp[:, :S] = v
    blocks = vp.reshape(B, S32 // 32, 32, H, D).permute(0, 3, 1, 4, 2)          # [B, H, NB, D, 32 slots]
    blocks = blocks[..., FRAG.to(v.device)].contiguous()                        # fragment order
    q, s = mx_ref.quantize(blocks.reshape(-1, 32))
    return q.reshape(B, H, S32 // 32, D, 32), s.reshape(B, H, S32 // 32, D)


def deq_k(kq: Tensor, ks: Tensor, dtype=torch.float64) -> Tensor:
    """[B, S32, H, 128] dequantised K^ (exact in fp32 and fp64)."""
    e = ks.to(torch.int32) - 127
    return (kq.to(dtype).reshape(*ks.shape, 32) * torch.pow(2.0, e.to(dtype)).unsqueeze(-1)).reshape(kq.shape)


def deq_v(vq: Tensor, vs: Tensor, dtype=torch.float64) -> Tensor:
    """[B, S32, H, 128] dequantised V^ in natural slot order."""
    B, H, NB, D, _ = vq.shape
    x = vq.to(dtype) * torch.pow(2.0, (vs.to(torch.int32) - 127).to(dtype)).unsqueeze(-1)
    nat = torch.empty_like(x)
    nat[..., FRAG.to(vq.device)] = x
    return nat.permute(0, 2, 4, 1, 3).reshape(B, NB * 32, H, D)


def merge_segments(segments, merge: bool = True) -> List[Tuple[int, int]]:
    segs = [(int(a), int(b)) for a, b in segments if b > a]
    if merge and len(segs) == 2 and segs[1][0] == segs[0][1]:
        segs = [(segs[0][0], segs[1][1])]
    return segs


def tiles(segments, align: int = 32, merge: bool = True, index: bool = False) -> List[Tuple[int, ...]]:
    """(base, lo, hi) of every key tile, in the kernel's order: tiles of range [lo, hi) start at lo & ~31, step 64.  index: also the
    range's number.  align / merge exist for tests/test_mx_attn_edges_host.py, which shows what each of them decides."""
    out = []
    for g, (lo, hi) in enumerate(merge_segments(segments, merge)):
        base = lo & ~(align - 1)
        while base < hi:
            out.append((base, lo, hi, g) if index else (base, lo, hi))
            base += KT
    return out


def trunc_e4m3(p: Tensor) -> Tensor:
    """e4m3fn by truncation of non-negative p <= 448 (a wrong rounding mode, for the edge suite's mutation list)."""
    e = torch.floor(torch.log2(p.double().clamp_min(2.0 ** -40))).clamp_min(-6.0)
    step = torch.pow(2.0, e - 3)
    return (torch.floor(p.double() / step) * step).to(p.dtype)


def mx_attention(q: Tensor, kd: Tensor, vd: Tensor, segments, scale: float = None, dtype=torch.float32, rcp: bool = False,
                 mut=(), perm: torch.Generator = None, hook=None, v_tile=None) -> Tensor:
    """The kernel's arithmetic on dequantised shadows kd, vd [B, S32, H, 128] (deq_k / deq_v): q [B, Lq, H, 128] bf16 -> fp32 O / l
    [B, Lq, H, 128].  dtype: the accumulation type (float32 = the kernel's; float64 to measure the quantisation alone).  rcp: the
    kernel's normalisation, fp32(O) times the fp32 reciprocal of fp32(l), instead of one division (for data whose sums are exact).
    The rest serves the edge suite (tests/mx_attn_exact.py) and leaves the scheme alone when unset: mut names deliberate departures
    from the scheme (each a bug the suite must see), perm permutes the keys of every tile (the sums' order), hook(dict) receives every
    tile's terms, v_tile(base, idx) supplies a tile's V^ rows [B, H, 64, 128] instead of vd."""
    B, Lq, H, D = q.shape
    S32 = kd.shape[1]
    mut = {mut} if isinstance(mut, str) else set(mut)
    if scale is None:
        scale = 1.0 / math.sqrt(D)
    c = torch.tensor(scale * LOG2E, dtype=torch.float32).item()
    qc, qsc = mx_ref.quantize(q.reshape(-1, D).to(torch.bfloat16))
    qd = mx_ref.dequantize(qc, qsc).to(q.device).to(dtype).reshape(B, Lq, H, D).permute(0, 2, 1, 3)   # [B, H, Lq, D]
    kdh = kd.to(dtype).permute(0, 2, 1, 3)                                                            # [B, H, S32, D]
    vdh = vd.to(dtype).permute(0, 2, 1, 3)
    M = torch.full((B, H, Lq, 1), -math.inf, dtype=torch.float32, device=q.device)
    l = torch.zeros(B, H, Lq, 1, dtype=dtype, device=q.device)
    O = torch.zeros(B, H, Lq, D, dtype=dtype, device=q.device)
    for base, lo, hi, g in tiles(segments, 64 if "base64" in mut else 32, "unmerged" not in mut, index=True):
        slot_ids = base + torch.arange(KT, device=q.device)
        if perm is not None:
            slot_ids = slot_ids[torch.randperm(KT, generator=perm)]
        idx = slot_ids.clamp(max=S32 - 1)
        s = (qd @ kdh[:, :, idx].transpose(-1, -2)).float()                      # [B, H, Lq, 64] fp32 scores
        mlo = lo + ("mask:lo%d+" % g in mut) - ("mask:lo%d-" % g in mut)            # "mask:hi1-": range 1's end one slot early
        mhi = hi + ("mask:hi%d+" % g in mut) - ("mask:hi%d-" % g in mut)
        valid = (slot_ids >= mlo) & (slot_ids < mhi)
        s = s.masked_fill(~valid, -math.inf)
        tm = s.amax(-1, keepdim=True) * c
        if "nonlazy" in mut:
            Mn = torch.maximum(tm, M)
        elif "ge" in mut:
            Mn = torch.where(tm - M >= THR, tm, M)
        else:
            Mn = torch.where(tm - M > THR, tm, M)
        alpha = torch.exp2(M - Mn)
        p = torch.exp2(s * c - Mn)
        ph = (trunc_e4m3(p) if "trunc" in mut else p.to(FP8)).to(dtype)
        if "flush" in mut:
            ph = torch.where(ph < 2.0 ** -6, torch.zeros_like(ph), ph)
        ph = ph.masked_fill(~valid, 0.0)
        vt = vdh[:, :, idx] if v_tile is None else v_tile(base, idx).to(dtype)
        al, ao = alpha.to(dtype), alpha.to(dtype)
        if "no_l_rescale" in mut:
            al = torch.ones_like(al)
        if "no_o_rescale" in mut:
            ao = torch.ones_like(ao)
        if hook is not None:
            hook(dict(base=base, lo=lo, hi=hi, l_old=l * al, O_old=O * ao, ph=ph, v=vt, M=M, Mn=Mn, valid=valid))
        rs = p.to(dtype).masked_fill(~valid, 0.0) if "l_unrounded" in mut else ph
        l = l * al + rs.sum(-1, keepdim=True)
        O = O * ao + ph @ vt
        M = Mn
    if rcp:
        return (O.float() * (1.0 / l.float())).permute(0, 2, 1, 3)
    return (O / l).permute(0, 2, 1, 3).float()


def mx_attention_cache(q: Tensor, k: Tensor, v: Tensor, segments, scale: float = None, dtype=torch.float32,
                       rcp: bool = False) -> Tensor:
    """mx_attention straight from the bf16 cache k, v [B, S, H, 128] (shadows derived here)."""
    kd = deq_k(*shadow_k(k), dtype=dtype)
    vd = deq_v(*shadow_v(v), dtype=dtype)
    return mx_attention(q, kd, vd, segments, scale, dtype, rcp)


class MXAttnRefModel(QuantRefModel):
    """RefModel with self-attention on the MX shadow scheme.  linears: the mode of the six block linears (a set_quant name that
    tests/quant_ref.py restates), or None for the bf16 linears of the oracle.  The cache is the oracle's (bf16 k / v written as
    RefModel writes them); attention reads it through the shadow with ABSOLUTE slot indices, so the V^ blocks are the kernel's."""

    def __init__(self, *a, linears: Optional[str] = None, **kw):
        super().__init__(*a, mode=linears, **kw)

    def self_attn(self, x: Tensor, p: str, grid, kv_cache: dict, current_start: int, sink_recache_after_switch: bool):
        c = self.cfg
        b, s, n, d = x.shape[0], x.shape[1], c.num_heads, c.dim // c.num_heads
        q = R.rms_norm(self.lin(x, p + "q"), self.sd[p + "norm_q.weight"], c.eps).view(b, s, n, d)
        k = R.rms_norm(self.lin(x, p + "k"), self.sd[p + "norm_k.weight"], c.eps).view(b, s, n, d)
        v = self.lin(x, p + "v").view(b, s, n, d)
        frame_seqlen = grid[1] * grid[2]
        start_frame = current_start // frame_seqlen
        rq = R.causal_rope_apply(q, grid, self.freqs, start_frame).type_as(v)
        rk = R.causal_rope_apply(k, grid, self.freqs, start_frame).type_as(v)
        plan = R.kv_plan(current_start, s, kv_cache["global_end_index"], kv_cache["local_end_index"],
                         kv_cache["k"].shape[1], c.sink_size * frame_seqlen, self.local_attn_size,
                         self.max_attention_size, sink_recache_after_switch)
        R.kv_apply(kv_cache["k"], kv_cache["v"], plan, rk, v)
        y = mx_attention_cache(rq.to(torch.bfloat16), kv_cache["k"].to(torch.bfloat16), kv_cache["v"].to(torch.bfloat16),
                               plan["segments"]).to(self.dtype)
        return self.lin(y.flatten(2), p + "o"), plan
