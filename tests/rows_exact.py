"""Data constructions of the row / cache / latent edge suite (csrc/elementwise.hip and ll_linear_small) and their host references
(plain helpers, no tests; the conventions of tests/bf16_exact.py and tests/vae_exact.py).

Exact rows: x = m + c / 4 with integer codes c in -4 .. 4 whose sum over the row is exactly 0 and a per-row m in {0, 2, -2, 0.5}.
Every x is a bf16 value; |x| <= 3, so any partial sum of a row is a multiple of 1/4 below 12 C <= 24576 quanta (< 2^24): exact in
fp32 in ANY order, and the mean is exactly m.  The centred values are c / 4, their squares multiples of 1/16 below 1, any partial sum
of them below 16 C <= 32768 quanta: exact too.  With -ffp-contract=off every other step of a row kernel is ONE IEEE fp32 operation
per element (sum / C, + eps, sqrt, 1 / ., the products, the sums, the bf16 roundings), so on these rows the output has one correct
bit pattern: the chains below, evaluated in torch on the CPU with fp32 steps and an explicit .to(bf16) where the reference rounds.
RMSNorm and the q/k norm use m = 0 (then the sum of x^2 is the exact one).  The modulation / affine vectors and the tables are
GENERIC hash-normal bf16 values, not on a grid: every rounding point matters.

ll_linear_small: integer codes under powers of two; LINEAR_CODE_BOUND states the partial-sum bound per (K, code range).

Everything a test compares against comes from here and never from a kernel's output; the mutations of
tests/test_rows_edges_host.py are applied to these references only (the `mut` arguments)."""
import math

import torch

from bf16_exact import NAN16, ulp_bf16  # noqa: F401  (re-exported)
from vae_exact import hash_bits

bf = torch.bfloat16
f32 = torch.float32
EPS = 1e-6
WIDTHS = [8, 256, 512, 520, 768, 1024, 1280, 1536, 1792, 2040, 2048]     # every (NCH, FULL) of DISPATCH_NCH; 520: a ragged chunk of one
#                                                                          lane, 2040: of 63 lanes
ROW_GEOS = [(1, 1, 1), (1, 5, 1), (2, 3, 7)]       # (B, F, frame_len): 1, 5, 42 rows; 42: batch 1 starts and frames change mid-workgroup
MOD_PAIRS = [(0, 1), (3, 4)]                       # (shift_idx, scale_idx) of the model's two modulated norms
MEANS = [0.0, 2.0, -2.0, 0.5]
MOD_TABLE_SHAPES = [(1, 1, 6, 8, 0b010010), (3, 5, 6, 520, 0b010010), (2, 7, 2, 1536, 0b01)]   # (NL, BF, nmod, C, one_plus_mask): 6, 5850, 5376 chunks
# (C, head_dim) of ll_qk_norm_rope_kv_store: <1> ragged, <3> whole, <2> whole, <4> whole, <2> ragged (nf 12), ragged with a head that is
# no multiple of 16 (nf 8: the handover falls on a lane boundary, a head boundary inside a chunk row), one lane (nf 2)
QK_SHAPES = [(256, 128), (1536, 128), (1024, 128), (2048, 128), (768, 64), (520, 40), (8, 8)]
QK_B, QK_F, QK_FL = 2, 2, 15                       # frame_len 15 = a 3 x 5 frame
QK_START_FRAMES = [0, 1022]                        # 1022 + F = 1024: the last value the table bound admits
# (S, write_start, roped_offset, write_len): all tokens | the window ends at L and at S | one token | nothing (roped_offset > L)
QK_WINDOWS = [(36, 3, 0, 30), (26, 3, 7, 23), (9, 5, 16, 1), (6, 2, 31, 0)]


def rbf(t):
    """One bf16 rounding point: fp32 -> bf16 -> fp32."""
    return t.to(bf).to(f32)


def bits(t):
    return t.contiguous().view(torch.int16)


def hnorm(shape, seed, scale=1.0, shift=0.0):
    """Generic bf16 values: a Box-Muller normal from two integer hashes of the element index (the same on every host)."""
    n = 1
    for s in shape:
        n *= s
    i = torch.arange(n, dtype=torch.int64)
    u1 = (hash_bits(i, seed).double() + 0.5) / 2.0 ** 32
    u2 = (hash_bits(i, seed + 0x9E3779B1).double() + 0.5) / 2.0 ** 32
    z = torch.sqrt(-2.0 * torch.log(u1)) * torch.cos(2.0 * math.pi * u2)
    return (z * scale + shift).to(bf).view(*shape)


def int_codes(shape, seed, lo=-4, hi=4):
    n = 1
    for s in shape:
        n *= s
    b = hash_bits(torch.arange(n, dtype=torch.int64), seed)
    return ((b >> 9) % (hi - lo + 1) + lo).view(*shape)


# ---- exact rows -----------------------------------------------------------------------------------------------------------------------
def last_chunk_start(C):
    """First column of the row's last 512-column chunk (the ragged one where C % 512 != 0)."""
    return (C - 1) // 512 * 512


def zero_sum_codes(rows, C, seed, zero_row=None, tail_row=None):
    """int64 [rows, C] codes in -4 .. 4 with every row summing to 0.  zero_row: all zero; tail_row: non-zero in the last chunk only."""
    c = int_codes((rows, C), seed)
    free = torch.ones(rows, C, dtype=torch.bool)
    if zero_row is not None and zero_row < rows:
        c[zero_row] = 0
    if tail_row is not None and tail_row < rows:
        c[tail_row, :last_chunk_start(C)] = 0
        free[tail_row, :last_chunk_start(C)] = False
        if not c[tail_row].any():
            c[tail_row, -1], c[tail_row, -2] = 3, -3
    for _ in range(16):                               # one unit per eligible element per pass, towards a zero sum
        s = c.sum(-1, keepdim=True)
        if not s.any():
            break
        down = free & (c > -4) & (s > 0)
        up = free & (c < 4) & (s < 0)
        c = c - (down & (torch.cumsum(down, -1) <= s)).long() + (up & (torch.cumsum(up, -1) <= -s)).long()
    assert not c.sum(-1).any() and int(c.abs().max()) <= 4
    return c


def exact_rows(rows, C, seed, means=None, special=True):
    """(x [rows, C] bf16, m [rows] float64).  means: None = MEANS in turn, or one value for every row.  With special (and rows >= 5):
    row 1 is all zero (rstd = 1 / sqrt(eps)) and row 3 is non-zero in the last chunk only, both with mean 0."""
    zr, tr = (1, 3) if special and rows >= 5 else (None, None)
    c = zero_sum_codes(rows, C, seed, zr, tr)
    m = torch.tensor([MEANS[r % 4] if means is None else means for r in range(rows)], dtype=torch.float64)
    if zr is not None:
        m[zr] = m[tr] = 0.0
    x = m.view(-1, 1) + c.double() / 4
    assert 12 * C < 2 ** 24 and 16 * C < 2 ** 24          # the two partial-sum bounds of the module docstring
    assert torch.equal(x.to(bf).double(), x) and float(x.abs().max()) <= 3.0
    return x.to(bf), m


# ---- the row chains ---------------------------------------------------------------------------------------------------------------------
def op32(fn, *args):
    """ONE correctly rounded fp32 operation (fn: + - * / sqrt) on fp32 operands: evaluated in fp64 and rounded once.  fp64's 53 bits
    >= 2 x 24 + 2, so rounding the fp64 result to fp32 gives the correctly rounded fp32 result of these operations (torch's own
    vectorised fp32 sqrt is not correctly rounded on every host; tests/test_rows_edges_host.py holds this against numpy's float32)."""
    return fn(*[a.double() if isinstance(a, torch.Tensor) else float(torch.tensor(a, dtype=f32)) for a in args]).to(f32)


def inv_sqrt(sumsq, C, eps=EPS):
    """1 / sqrt(sumsq / C + eps) as four single fp32 operations on an fp32 tensor."""
    v = op32(torch.add, op32(torch.div, sumsq, float(C)), eps)
    return op32(torch.reciprocal, op32(torch.sqrt, v))


def _sum32(t):
    """Row sum: fp64 accumulation rounded to fp32 once -- the exact sum on the exact rows, where every order gives it."""
    return t.double().sum(-1).to(f32)


def center(x, mut=()):
    """(x - mean [rows, C] fp32, rstd [rows, 1] fp32) of layernorm_center.  Mutation 'cpad': C rounded up to whole chunks as divisor."""
    C = x.shape[-1]
    div = (C + 511) // 512 * 512 if "cpad" in mut else C
    xf = x.to(f32)
    mean = op32(torch.div, _sum32(xf), float(div))
    d = xf - mean.unsqueeze(-1)
    return d, inv_sqrt(_sum32(d * d), div).unsqueeze(-1)


def _frame_rows(B, L, F, mut=()):
    """Per row of [B L]: the index b F + f of its modulation vectors.  Mutation 'frame+1': those of the next row."""
    r = torch.arange(B * L)
    if "frame+1" in mut:
        r = (r + 1).clamp_max(B * L - 1)
    return (r // L) * F + (r % L) // (L // F)


def ln_modulate_host(x, e, mod, shift_idx, scale_idx, F, mut=()):
    """x [B, L, C], e [B, F, nmod, C], mod [nmod, C] or None (e is then the precomputed bf16(mod + e)) -> [B L, C] bf16:
    y = bf16(LN(x)); s1 = bf16(1 + bf16(mod_s + e_s)); out = bf16(bf16(y s1) + bf16(mod_t + e_t)).
    Mutations: 'no_round_y' (y kept in fp32), 'swap' (shift and scale exchanged), 'frame+1', 'cpad'."""
    B, L, C = x.shape
    if "swap" in mut:
        shift_idx, scale_idx = scale_idx, shift_idx
    d, rstd = center(x.reshape(B * L, C), mut)
    y = d * rstd if "no_round_y" in mut else rbf(d * rstd)
    ef = e.reshape(-1, e.shape[-2], C).to(f32)[_frame_rows(B, L, F, mut)]            # [rows, nmod, C]
    sc, t = ef[:, scale_idx], ef[:, shift_idx]
    if mod is not None:
        sc, t = rbf(mod[scale_idx].to(f32) + sc), rbf(mod[shift_idx].to(f32) + t)
    s1 = rbf(1.0 + sc)
    return (rbf(y * s1) + t).to(bf)


def ln_modulate_tab_host(x, tab, shift_idx, scale_idx, F, mut=()):
    """The same from the fp32 table of modulation_table_f32_host: out = bf16(bf16(bf16(LN(x)) s1) + t)."""
    B, L, C = x.shape
    if "swap" in mut:
        shift_idx, scale_idx = scale_idx, shift_idx
    d, rstd = center(x.reshape(B * L, C), mut)
    tf = tab.reshape(-1, tab.shape[-2], C)[_frame_rows(B, L, F, mut)]
    return (rbf(rbf(d * rstd) * tf[:, scale_idx]) + tf[:, shift_idx]).to(bf)


def modulation_table_host(e, mods):
    """e [BF, nmod, C], mods [NL, nmod, C] -> [NL, BF, nmod, C] bf16 = bf16(mods + e)."""
    return (mods.to(f32).unsqueeze(1) + e.to(f32).unsqueeze(0)).to(bf)


def modulation_table_f32_host(e, mods, one_plus_mask):
    t = modulation_table_host(e, mods).to(f32)
    for i in range(t.shape[2]):
        if (one_plus_mask >> i) & 1:
            t[:, :, i] = rbf(1.0 + t[:, :, i])
    return t


def layernorm_affine_host(x, w, b, mut=()):
    """F.layer_norm's (x - mean) rstd w + b in fp32 steps, rounded once.  Mutation 'round_y': an extra rounding of the normalised value."""
    d, rstd = center(x, mut)
    y = rbf(d * rstd) if "round_y" in mut else d * rstd
    return (y * w.to(f32) + b.to(f32)).to(bf)


def rmsnorm_host(x, w, mut=()):
    """WanRMSNorm: bf16(bf16(x rinv) w).  Mutation 'no_round_y'."""
    xf = x.to(f32)
    y = xf * inv_sqrt(_sum32(xf * xf), x.shape[-1]).unsqueeze(-1)
    return ((y if "no_round_y" in mut else rbf(y)) * w.to(f32)).to(bf)


# ---- q/k norm + RoPE + KV insert ------------------------------------------------------------------------------------------------------
def rope_nf(head_dim):
    half = head_dim // 2
    return half - 2 * (half // 3)


def rope_hash_tables(nfr, head_dim, frame_len):
    """Hash-valued fp32 (cos, sin) tables rope_f [nfr, nf, 2], rope_hw [frame_len, half - nf, 2] with EVERY entry distinct: entry i
    holds ((i 40503 mod 2^17) 2^7 + 7 hash bits) / 2^23 - 1, a bijection of the index scattered over [-1, 1)."""
    half, nf = head_dim // 2, rope_nf(head_dim)
    n = nfr * nf * 2 + frame_len * (half - nf) * 2
    assert n < 2 ** 17
    i = torch.arange(n, dtype=torch.int64)
    v = ((((i * 40503) % 2 ** 17) << 7) | (hash_bits(i, 77) & 127)).double() / 2.0 ** 23 - 1.0
    assert torch.equal(v.to(f32).double(), v)
    v = v.to(f32)
    return v[:nfr * nf * 2].view(nfr, nf, 2).clone(), v[nfr * nf * 2:].view(frame_len, half - nf, 2).clone()


def rope_model_tables(nfr, head_dim, hp, wp):
    """The model's tables (CausalWanModelHIP._rope_tables; wan/modules/model.py:29-36, causal_model.py:622-629): fp32 (cos, sin) of the
    reference's fp64 angles, frame axis | (h angles, w angles) per spatial token."""
    d, half = head_dim, head_dim // 2
    c3, nf = half // 3, rope_nf(head_dim)

    def angles(n, dim):
        return torch.outer(torch.arange(n, dtype=torch.float64), 1.0 / torch.pow(10000.0, torch.arange(0, dim, 2, dtype=torch.float64).div(dim)))

    a = angles(nfr, d - 4 * (d // 6))
    assert a.shape[1] == nf
    rf = torch.stack([a.cos(), a.sin()], -1).to(f32)
    ah, aw = angles(hp, 2 * (d // 6)), angles(wp, 2 * (d // 6))
    a = torch.cat([ah.view(hp, 1, c3).expand(hp, wp, c3), aw.view(1, wp, c3).expand(hp, wp, c3)], -1).reshape(hp * wp, 2 * c3)
    return rf.contiguous(), torch.stack([a.cos(), a.sin()], -1).to(f32).contiguous()


def qk_rope_host(x, w, rope_f, rope_hw, L, frame_len, start_frame, head_dim, mut=()):
    """x [rows, C] bf16 (the q or the k third), w [C] -> roped [rows, C] bf16: a = bf16(bf16(x rinv) w) per element, then per pair
    (a, b) of a head: bf16(a cos - b sin), bf16(a sin + b cos), every product and sum rounded to fp32 separately.  Pair p of a head takes
    rope_f[frame, p] for p < nf, else rope_hw[spatial, p - nf].
    Mutations: 'frame+1' (the frame of row + 1), 'nf+1' / 'nf-1' (the handover moved), 'no_mod' (the pair index not reduced modulo the
    head), 'no_round_y' (the normalised value kept in fp32)."""
    rows, C = x.shape
    half, nf = head_dim // 2, rope_nf(head_dim)
    xf = x.to(f32)
    y = xf * inv_sqrt(_sum32(xf * xf), C).unsqueeze(-1)
    a = rbf((y if "no_round_y" in mut else rbf(y)) * w.to(f32))
    r = torch.arange(rows)
    t = ((r + 1).clamp_max(rows - 1) if "frame+1" in mut else r) % L
    f, sp = t // frame_len + start_frame, r % L % frame_len
    p = torch.arange(C // 2)
    if "no_mod" not in mut:
        p = p % half
    nfm = nf + (1 if "nf+1" in mut else -1 if "nf-1" in mut else 0)
    ff, fh = rope_f.reshape(-1, 2), rope_hw.reshape(-1, 2)
    idx_f = (f.view(-1, 1) * nf + p.view(1, -1)).clamp_max(ff.shape[0] - 1)
    idx_h = (sp.view(-1, 1) * (half - nf) + p.view(1, -1) - nfm).clamp(0, fh.shape[0] - 1)
    cs = torch.where((p < nfm).view(1, -1, 1), ff[idx_f], fh[idx_h])                  # [rows, C / 2, 2]
    ae, ao, cx, sy = a[:, 0::2], a[:, 1::2], cs[..., 0], cs[..., 1]
    out = torch.empty(rows, C, dtype=bf)
    out[:, 0::2] = (ae * cx - ao * sy).to(bf)
    out[:, 1::2] = (ae * sy + ao * cx).to(bf)
    return out


def kv_insert_host(cache, new, S, write_start, roped_offset, write_len, mut=()):
    """cache [B, S, C] (copied), new [B, L, C]: slots [write_start, +write_len) take tokens [roped_offset, +write_len).
    Mutation 'window+1': the slots one further on."""
    out = cache.clone()
    ws = write_start + (1 if "window+1" in mut else 0)
    if write_len > 0:
        out[:, ws:ws + write_len] = new[:, roped_offset:roped_offset + write_len]
    return out


class QKData:
    """One (C, head_dim): qkv [B L, 3C] with exact q and k thirds (m = 0; a zero row and a last-chunk-only row in each, on different
    rows) and a generic v third, generic norm weights."""

    def __init__(self, C, head_dim, seed=11):
        self.C, self.D, self.B, self.F, self.fl = C, head_dim, QK_B, QK_F, QK_FL
        self.L = QK_F * QK_FL
        rows = self.B * self.L
        q = zero_sum_codes(rows, C, seed, zero_row=1, tail_row=3).double() / 4
        k = zero_sum_codes(rows, C, seed + 1, zero_row=34, tail_row=47).double() / 4
        self.q, self.k = q.to(bf), k.to(bf)
        self.v = hnorm((rows, C), seed + 2, 0.7)
        self.qkv = torch.cat([self.q, self.k, self.v], -1).contiguous()
        self.wq, self.wk = hnorm((C,), seed + 3, 0.1, 1.0), hnorm((C,), seed + 4, 0.1, 1.0)

    def tables(self, kind, start_frame):
        """rope_f with exactly start_frame + F rows, rope_hw with frame_len rows ('hash' or 'model')."""
        nfr = start_frame + self.F
        return rope_hash_tables(nfr, self.D, self.fl) if kind == "hash" else rope_model_tables(nfr, self.D, 3, 5)

    def expected(self, kind, start_frame, mut=()):
        """(q_out [B L, C], roped k [B, L, C]) bf16."""
        rf, rhw = self.tables(kind, start_frame)
        a = (rf, rhw, self.L, self.fl, start_frame, self.D, mut)
        return qk_rope_host(self.q, self.wq, *a), qk_rope_host(self.k, self.wk, *a).view(self.B, self.L, self.C)


# ---- cache and latent kernels -----------------------------------------------------------------------------------------------------------
KV_ROLL_CASES = [(1, 6200, 1536, 0, 3000, 3100),    # 576 000 16-byte chunks in the first launch (> 2048 x 256: the grid-stride loop), then 100 rows
                 (2, 40, 8, 3, 4, 30),              # step 1: 30 launches, one chunk per row, batch stride
                 (1, 64, 264, 5, 12, 20),           # n no multiple of the step (7, 7, 6)
                 (2, 16, 8, 2, 9, 0)]               # n = 0: nothing moves
LATENT_SHAPES = [(1, 1, 1, 2, 2), (1, 2, 3, 6, 10), (2, 3, 16, 8, 12)]      # (B, F, C, H, W): 2, 360 and 4608 = 18 x 256 threads of work
ADD_NOISE_SHAPES = [(1, 8), (3, 2056), (5, 1536)]
SIGMA_GENERIC = 0.8408203125 + 2.0 ** -20                                    # an fp32 value that is no bf16 value
SINUSOID_CASES = [(2, [0.0]), (6, [0.0, 1000.0, 937.5, -3.25, 833.3333]),
                  (256, [1000.0, 937.5, 833.3333, 625.0, 0.0, 3.0, 17.0, 999.0, 500.0, 250.0, -42.0, 7.5]), (1536, [1000.0, 0.0, -17.5])]


def hash_bf16_bits(shape, seed):
    """int16 [shape]: hash-valued bit patterns (finite bf16 values: the exponent field is never all ones)."""
    n = 1
    for s in shape:
        n *= s
    b = hash_bits(torch.arange(n, dtype=torch.int64), seed) & 0xFFFF
    b = torch.where((b & 0x7F80) == 0x7F80, b & 0xBFFF, b)
    return torch.where(b >= 0x8000, b - 0x10000, b).to(torch.int16).view(*shape)


def kv_roll_host(cache, dst, src, n):
    """cache [B, S, C] -> cache[:, dst:dst + n] = the old cache[:, src:src + n]."""
    out = cache.clone()
    out[:, dst:dst + n] = cache[:, src:src + n]
    return out


def patchify_host(x):
    """patches[b, (f, h, w), c 4 + p 2 + q] = x[b, f, c, 2h + p, 2w + q]."""
    B, F, C, H, W = x.shape
    return x.view(B, F, C, H // 2, 2, W // 2, 2).permute(0, 1, 3, 5, 2, 4, 6).reshape(B, F * (H // 2) * (W // 2), C * 4).contiguous()


def unpatchify_host(head, B, F, C, H, W):
    """flow[b, f, c, 2h + q, 2w + r] = head[b, (f, h, w), (q 2 + r) C + c]: the inverse permutation."""
    return head.view(B, F, H // 2, W // 2, 2, 2, C).permute(0, 1, 6, 2, 4, 3, 5).reshape(B, F, C, H, W).contiguous()


def x0_host(xt, flow, sigma):
    """bf16(float(double(xt) - double(sigma[b, f]) double(flow)))  (utils/wan_wrapper.py:189-199)."""
    B, F = xt.shape[:2]
    return (xt.double() - sigma.double().view(B, F, 1, 1, 1) * flow.double()).to(f32).to(bf)


def add_noise_host(x0, nz, sigma):
    """bf16((1 - s) x0 + s n), four separately rounded fp32 operations; x0 / nz [N, inner], sigma [N] fp32."""
    s = sigma.to(f32).view(-1, 1)
    return ((1.0 - s) * x0.to(f32) + s * nz.to(f32)).to(bf)


def sinusoid_host(t, dim):
    """fp64 [cos(t w_j), sin(t w_j)], w_j = 10000^(-j / half) (wan/modules/model.py:15-25)."""
    half = dim // 2
    a = torch.outer(t.double(), torch.pow(10000.0, -torch.arange(half, dtype=torch.float64).div(half)))
    return torch.cat([a.cos(), a.sin()], 1)


def sigma_tables():
    """name -> (timesteps, sigmas) fp32: the scheduler's 1000 entries; 5, 64 and 65 integers 8 apart (every midpoint exact); 64 entries
    with a repeated timestep (entries 20 and 21).  Sigmas are distinct everywhere, so a wrong index shows."""
    from oracle import ref_ops as R
    sch = R.FlowMatchSchedulerRef(5.0)
    out = {"real": (sch.timesteps.to(f32).clone(), sch.sigmas.to(f32).clone())}
    for n in (5, 64, 65):
        out[f"n{n}"] = (1000.0 - 8.0 * torch.arange(n, dtype=f32), 1.0 - torch.arange(n, dtype=f32) / 128)
    ts, sg = out["n64"][0].clone(), out["n64"][1].clone()
    ts[21] = ts[20]
    out["repeat"] = (ts, sg)
    return out


def sigma_queries(ts):
    """Every table value, the midpoints of neighbours, values beyond both ends, +-inf, NaN."""
    mid = ((ts[:-1].double() + ts[1:].double()) / 2).to(f32)
    lo, hi = float(ts.min()), float(ts.max())
    ext = torch.tensor([lo - 0.5, lo - 1e4, hi + 0.5, hi + 1e4, float("inf"), float("-inf"), float("nan")], dtype=f32)
    return torch.cat([ts, mid, ext])


def sigma_lookup_host(t, ts, sg, mut=()):
    """sigmas[argmin_i |timesteps[i] - t|] with fp64 distances; the lowest index wins a tie (and an all-NaN / all-inf row gives 0).
    Mutation 'tie_up': the highest index wins."""
    d = (ts.double().unsqueeze(0) - t.double().unsqueeze(1)).abs()
    idx = torch.argmin(d, 1)
    if "tie_up" in mut:
        idx = d.shape[1] - 1 - torch.argmin(d.flip(1), 1)
    return sg[idx]


# ---- ll_linear_small ------------------------------------------------------------------------------------------------------------------
LINEAR_M, LINEAR_N, LINEAR_K = [1, 3, 8], [1, 6, 258], [8, 504, 512, 520, 1536]
LINEAR_ACT_IN_K = [8, 256]
# |any partial sum of products| in quanta of the product grid: codes -4 .. 4 on both sides -> 16 K; act_in: bf16(silu(x)) for |x| <= 4
# is a multiple of 2^-11 below 4 (2^13 quanta; asserted in linear_act_in_values) times |w| <= 2 -> 2^14 K
LINEAR_CODE_BOUND = {K: 16 * K for K in LINEAR_K}
LINEAR_ACT_IN_BOUND = {K: 2 ** 14 * K for K in LINEAR_ACT_IN_K}
assert all(v < 2 ** 24 for v in list(LINEAR_CODE_BOUND.values()) + list(LINEAR_ACT_IN_BOUND.values()))
SILU_MARGIN = 2.0 ** -18            # act_in: fp64 SiLU must lie further than this (relative) from a bf16 rounding boundary
SILU_MAX_DROPPED = 3
# act_out = 1: the kernel within 1 bf16 ulp of fp64 SiLU of the exact pre-activation rounded once, and its bit-exact share no more than
# this below torch's own (fp32 SiLU rounded to bf16 against the same fp64 value on the same inputs; the shares measured per K are in
# tests/test_rows_edges_gpu.py next to the assertion)
SILU_SHARE_SLACK = 0.01


class LinearData:
    """x [M, K] = codes -4 .. 4 x 2^-(m % 3), w [N, K] = codes -4 .. 4 x 2^(sh - n % 3) with sh chosen so that the outputs are O(1),
    bias generic bf16.  acc = the exact fp64 product; pre = bf16(fp32(acc) + bias): acc is exact in fp32 (LINEAR_CODE_BOUND), so the one
    fp32 addition and the rounding leave one bit pattern."""

    def __init__(self, M, N, K, seed=5):
        assert LINEAR_CODE_BOUND[K] < 2 ** 24
        self.M, self.N, self.K = M, N, K
        sh = -round(math.log2(60 / 9 * math.sqrt(K)))
        self.sx, self.sw = torch.pow(2.0, -(torch.arange(M) % 3).double()), torch.pow(2.0, sh - (torch.arange(N) % 3).double())
        x = int_codes((M, K), seed + K).double() * self.sx.view(-1, 1)
        w = int_codes((N, K), seed + K + 1).double() * self.sw.view(-1, 1)
        w[:, 0] = (torch.arange(N) % 3 + 1).double() * 2.0 ** sh
        self.x, self.w, self.bias = x.to(bf), w.to(bf), hnorm((N,), seed + 2, 0.5)
        assert torch.equal(self.x.double(), x) and torch.equal(self.w.double(), w)
        self.acc = x @ w.t()
        # per output one product grid sx[m] sw[n]: the sum of |products| in its quanta is the bound on every partial sum
        assert float(((x.abs() @ w.abs().t()) / (self.sx.view(-1, 1) * self.sw.view(1, -1))).max()) <= LINEAR_CODE_BOUND[K]
        assert torch.equal(self.acc.to(f32).double(), self.acc)
        self.pre = (self.acc.to(f32) + self.bias.to(f32)).to(bf)

    def silu64(self):
        """fp64 SiLU of the exact pre-activation (not yet rounded)."""
        p = self.pre.double()
        return p / (1.0 + torch.exp(-p))


def silu_boundary_margin(v):
    """Relative distance of fp64 values from the nearest bf16 rounding boundary (the midpoint of two neighbouring bf16 values)."""
    u = ulp_bf16(v)
    frac = (v.abs() / u) % 1.0                            # position inside the bf16 interval, in ulp
    return (frac - 0.5).abs() * u / v.abs()


def linear_act_in_values():
    """The grid values c / 4, |c| <= 16, whose bf16(silu(x)) is determined whatever the fp32 evaluation: fp64 SiLU further than
    SILU_MARGIN (relative) from a rounding boundary (0 included: x rcp(.) is 0 exactly).  Returns (x values float64, bf16(silu) float64)."""
    x = torch.arange(-16, 17).double() / 4
    s = x / (1.0 + torch.exp(-x))
    keep = (x == 0) | (silu_boundary_margin(torch.where(x == 0, torch.ones_like(s), s)) > SILU_MARGIN)
    assert int((~keep).sum()) <= SILU_MAX_DROPPED
    x, s = x[keep], s[keep].to(bf).double()
    assert torch.equal((s * 2 ** 11).round(), s * 2 ** 11) and float(s.abs().max()) < 4.0       # multiples of 2^-11 below 4
    return x, s


class LinearActInData:
    """act_in = 1: x takes the values of linear_act_in_values, w integer codes -2 .. 2, bias generic.  The products of bf16(silu(x)) and w
    sum exactly (LINEAR_ACT_IN_BOUND), so out = bf16(fp32(acc) + bias) has one bit pattern."""

    def __init__(self, M, N, K, seed=9):
        assert LINEAR_ACT_IN_BOUND[K] < 2 ** 24
        xv, sv = linear_act_in_values()
        pick = hash_bits(torch.arange(M * K, dtype=torch.int64), seed + K) % len(xv)
        self.x = xv[pick].view(M, K).to(bf)
        w = int_codes((N, K), seed + K + 1, -2, 2).double()
        self.w, self.bias = w.to(bf), hnorm((N,), seed + 2, 0.5)
        self.acc = sv[pick].view(M, K) @ w.t()
        assert float((sv[pick].view(M, K).abs() @ w.abs().t()).max()) * 2 ** 11 <= LINEAR_ACT_IN_BOUND[K]        # in quanta of 2^-11
        assert torch.equal(self.acc.to(f32).double(), self.acc)
        self.want = (self.acc.to(f32) + self.bias.to(f32)).to(bf)
