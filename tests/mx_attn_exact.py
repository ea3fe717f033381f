"""Data constructions of the MXFP8 attention edge suite and their expected bits (plain helpers, no tests).  The scheme itself is
tests/mx_attn_ref.py's (shadow_k, shadow_v, tiles, mx_attention); nothing of it is restated here.

Exact attention data.  c = 1 (quant_exact.unit_c_scale).  A key slot j carries a LEVEL l_j (a multiple of 1/4) spread over three
32-channel blocks, a query row r an offset a_r, and up to nine PROBE keys answer one bit of the row number each:

    k_j = 1 e[o] + u_j e[o + 1] + [j probes bit i] e[32 + (o + i) % 32] + f_j e[64 + o] + w_j e[96 + o],   l_j = u_j + f_j / 4 + 4 w_j
    q_r = a_r e[o] + 1 e[o + 1] + sum_i bit_i(r) e[32 + (o + i) % 32] + 1/4 e[64 + o] + 4 e[96 + o]
    score(r, j) = a_r + l_j + [j probes bit i] bit_i(r)

(o depends on batch and head, w_j in {-1, 0, 1} on a hash, so every channel block of K^ and Q^ has its own scale and every row its own
softmax.)  Every block holds at most two magnitudes of <= 4 significant bits, so Q^ and K^ are exact.  V = w 2^p with integer
|w| <= 7 (x 8 on the slots a case marks `big`, 0 on those it marks `vzero`) and p in {-1, 0, 1} per (batch, head, channel, 32-slot
block): V^ is exact, both blocks of a tile differ in scale, every slot has its own V row.  With integer levels every P is a power of
two 2^-9 .. 2^8 or rounds to 0 (2^-10 is the tie below e4m3's smallest subnormal); quarter levels give P = 2^(n/4), whose e4m3
rounding is far from a tie (asserted through the fp32 / fp64 agreement of the restatement).  Whether the sums are exact in ANY order
is not assumed from this description: span_report() measures it per tile.

Kinds of case: `sweep` (range boundaries: the first and last slot of every range sit at level 0, the slots just outside at level +3,
everything else -3 .. 0 by hash: an off-by-one at any end of any range moves bits) and the lazy-max constructions, whose levels are
listed per slot (LAZY)."""
import math

import torch

import mx_attn_ref as MA
from bf16_exact import _hash_bits
from quant_exact import unit_c_scale

bf = torch.bfloat16
KT = MA.KT
SCALE = unit_c_scale()
NPROBE = 9
# Data seeds: the first seed (from 1) at which no expected element of the case lies within 3 fp32 ulp of a bf16 rounding tie
# (tests/test_mx_attn_edges_host.py asserts it); unlisted cases use 1.
SEEDS = {"s0n63": 3, "s0n65": 2, "s0n129": 3, "s1n32": 5, "s31n32": 4, "s31n64": 4, "s96n31": 3, "s96n65": 3, "s33n32": 2, "s33n64": 2,
         "s127n31": 3, "s127n63": 2, "s127n64": 5, "clamp_S90_two": 2, "two_share_block": 5, "batch2_heads3": 4,
         "q_batch2_heads4": 4, "q_heads12": 29, "q_s31n65_h2": 4}


class Case:
    """segs = [(lo, hi)] in the kernel's walk order.  levels: {slot: level} overriding the sweep rule (lazy cases list every in-range
    slot).  probes: slots answering row bits 0, 1, ... (default: the first interior in-range slots).  big / vzero / even: slots whose V is
    x 8 / zero / an even integer.  zero_k: all-zero K slots; zero_v: all-zero V blocks."""

    def __init__(self, name, B, Lq, H, S, segs, levels=None, probes=None, big=(), vzero=(), even=(), zero_k=(), zero_v=()):
        self.name, self.B, self.Lq, self.H, self.S, self.segs, self.seed = name, B, Lq, H, S, [tuple(s) for s in segs], SEEDS.get(name, 1)
        self.S32 = (S + 31) // 32 * 32
        self.levels, self.big, self.vzero, self.even, self.zero_k, self.zero_v = levels, big, vzero, even, zero_k, zero_v
        inr = [j for lo, hi in self.segs for j in range(lo, hi)]
        assert len(set(inr)) == len(inr) and all(0 <= lo < hi <= S for lo, hi in self.segs)
        self.inr = inr
        self.bounds = [j for lo, hi in self.segs for j in (lo, hi - 1)]
        self.outer = [j for lo, hi in self.segs for j in (lo - 1, hi) if 0 <= j < S and j not in set(inr)]
        if probes is None:
            probes = [j for j in inr if j not in self.bounds and j not in zero_k][:NPROBE]
        self.probes = list(probes)

    def __repr__(self):
        return self.name

    # ---- plan ------------------------------------------------------------------------------------------------------------------------
    def seg_args(self):
        (s0, e0), (s1, e1) = self.segs[0], (self.segs[1] if len(self.segs) > 1 else (0, 0))
        return s0, e0 - s0, s1, e1 - s1

    def plan_counts(self):
        """(key tiles, ranges) the kernel walks: the restatement's tile list."""
        t = MA.tiles(self.segs, index=True)
        return len(t), len({g for *_, g in t})

    def staged_blocks(self):
        """32-slot blocks some tile stages (the clamp re-reads the last block)."""
        NB = self.S32 // 32
        return sorted({min(b // 32 + i, NB - 1) for b, _, _ in MA.tiles(self.segs) for i in (0, 1)})

    def touched_blocks(self):
        return sorted({j // 32 for j in self.inr})

    # ---- data ------------------------------------------------------------------------------------------------------------------------
    def _hash(self, shape_idx, salt):
        return _hash_bits(shape_idx, self.seed * 7919 + salt)

    def build(self):
        """q [B, Lq, H, 128], k / v [B, S, H, 128] bf16."""
        B, Lq, H, S = self.B, self.Lq, self.H, self.S
        b = torch.arange(B).view(B, 1, 1)
        h = torch.arange(H).view(1, H, 1)
        j = torch.arange(S).view(1, 1, S)
        bhj = (b * H + h) * 4096 + j
        lev = -(self._hash(bhj, 11) % 4).double()                                  # [B, H, S]: 0 .. -3
        for s in self.bounds:
            lev[:, :, s] = 0.0
        for s in self.outer:
            lev[:, :, s] = 3.0
        for s, v in (self.levels or {}).items():
            lev[:, :, s] = v
        w = torch.round(torch.floor(lev) / 4) + (self._hash(bhj, 13) % 3).double() - 1      # |u| <= 6, |w| <= 9: one hex digit each
        f = torch.remainder(lev * 4, 4)
        u = torch.floor(lev) - 4 * w
        assert u.abs().max() <= 6 and w.abs().max() <= 9 and torch.equal(u + f / 4 + 4 * w, lev)
        o = ((5 * h + 3 * b) % 16).expand(B, H, 1)                                  # channel offset of (batch, head)
        k = torch.zeros(B, H, S, 128, dtype=torch.float64)
        q = torch.zeros(B, H, Lq, 128, dtype=torch.float64)
        r = torch.arange(Lq).view(1, 1, Lq)
        one_s, one_r = torch.ones(B, H, S, dtype=torch.float64), torch.ones(B, H, Lq, dtype=torch.float64)

        def put(t, ch, val):
            t.scatter_(3, ch.expand(val.shape).unsqueeze(-1), val.unsqueeze(-1))

        put(k, o, one_s); put(k, o + 1, u); put(k, 64 + o, f); put(k, 96 + o, w)
        put(q, o, ((r * 5) % 7 - 3).double().expand(B, H, Lq)); put(q, o + 1, one_r)
        put(q, 64 + o, 0.25 * one_r); put(q, 96 + o, 4 * one_r)
        for i, s in enumerate(self.probes):
            ch = 32 + (o + i) % 32
            put(k[:, :, s:s + 1], ch, one_s[:, :, :1])
            put(q, ch, ((r >> i) & 1).double().expand(B, H, Lq))
        for s in self.zero_k:
            k[:, :, s] = 0.0
        d = torch.arange(128).view(1, 1, 1, 128)
        bhjd = bhj.unsqueeze(-1) * 128 + d
        hv = self._hash(bhjd, 17)
        wv = ((hv >> 3) % 7 + 1).double() * (((hv >> 9) & 1).double() * 2 - 1)                 # +-1 .. +-7
        pv = (self._hash(((b * H + h) * 4096 + j // 32).unsqueeze(-1) * 128 + d, 19) % 3).double() - 1
        v = wv * torch.pow(2.0, pv)
        for s in self.big:
            v[:, :, s] *= 8
        for s in self.even:
            v[:, :, s] = 2 * wv[:, :, s]
        for s in self.vzero:
            v[:, :, s] = 0.0
        for blk in self.zero_v:
            v[:, :, 32 * blk:32 * blk + 32] = 0.0
        q, k, v = (t.permute(0, 2, 1, 3).contiguous() for t in (q, k, v))
        qb, kb, vb = q.to(bf), k.to(bf), v.to(bf)
        assert torch.equal(qb.double(), q) and torch.equal(kb.double(), k) and torch.equal(vb.double(), v)
        return qb, kb, vb


class Built:
    """A case's tensors, shadows and expected bits, computed once."""
    _cache = {}

    def __init__(self, case):
        self.case = case
        self.q, self.k, self.v = case.build()
        self.kq, self.ks = MA.shadow_k(self.k)
        self.vq, self.vs = MA.shadow_v(self.v)
        self.kd, self.vd = MA.deq_k(self.kq, self.ks), MA.deq_v(self.vq, self.vs)
        self.want32 = self.run()
        self.want = self.want32.to(bf)

    def run(self, dtype=torch.float32, **kw):
        return MA.mx_attention(self.q, self.kd, self.vd, self.case.segs, scale=SCALE, dtype=dtype, rcp=True, **kw)

    @classmethod
    def get(cls, case):
        if case.name not in cls._cache:
            cls._cache[case.name] = cls(case)
        return cls._cache[case.name]


# ---- the host proof's instruments ------------------------------------------------------------------------------------------------------
def lowbit(x):
    """The value of the lowest set bit of each float64 element (+inf at 0)."""
    m, e = torch.frexp(x.double())
    mi = (m.abs() * 2.0 ** 53).to(torch.int64)
    lb = (mi & -mi).double() * torch.pow(2.0, (e - 53).double())
    return torch.where(x != 0, lb, torch.full_like(lb, math.inf))


def span_report(built):
    """Worst log2(sum of |terms| / grain) over every tile's l and O updates, rescaled carry included.  grain = the coarsest power of two
    every term of the update is a multiple of (for O conservatively: the row's finest P^ times the tile's finest V^, against the
    element's rescaled carry).  Every partial sum of such terms, in any order and grouping, is a multiple of grain below the sum of
    magnitudes: below 24 bits of span it is exact in fp32."""
    worst = {"l": -math.inf, "O": -math.inf}

    def hook(t):
        ph, v = t["ph"].double(), t["v"].double()
        gp = lowbit(ph).amin(-1, keepdim=True)                                       # [B, H, Lq, 1]
        gl = torch.minimum(gp, lowbit(t["l_old"]))
        sl = ph.sum(-1, keepdim=True) + t["l_old"].abs()
        gv = lowbit(v).amin((-1, -2), keepdim=True)                                  # [B, H, 1, 1]
        go = torch.minimum(gp * gv, lowbit(t["O_old"]))
        so = ph @ v.abs() + t["O_old"].abs()
        for name, s, g in (("l", sl, gl), ("O", so, go)):
            ok = torch.isfinite(g) & (s > 0)
            if ok.any():
                worst[name] = max(worst[name], torch.log2(s[ok] / g.expand_as(s)[ok]).max().item())

    built.run(dtype=torch.float64, hook=hook)
    return worst


def tie_distance(x32):
    """Distance of fp32 values from the nearest bf16 rounding tie, in fp32 ulp (the low 16 bits against 0x8000)."""
    low = x32.contiguous().view(torch.int32) & 0xFFFF
    return (low - 0x8000).abs()


def rounding_error_bound(built):
    """Per element, how far ANY per-key rounding of P within the scheme's limits can move O / l from the fp64 softmax over the
    dequantised shadows: |dP_j| <= max(2^-4 P_j, 2^-10) in units in which the largest P is >= 1 (the lazy reference never exceeds the
    true maximum), and 0 for a P that is a power of two >= 2^-9 against the true maximum -- it is one against every lazy reference the
    integer tile maxima of these data allow, and e4m3 holds it.  Returns (softmax, bound) [B, Lq, H, 128] in fp64."""
    c = built.case
    idx = torch.tensor(c.inr)
    qd = MA.mx_ref.dequantize(*MA.mx_ref.quantize(built.q.reshape(-1, 128))).reshape(c.B, c.Lq, c.H, 128).permute(0, 2, 1, 3)
    kd, vd = built.kd.permute(0, 2, 1, 3)[:, :, idx], built.vd.permute(0, 2, 1, 3)[:, :, idx]
    s = qd @ kd.transpose(-1, -2)
    p = torch.exp2(s - s.amax(-1, keepdim=True))
    l = p.sum(-1, keepdim=True)
    out = (p @ vd) / l
    dp = torch.maximum(p * 2.0 ** -4, torch.full_like(p, 2.0 ** -10))
    dp = torch.where((torch.frexp(p)[0] == 0.5) & (p >= 2.0 ** -9), torch.zeros_like(p), dp)      # a power of two in e4m3's range: exact
    bound = (dp @ vd.abs() + dp.sum(-1, keepdim=True) * out.abs()) / (l - dp.sum(-1, keepdim=True)).clamp_min(2.0 ** -3)
    return out.permute(0, 2, 1, 3), bound.permute(0, 2, 1, 3)


# ---- mutations -------------------------------------------------------------------------------------------------------------------------
MASK_MUTS = [f"mask:{end}{g}{d}" for g in (0, 1) for end in ("lo", "hi") for d in "+-"]
LOOP_MUTS = ["nonlazy", "ge", "flush", "trunc", "l_unrounded", "no_l_rescale", "no_o_rescale", "base64"] + MASK_MUTS
DATA_MUTS = ["v_natural", "k_scale_neighbour", "v_scale_other"]


def run_mutant(built, mut):
    """The expected fp32 values under one named departure from the scheme."""
    if mut in LOOP_MUTS or mut == "unmerged":
        return built.run(mut=mut)
    if mut == "v_natural":                 # the kernel's P^ fragment against V^ codes stored in natural slot order
        vd = built.vd.reshape(built.case.B, -1, 32, built.case.H, 128)[:, :, MA.FRAG].reshape(built.vd.shape)
        return MA.mx_attention(built.q, built.kd, vd, built.case.segs, scale=SCALE, rcp=True)
    if mut == "k_scale_neighbour":         # every channel block of K^ under the scale byte of the next one
        kd = MA.deq_k(built.kq, built.ks.roll(1, -1))
        return MA.mx_attention(built.q, kd, built.vd, built.case.segs, scale=SCALE, rcp=True)
    if mut == "v_scale_other":             # each of a tile's two V^ blocks under the other one's scale bytes
        nxt, prv = MA.deq_v(built.vq, built.vs.roll(-1, 2)), MA.deq_v(built.vq, built.vs.roll(1, 2))      # block j under j + 1 / j - 1

        def v_tile(base, idx):
            first = (idx // 32 == base // 32).view(1, 1, -1, 1)
            return torch.where(first, nxt.permute(0, 2, 1, 3)[:, :, idx], prv.permute(0, 2, 1, 3)[:, :, idx])

        return built.run(v_tile=v_tile)
    raise KeyError(mut)


# ---- cases ---------------------------------------------------------------------------------------------------------------------------
def _sweep(name, B, Lq, H, S, segs, **kw):
    return Case(name, B, Lq, H, S, segs, **kw)


STARTS = (0, 1, 31, 96, 33, 127)            # mod 64: 0, 1, 31, 32, 33, 63
LENGTHS = (1, 31, 32, 33, 63, 64, 65, 129)
GEOMETRY = [_sweep(f"s{a}n{n}", 1, 33, 1 + 2 * ((a + n) % 2), a + n + 70, [(a, a + n)]) for a in STARTS for n in LENGTHS]

ENDS = [
    _sweep("end_S64", 1, 33, 1, 64, [(3, 64)]), _sweep("end_S65", 1, 33, 3, 65, [(40, 65)]), _sweep("end_S95", 1, 33, 1, 95, [(1, 95)]),
    # the clamp path: S32 / 32 odd and the range starts in the last block, so the last tile's second block lies past the shadow
    _sweep("clamp_S96", 1, 33, 1, 96, [(70, 96)]), _sweep("clamp_S65", 1, 33, 3, 65, [(64, 65)]), _sweep("clamp_S31", 1, 33, 1, 31, [(0, 31)]),
    _sweep("clamp_S90_two", 1, 33, 1, 90, [(65, 90), (2, 30)]),
]

TWO = [
    _sweep("two_apart", 1, 33, 3, 300, [(0, 40), (164, 300)]), _sweep("two_adjacent", 1, 33, 1, 200, [(5, 70), (70, 180)]),
    _sweep("two_share_block", 1, 33, 3, 128, [(0, 40), (50, 100)]), _sweep("two_share_tile", 1, 33, 1, 160, [(33, 60), (70, 129)]),
    _sweep("two_second_first", 1, 33, 3, 256, [(130, 200), (3, 66)]), _sweep("two_gap_one", 1, 33, 1, 140, [(1, 64), (65, 130)]),
]

ZERO = [_sweep("zero_k_and_v", 1, 33, 3, 200, [(20, 180)], zero_k=(40, 41, 97), zero_v=(2,))]

LQ = (1, 31, 32, 33, 127, 128, 129, 257)
ROWS = _sweep("rows", 1, 257, 3, 160, [(1, 40), (50, 131)])           # its first Lq rows serve every Lq (rows are independent)
BATCH = _sweep("batch2_heads3", 2, 129, 3, 200, [(130, 199), (31, 97)])


def _lazy(name, tile_max, kinds, probes=True, start=0, imax=5):
    """Range [start, start + 64 T).  Tile t holds its maximum tile_max[t] once (slot start + 64 t + imax, V = 0); every other level is set against the lazy
    reference M_t the scheme must hold in tile t, by the tile's kind; unlisted slots sit at M_t - 20 (P^ = 0).
      full    20 keys at M_t - 9 (P = 2^-9, the smallest e4m3 subnormal), 6 at M_t - 8.25 (2 x 2^-9 by RNE, 1 x by truncation) and 6 at
              M_t - 10 (the tie: rounds to 0), all with V x 8; 4 at M_t - 0.75 (10/16 by RNE, 9/16 truncated); 8 at M_t - 2
      plain   the 4 at M_t - 0.75 and the 8 at M_t - 2 only: a carry whose grain survives one rescale by 2^-11
      coarse  6 keys at M_t with even V: a carry whose grain survives two rescales by 2^-9
    Nine probe keys at tile_max[0] - 3 in tile 0 (not with a coarse first tile)."""
    T = len(tile_max)
    levels, big, vzero, even = {}, [], [], []
    M = None
    for t, (tm, kind) in enumerate(zip(tile_max, kinds)):
        M = tm if M is None or tm - M > MA.THR else M
        for i in range(64):
            s = start + 64 * t + i
            levels[s] = M - 20
            if i == imax:
                levels[s] = tm; vzero.append(s)
            elif kind == "coarse":
                if 8 <= i < 14:
                    levels[s] = M; even.append(s)
            elif kind == "full" and 8 <= i < 28:
                levels[s] = M - 9; big.append(s)
            elif kind == "full" and 28 <= i < 34:
                levels[s] = M - 8.25; big.append(s)
            elif kind == "full" and 34 <= i < 40:
                levels[s] = M - 10; big.append(s)
            elif 40 <= i < 44:
                levels[s] = M - 0.75
            elif 56 <= i < 64:
                levels[s] = M - 2
    pr = list(range(start + 44, start + 53)) if probes else []
    for s in pr:
        levels[s] = tile_max[0] - 3
    return Case(name, 1, 33, 1, start + 64 * T, [(start, start + 64 * T)], levels=levels, probes=pr, big=big, vzero=vzero, even=even)


LAZY = [
    _lazy("lazy_move9_stay8", [-8, 1, 9], ["plain", "plain", "full"]),                # +9: M moves; +8 above it: M stays, P = 256
    _lazy("lazy_rise_every_tile", [-9, 0, 9], ["coarse", "plain", "full"], probes=False),      # +9, +9: every tile rescales
    _lazy("lazy_first_only", [5, 1, 4, -3], ["full"] * 4),                           # the maximum in the first tile: no rescale
    _lazy("lazy_last_only", [-6, -6, -2, 5], ["plain", "plain", "plain", "full"]),   # +11 in the last tile only
    # tiles from slot 32: the first tile's maximum sits in its second block, which a walk from slot 0 (a & ~63) meets a tile later
    _lazy("lazy_from_32", [9, 0], ["full", "plain"], probes=False, start=32, imax=50),
]

RANDOM = {          # one random-data case per geometry class: (B, Lq, H, S, segs)
    "ragged_lq": (1, 131, 3, 300, [(0, 300)]),
    "clamped_tile": (2, 33, 3, 96, [(70, 96)]),
    "two_in_tile": (1, 65, 3, 160, [(33, 60), (70, 129)]),
}

EXACT_CASES = GEOMETRY + ENDS + TWO + ZERO + LAZY + [ROWS, BATCH]

# Even head counts, for the packed output formats of ll_flash_attn_mx_q (they pair heads in a super-block; every case above has
# H = 1 or 3 and serves the 8-bit format as it is): ROWS and BATCH again, one clamp case, H = 12, two single-range sweeps
QOUT_ROWS = _sweep("q_rows_h2", 1, 257, 2, 160, [(1, 40), (50, 131)])
QOUT_BATCH = _sweep("q_batch2_heads4", 2, 129, 4, 200, [(130, 199), (31, 97)])
QOUT_EVEN = [
    QOUT_ROWS, QOUT_BATCH, _sweep("q_clamp_S96_h2", 1, 33, 2, 96, [(70, 96)]), _sweep("q_heads12", 1, 33, 12, 200, [(33, 130)]),
    _sweep("q_s31n65_h2", 1, 33, 2, 166, [(31, 96)]), _sweep("q_s33n129_h2", 1, 33, 2, 232, [(33, 162)]),
]


def random_data(B, Lq, H, S, seed=23):
    """q, k, v of a random-data case (the distributions of tests/test_mx_attn_gpu.py)."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, Lq, H, 128, generator=g).to(bf)
    k = torch.randn(B, S, H, 128, generator=g).to(bf)
    v = (0.5 * torch.randn(B, S, H, 128, generator=g)).to(bf)
    return q, k, v
