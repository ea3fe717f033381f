"""Data of the code-emitting attention edge suites (plain helpers, no tests): an exact "picked row" construction for the generated
kernels flash_attn_asm_mx / mx6 / mx4_kernel over a geometry (B, Lq, H, [(start, len)...]), and the geometry list.  The formats, the
host quantisers (QUANT), the packed-row layout (head_code_bytes, expected) and the edge blocks are tests/attn_qout_emu.py's;
nothing of them is restated here.

Every in-range key slot j of (b, head) carries its own +-1 pattern s_j of 128 entries, k_j = 20 s_j; query row r picks the slot
pos[b, head, r] of the range and has q_r = s_pos.  The picked key scores 20 x 128, any other key 20 x dot(s_pos, s_j): with |dot| < 69
it trails by more than 150 binary orders of scale x log2 e x score under scale = 128^-0.5, so its probability is 0 in fp32 (flushed
or not: the smallest subnormal is 2^-149), l = 1 and the output row is V[pos] bit for bit.  The expected bytes are the HOST
quantiser's of those V rows: no kernel and no device quantiser has a part in them.

  pos      a permutation of the range's slots per (b, head) (rows share slots when Lq exceeds the key count): a row written to another
           head's or batch element's bytes moves bytes.  The first and the last slot of the range are each picked in every (b, head)
           (Lq = 1 has one row per (b, head): they alternate between the two ends).
  decoys   every slot OUTSIDE the range -- start - 1, start + len, the rest of a ragged last tile and a tile beyond -- holds the
           picked key of some query row and a V row of large distinct values: a kernel that admits one of them gives that row l = 2
           and other bytes.
  V        block maxima over sixteen binades with exact zeros; on rows of the first and of the last wave of the last workgroup, in
           both 32-row halves of the wave, the edge blocks (zero block, amax at / one ulp above / one ulp below the largest code,
           ties, the clamped exponent), each also rotated by four channels so that the block's maximum sits in the upper 32 lanes
           (a lane (r, h) holds channels 32 db + 8 g4 + 4 h + (0..3)).  One block of every such row stays random: heads differ."""
import math

import numpy as np
import torch

import bf16_exact
from attn_qout_emu import BITS, QUANT, bf16_bits, bf16_val, edge_blocks, head_code_bytes  # noqa: F401  (re-exported)
from longlive_amd import synth

D = 128
KT = 64
AMP = 20.0
SCALE = 1.0 / math.sqrt(D)
LEAD_MIN = 150.0                   # binary orders every other in-range key trails the picked one by (asserted per case)
DOT_MAX = 69                       # |dot| of two distinct patterns stays below this
WG_ROWS = 256                      # query rows per workgroup of the generated kernels, 4 waves x 64 rows
FMTS = ["mx", "mx6", "mx4"]
# seeds: the first (from 1) for which the lead condition holds in every (b, head); unlisted geometries use 1
SEEDS = {}

# (B, Lq, H, [(start, len), ...]): bf16_exact.ASM_CASES with even head counts (attn_asm_min_keys lowered to 128 for all of them) ...
QOUT_ASM_CASES = [(B, Lq, H + (H & 1), rg) for B, Lq, H, rg in bf16_exact.ASM_CASES]
# ... and two adjacent-range cases with a ragged seam, which the entry point merges
QOUT_ASM_CASES += [(1, 129, 2, [(1, 65), (66, 511)]), (2, 257, 4, [(37, 100), (137, 1337)])]
# MX (8-bit) only: odd head counts
QOUT_ASM_ODD = [(1, 33, 1, [(63, 512)]), (1, 33, 3, [(1, 129)]), (1, 257, 1, [(64, 513)]), (1, 257, 3, [(37, 511)])]

EDGE_COMBOS = [("zero", 0), ("clamp", 0), ("amax_at_max", 0), ("amax_one_ulp_above", 0), ("amax_one_ulp_below", 0), ("clamp", 4),
               ("amax_at_max", 4), ("amax_one_ulp_above", 4), ("amax_one_ulp_below", 4), ("zero", 0)]


def hash_qkv(tag, B, Lq, H, Sk, dev="cuda"):
    """Hash q [B, Lq, H, 128], k and v [B, Sk, H, 128] (bf16, on dev): V with block maxima over several binades and exact zeros, so
    scale bytes, subnormal codes and zero codes all occur."""
    def hn(name, shape):
        return synth.hash_normal(151, name, shape).to(torch.bfloat16).to(dev)
    v = synth.hash_normal(151, tag + "v", (B, Sk, H, 128)) * torch.exp2(torch.arange(B * Sk * H * 4).view(B, Sk, H, 4).remainder(9).sub(4).float()
                                                                        ).repeat_interleave(32, -1)
    v[..., ::7] = 0.0
    return hn(tag + "q", (B, Lq, H, 128)), hn(tag + "k", (B, Sk, H, 128)), v.to(torch.bfloat16).to(dev)


def case_id(g):
    return f"B{g[0]}-Lq{g[1]}-H{g[2]}-{g[3]}".replace(" ", "")


def merged(ranges):
    """(start, len) of the one range the entry point walks: adjacent ranges are one."""
    s, n = ranges[0]
    for s1, n1 in ranges[1:]:
        assert s1 == s + n, ranges
        n += n1
    return s, n


def edge_zones(Lq):
    """Rows that carry edge blocks: up to four rows from the start of each 32-row half of the first and of the last wave (with valid
    rows) of the last workgroup -> [(wave, half, [rows])]."""
    q0 = (Lq - 1) // WG_ROWS * WG_ROWS
    waves = sorted({0, (Lq - q0 - 1) // 64})
    zones = []
    for w in waves:
        for half in (0, 1):
            r0 = q0 + 64 * w + 32 * half
            rows = [r for r in range(r0, r0 + 4) if r < Lq]
            if rows:
                zones.append((w, half, rows))
    return zones


class Picked:
    """One geometry's tensors as bf16 bit arrays (q [B, Lq, H, 128], k / v [B, Sk, H, 128]), pos [B, H, Lq] (slot numbers), and
    the expected bytes per format."""
    _cache = {}

    def __init__(self, B, Lq, H, ranges, fmt, seed=None):
        self.B, self.Lq, self.H, self.ranges, self.fmt = B, Lq, H, [tuple(r) for r in ranges], fmt
        self.start, self.n = merged(self.ranges)
        self.end = self.start + self.n
        self.nt = (self.n + KT - 1) // KT
        self.Sk = self.start + KT * self.nt + KT
        self.seed = SEEDS.get((B, Lq, H, self.start, self.n), 1) if seed is None else seed
        self.outside = [j for j in range(self.Sk) if not self.start <= j < self.end]
        # nearest first: the slot below the range, the slot at its end, the rest of the ragged last tile
        self.near = [j for j in [self.start - 1] + list(range(self.end, self.start + KT * self.nt + 1)) if 0 <= j < self.Sk]
        rng = np.random.default_rng(1000003 * self.seed + 7919 * Lq + 131 * self.n + 17 * self.start + 3 * H + B)
        n, st = self.n, self.start
        s = rng.choice([-1.0, 1.0], size=(B, H, n, D)).astype(np.float32)
        pos = np.zeros((B, H, Lq), dtype=np.int64)
        for b in range(B):
            for h in range(H):
                perm = rng.permutation(n)
                i = b * H + h
                if Lq == 1:
                    want = {0: 0 if i % 2 == 0 else n - 1}
                else:
                    r0 = (3 * h + b) % min(Lq, n)
                    r1 = (r0 + 1 + h) % min(Lq, n)
                    r1 = r1 if r1 != r0 else (r0 + 1) % min(Lq, n)
                    want = {r0: 0, r1: n - 1}
                for r, slot in want.items():
                    at = int(np.nonzero(perm == slot)[0][0])
                    perm[[r, at]] = perm[[at, r]]
                pos[b, h] = perm[np.arange(Lq) % n]
        self.pos = pos + st
        v = (rng.standard_normal((B, self.Sk, H, D)) * np.exp2(rng.integers(-8, 8, (B, self.Sk, H, 4)).repeat(32, -1))).astype(np.float32)
        v[rng.random(v.shape) < 0.05] = 0.0
        k = np.zeros((B, self.Sk, H, D), dtype=np.float32)
        q = np.zeros((B, Lq, H, D), dtype=np.float32)
        blocks = edge_blocks(fmt)
        self.decoy_row = {}
        for b in range(B):
            for h in range(H):
                k[b, st:self.end, h] = AMP * s[b, h]
                q[b, :, h] = s[b, h][pos[b, h]]
                for i, j in enumerate(self.near + [j for j in self.outside if j not in self.near]):
                    r = i % Lq                                          # the decoy is the picked key of row r ...
                    k[b, j, h] = AMP * s[b, h][pos[b, h, r]]
                    sign = np.where((np.arange(D) + j) % 3 == 0, -1.0, 1.0)
                    v[b, j, h] = sign * 4096.0 * (1.0 + (j % 64) / 64.0 + ((np.arange(D) * 5 + h) % 16) / 1024.0)      # ... with a loud V row
                    self.decoy_row[(b, h, j)] = r
                cnt = 3 * (b * H + h)
                for w, half, rows in edge_zones(Lq):
                    for i, r in enumerate(rows):
                        for db in range(4):
                            if db == (i + h) % 4:
                                continue                                 # one block stays random: heads differ
                            name, roll = EDGE_COMBOS[cnt % len(EDGE_COMBOS)]
                            cnt += 1
                            v[b, self.pos[b, h, r], h, 32 * db:32 * db + 32] = np.roll(blocks[name], roll)
        self.q, self.k, self.v = bf16_bits(q), bf16_bits(k), bf16_bits(v)
        assert np.array_equal(bf16_val(self.q), q) and np.array_equal(bf16_val(self.k), k)
        self.check_lead(s, pos)
        # the output rows: V[pos]
        bi, hi = np.arange(B)[:, None, None], np.arange(H)[None, :, None]
        self.rows_bits = self.v[bi, self.pos, hi].transpose(0, 2, 1, 3).copy()          # [B, Lq, H, 128]
        x = torch.from_numpy((self.rows_bits.reshape(B * Lq, H * D).astype(np.uint32) << 16).view(np.float32).copy()).to(torch.bfloat16)
        codes, scales = QUANT[fmt](x)
        self.codes = np.ascontiguousarray(codes).reshape(B * Lq, H * 16 * BITS[fmt]).view(np.uint8)
        self.scales = np.ascontiguousarray(scales).reshape(B * Lq, H * 4).view(np.uint8)

    def check_lead(self, s, pos):
        """Every other in-range key trails the picked one by more than LEAD_MIN binary orders, in every (b, head) and row."""
        c = float(np.float32(SCALE) * np.float32(1.4426950408889634))
        worst_dot, self.lead = 0.0, math.inf
        for b in range(self.B):
            for h in range(self.H):
                dots = s[b, h][pos[b, h]] @ s[b, h].T                     # [Lq, n], exact small integers
                dots[np.arange(self.Lq), pos[b, h]] = 0.0
                worst_dot = max(worst_dot, float(np.abs(dots).max()))
                self.lead = min(self.lead, float((c * AMP * (D - dots.max(-1))).min()))
        self.worst_dot = worst_dot
        assert worst_dot < DOT_MAX and self.lead > LEAD_MIN, (self, worst_dot, self.lead)

    def __repr__(self):
        return f"Picked({case_id((self.B, self.Lq, self.H, self.ranges))}, {self.fmt})"

    @classmethod
    def get(cls, geom, fmt):
        key = (case_id(geom), fmt)
        if key not in cls._cache:
            cls._cache[key] = cls(*geom, fmt)
        return cls._cache[key]

    def segs_args(self):
        """seg0_start, seg0_len, seg1_start, seg1_len as the case lists them (adjacent ranges unmerged)."""
        (s0, n0), (s1, n1) = self.ranges[0], (self.ranges[1] if len(self.ranges) > 1 else (0, 0))
        return s0, n0, s1, n1

    def segments(self):
        """[(start, end)] as ops.* take them."""
        return [(s, s + n) for s, n in self.ranges]

    def tensors(self, device="cpu"):
        """q, k, v as bf16 tensors."""
        return tuple(torch.from_numpy(a.view(np.int16).copy()).view(torch.bfloat16).to(device) for a in (self.q, self.k, self.v))
