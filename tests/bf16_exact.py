"""Data constructions of the bf16 edge suite and their host references (plain helpers, no tests).

GEMM: small-integer codes under a distinct power of two per activation row / output channel.  Both operands are exact in bf16, every
product is exact and every fp32 partial sum is exact in ANY order (|sum of codes| <= 16 K < 2^24), so the bf16 output has one correct
bit pattern: the fp64 product + bias rounded once.

Attention: two constructions in one set of tensors, told apart per query row.
  gather   q_r = a u_pi(r), k_j = a u_j with +-1 sign codes u of length 128: the target key leads every other key of the row by more
           than 30 binary orders, so the output row is V[pi(r)] -- a vector of integers.  Targets sit on the boundary slots of the key
           ranges and of the 64-key tiles.  Every slot OUTSIDE the ranges carries some target's code at 1.5 x the amplitude and a V row
           of -100: admitted by mistake it wins the softmax of the rows that aim at that target.
  uniform  q_r = 0: every in-range key weighs 1 / n, the output is the mean of V over exactly the range's keys.  V has a constant
           channel, integer channels and +64 markers on the range-boundary slots (the slots just outside hold -100 on every channel).
Both are bf16-exact inputs; the expected outputs come from the construction, not from a kernel."""
import math

import torch

bf = torch.bfloat16
NAN16 = 0x7FC1                     # a bf16 quiet-NaN bit pattern: padding and sentinel rows
KT = 64                            # keys per tile of every bf16 attention kernel
LEAD_MIN = 30                      # binary orders the target key leads by (asserted per case on the host)
V_OUT = -100.0                     # every channel of a V row outside the key ranges
MARK = 64.0                        # marker on the range-boundary slots
CONST = 3.0                        # channel 0 of every in-range V row
# The tolerance of the attention checks, in bf16 ulp of the expected element: the larger of 2 (P rounded to bf16 once, the output
# once: a relative 2^-8 each) and the distance of the oracle's own bf16 path (oracle.ref_ops.attention) from the expected values,
# which tests/test_bf16_edges_host.py measures for every geometry and holds below this.
ATTN_BOUND_ULP = 2


# ---- GEMM ---------------------------------------------------------------------------------------------------------------------------
class GemmData:
    """X [M, K] = cx 2^ex[row], W [N, K] = cw 2^ew[channel] (codes -4 .. 4, W's first column asymmetric), bias = cb 2^-3; `unit`: codes
    -2 .. 2 (-1 .. 1 above K = 320) under scale 1 and an integer bias, so the outputs are small integers.  acc = the exact fp64 product.
    `o1`: the powers of two are chosen so that the outputs are O(1) (row sums of standard deviation 1/16 .. 1), for the GELU cases:
    torch's tanh-GELU, the reference of that check, evaluates 0.5 x (1 + tanh u) in fp32, which cancels for x << 0 -- on the wide
    scales of the default set 5 % of the outputs lie in -9 < x < -3, where 69 % of torch's own bf16 results differ from the fp64
    value (0.9 % elsewhere; measured on 300 x 448 x 320), so the reference itself would miss the 97 % it is held to."""

    def __init__(self, M, N, K, seed, unit=False, o1=False):
        assert K <= 8960 and 16 * K < 2 ** 24          # |any partial sum of codes| <= 16 K: exact in fp32 in any order
        self.M, self.N, self.K = M, N, K
        g = torch.Generator().manual_seed(seed)
        c = (2 if K <= 320 else 1) if unit else 4      # unit: |outputs| stay below 362 (asserted below) up to K = 8960
        cx = torch.randint(-c, c + 1, (M, K), generator=g).double()
        cw = torch.randint(-c, c + 1, (N, K), generator=g).double()
        cw[:, 0] = (torch.arange(N) % 3).double()                        # W is not X's pattern transposed
        ex = torch.zeros(M) if unit else ((torch.arange(M) * 3) % 7 - 3).double()
        ew = torch.zeros(N) if unit else ((torch.arange(N) * 5) % 7 - 3).double()
        grid = 2.0 ** -6                                                   # acc and bias are multiples of this
        if o1:
            sh = -round(math.log2(60 / 9 * math.sqrt(K)))                  # codes -4 .. 4 have variance 60 / 9
            ex, ew = -(torch.arange(M) % 3).double(), sh - ((torch.arange(N) * 2) % 3).double()
            grid = 2.0 ** (sh - 4)
        x = cx * torch.pow(2.0, ex).double().unsqueeze(1)
        w = cw * torch.pow(2.0, ew).double().unsqueeze(1)
        cb = torch.randint(-8, 9, (N,), generator=g).double()
        bias = cb if unit else cb * 2.0 ** -3
        self.x, self.w, self.bias = x.to(bf), w.to(bf), bias.to(bf)
        assert torch.equal(self.x.double(), x) and torch.equal(self.w.double(), w) and torch.equal(self.bias.double(), bias)
        self.acc = x @ w.t()
        # acc and bias are multiples of `grid` (2^-6): acc + bias is exact in fp32 (24 bits) below 2^24 grid (2^18), so
        # fp32(acc + bias) rounded to bf16 is the fp64 sum rounded once
        assert (self.acc.abs() + bias.abs()).max() < 2 ** 24 * grid
        self.want = (self.acc + bias).to(bf)
        if unit:
            assert self.want.float().abs().max() ** 2 * 128 < 2 ** 24      # a plane's sum of squares: integers, exact in fp32

    def ssq(self, M):
        """[N / 128, M] fp32: per 128-column plane the sum of squares of the bf16 outputs of the first M rows (exact for `unit`)."""
        return self.want[:M].double().pow(2).view(M, self.N // 128, 128).sum(-1).t().contiguous().float()


# ---- attention ------------------------------------------------------------------------------------------------------------------------
def _hash_bits(idx, seed):
    """A 32-bit integer hash of int64 indices in torch (the same integers on the host and on the device)."""
    x = (idx * 2654435761 + seed) & 0xFFFFFFFF
    x = x ^ (x >> 15)
    x = (x * 2246822519) & 0xFFFFFFFF
    x = x ^ (x >> 13)
    x = (x * 3266489917) & 0xFFFFFFFF
    return x ^ (x >> 16)


class AttnCase:
    """One geometry: ranges = [(start, len)] (one or two), in the order the kernel walks them."""

    def __init__(self, B, Lq, H, ranges, a_q=2.0, a_k=2.0, seed=1):
        self.B, self.Lq, self.H, self.ranges, self.a_q, self.a_k, self.seed = B, Lq, H, [tuple(r) for r in ranges], a_q, a_k, seed
        self.end = max(s + n for s, n in self.ranges)
        self.Sk = self.end + KT                          # the remainder of a ragged last tile and a tile beyond: all outside slots
        inr = []
        for s, n in self.ranges:
            inr += list(range(s, s + n))
        assert len(set(inr)) == len(inr)
        self.inr = inr
        self.nkeys = len(inr)
        inset = set(inr)
        self.outside = [j for j in range(self.Sk) if j not in inset]
        # range-boundary slots (marked in V): first and last slot of each range, first slot of each ragged tail tile
        rb = []
        for s, n in self.ranges:
            rb += [s + n - 1, s, s + (n - 1) // KT * KT]
        self.range_bounds = list(dict.fromkeys(rb))
        # targets: the range boundaries, then the tile seams (last slot of a tile, first of the next) from the end of the walk backwards
        t = list(self.range_bounds)
        for s, n in reversed(self.ranges):
            for e in range((n - 1) // KT * KT, 0, -KT):
                t += [s + e, s + e - 1]
        self.targets = list(dict.fromkeys(t))
        # outside slots, nearest to the ranges first: end, start - 1, the gap, the rest of the last tile, ...
        near = []
        for s, n in reversed(self.ranges):
            near += [s + n, s - 1]
        near = [j for j in near if 0 <= j < self.Sk and j not in inset]
        self.outside = list(dict.fromkeys(near + self.outside))
        self.poison_target = {o: self.targets[i % len(self.targets)] for i, o in enumerate(self.outside)}

    def row_plan(self, phase):
        """(is_uniform [Lq] bool, target slot [Lq]): rows with (r + phase) % 4 == 0 are uniform rows; the g-th gather row aims at
        targets[g % len(targets)]."""
        r = torch.arange(self.Lq)
        uni = (r + phase) % 4 == 0
        g = torch.cumsum((~uni).long(), 0) - 1
        tg = torch.tensor(self.targets)[g.clamp_min(0) % len(self.targets)]
        return uni, tg

    def codes(self, slots, device):
        """+-1 sign codes [len(slots), H, 128] of key slots (shared by the batch elements)."""
        s = torch.as_tensor(slots, dtype=torch.int64, device=device).view(-1, 1, 1)
        h = torch.arange(self.H, dtype=torch.int64, device=device).view(1, -1, 1)
        c = torch.arange(128, dtype=torch.int64, device=device).view(1, 1, -1)
        bits = _hash_bits((s * self.H + h) * 128 + c, self.seed)
        return ((bits >> 7) & 1).double() * 2 - 1

    def build(self, phase, device="cpu"):
        """q [B, Lq, H, 128], k / v [B, Sk, H, 128] (bf16-exact values as float64) and the expected output [B, Lq, H, 128] (float64).
        Batch element b's V rows are rotated by b channels, so a kernel that reads the wrong batch element shows."""
        B, Lq, H, Sk = self.B, self.Lq, self.H, self.Sk
        uni, tg = self.row_plan(phase)
        uni, tg = uni.to(device), tg.to(device)
        u = self.codes(range(Sk), device)                                     # [Sk, H, 128]
        k = self.a_k * u
        out_idx = torch.tensor(self.outside, device=device)
        pt = torch.tensor([self.poison_target[o] for o in self.outside], device=device)
        k[out_idx] = 1.5 * self.a_k * u[pt]
        q = self.a_q * u[tg]
        q[uni] = 0.0
        # V: channel 0 constant, channels 1 .. 63 non-zero integers in -4 .. 4 distinct per slot and head, channels 64 .. 127 zero but
        # for one +64 marker per range-boundary slot
        s = torch.arange(Sk, dtype=torch.int64, device=device).view(-1, 1, 1)
        h = torch.arange(H, dtype=torch.int64, device=device).view(1, -1, 1)
        c = torch.arange(128, dtype=torch.int64, device=device).view(1, 1, -1)
        bits = _hash_bits((s * H + h) * 128 + c, self.seed + 77)
        mag = ((bits >> 5) % 4 + 1).double() * (((bits >> 11) & 1).double() * 2 - 1)
        v = torch.where(c < 64, mag, torch.zeros_like(mag))
        v[:, :, 0] = CONST
        for i, j in enumerate(self.range_bounds):
            v[j, :, 64 + i] = MARK
        v[out_idx] = V_OUT
        qs, ks, vs, es = [], [], [], []
        inr = torch.tensor(self.inr, device=device)
        for b in range(B):
            vb = torch.roll(v, b, dims=2) if b else v
            exp = vb[tg]                                                       # gather rows: V[pi(r)]
            exp = torch.where(uni.view(-1, 1, 1), vb[inr].mean(0, keepdim=True).expand(Lq, H, 128), exp)
            qs.append(q), ks.append(k), vs.append(vb), es.append(exp)
        return torch.stack(qs), torch.stack(ks), torch.stack(vs), torch.stack(es)

    def q_raw_and_ssq(self, q):
        """For the q-norm kernel: q as built is the RAW projection (amplitude a_q); WanRMSNorm with a unit weight turns a gather row into
        its +-1 code exactly (every |x| equal: x * rsqrt(mean x^2 + eps) rounds to +-1 in bf16) and leaves a zero row zero.  Returns
        ssq [H, B * Lq] fp32 (per-head plane sums of squares) and the normalised q."""
        B, Lq, H, _ = q.shape
        ssq = q.double().pow(2).sum(-1).view(B * Lq, H).t().contiguous().float()
        rinv = torch.rsqrt(ssq.double().sum(0) / (H * 128) + 1e-6).float().view(B, Lq, 1, 1)
        qn = (q.float() * rinv).to(bf).double()
        return ssq, qn


def ulp_bf16(x):
    """The bf16 unit in the last place at |x| (float64 tensor; 0 at 0)."""
    ax = x.abs()
    e = torch.floor(torch.log2(ax.clamp_min(2.0 ** -126)))
    return torch.where(ax > 0, torch.pow(2.0, e - 7), torch.zeros_like(ax))


def attn_bound(expected, nkeys, bound_ulp=ATTN_BOUND_ULP):
    """Per element: bound_ulp bf16 ulp of the expected value; where the expected value is zero (ulp distance means nothing there) an
    absolute floor: the weight of all non-target keys together, nkeys 2^-LEAD_MIN, times the largest |V| a range holds (MARK)."""
    return torch.where(expected != 0, bound_ulp * ulp_bf16(expected), torch.full_like(expected, nkeys * 2.0 ** -LEAD_MIN * MARK))


def attn_host(q, k, v, slots, scale=1.0 / math.sqrt(128)):
    """fp64 softmax(q k^T scale) v over the key slots `slots` for one head: q [R, 128], k / v [Sk, 128] -> [R, 128]."""
    idx = torch.as_tensor(slots)
    s = (q @ k[idx].t()) * scale
    return torch.softmax(s, -1) @ v[idx]


def attn_lead(q, k, slots, scale=1.0 / math.sqrt(128)):
    """Binary orders by which each row's best key leads its second best (gather rows only make sense here)."""
    idx = torch.as_tensor(slots)
    s = (q @ k[idx].t()) * scale * 1.4426950408889634
    top = torch.topk(s, min(2, s.shape[1]), dim=1).values
    return top[:, 0] - top[:, 1] if top.shape[1] > 1 else torch.full((s.shape[0],), float("inf"), dtype=s.dtype)


# (name, B, Lq, H, ranges) of every attention geometry of tests/test_bf16_edges_gpu.py, grouped by the kernel they run on; the host
# module checks each of them.  Lq in {1, 31, 32, 33, 64, 127, 128, 129, 255, 256, 257, 328}, H in {1, 3, 12}, B in {1, 2}, range
# starts {0, 1, 37, 63, 64, 65}, lengths {1, 7, 63, 64, 65, 127, 128, 129, 511, 512, 513, 1023, 1024, 1025, 1437}.
PIPE0_CASES = [      # flash_attn_pipe_kernel<8, 0>: one range below attn_pp_min_keys (attn_asm 0 from 128 keys on)
    (1, 1, 1, [(0, 1)]), (1, 31, 1, [(1, 7)]), (1, 32, 3, [(37, 63)]), (2, 33, 1, [(63, 64)]), (1, 64, 1, [(64, 65)]),
    (1, 127, 3, [(65, 127)]), (1, 128, 1, [(0, 128)]), (2, 129, 3, [(1, 129)]), (1, 255, 1, [(37, 511)]), (1, 256, 12, [(63, 512)]),
    (1, 257, 1, [(64, 513)]), (1, 328, 3, [(65, 1023)]),
]
PIPE1_CASES = [      # flash_attn_pipe_kernel<8, 1>: attn_asm 0, >= 1024 keys
    (1, 1, 1, [(0, 1024)]), (1, 31, 3, [(1, 1025)]), (1, 32, 1, [(64, 1024)]), (2, 33, 1, [(37, 1437)]), (1, 64, 1, [(63, 1024)]),
    (2, 127, 1, [(65, 1025)]), (1, 128, 3, [(1, 1437)]), (1, 129, 12, [(64, 1025)]), (1, 255, 12, [(63, 1025)]), (1, 256, 1, [(65, 1437)]),
    (2, 257, 3, [(0, 1025)]), (1, 328, 3, [(37, 1024)]),
]
ASM_CASES = [        # flash_attn_asm_kernel: attn_asm_min_keys lowered to its floor (two tiles = 128 keys)
    (1, 1, 1, [(0, 128)]), (1, 31, 1, [(1, 129)]), (1, 32, 3, [(37, 511)]), (2, 33, 1, [(63, 512)]), (1, 64, 1, [(64, 513)]),
    (1, 127, 3, [(65, 1023)]), (1, 128, 1, [(0, 1024)]), (2, 129, 3, [(1, 1025)]), (1, 255, 1, [(37, 1437)]), (1, 256, 12, [(63, 512)]),
    (1, 257, 1, [(64, 1437)]), (1, 328, 3, [(65, 129)]),
]
TWO_RANGE_CASES = [  # flash_attn_kernel<4>: two non-adjacent ranges (a one-slot gap, ragged first / second range), and one range
    (1, 1, 1, [(0, 64), (65, 64)]), (1, 31, 3, [(1, 7), (37, 63)]), (1, 32, 1, [(0, 512), (600, 64)]), (2, 33, 1, [(0, 65), (66, 129)]),
    (1, 64, 1, [(37, 127), (200, 128)]), (1, 127, 3, [(63, 1), (65, 511)]), (2, 128, 3, [(1, 1023), (1100, 128)]),
    (1, 129, 12, [(0, 64), (128, 65)]), (1, 255, 1, [(37, 1024), (1200, 65)]), (2, 256, 1, [(64, 513), (600, 7)]),
    (2, 256, 3, [(63, 64), (200, 512)]), (1, 257, 3, [(65, 129), (195, 1025)]), (1, 328, 1, [(1, 1437), (1500, 63)]),
    (2, 328, 12, [(64, 127), (300, 1023)]),
]
PLAIN_ONE_RANGE_CASES = [   # flash_attn_kernel<4> through attn_variant 0 on ONE range (adjacent ranges merge into this form)
    (1, 33, 1, [(37, 65)]), (2, 129, 3, [(0, 1025)]), (1, 328, 1, [(63, 7)]),
]
ADJACENT_CASES = [   # two ADJACENT ranges: merged into one (the plan says so); ragged first range, so the seam falls inside a tile
    (1, 129, 3, [(1, 65), (66, 511)]), (2, 257, 1, [(37, 100), (137, 1337)]),
]
PROD_CASES = [       # the production shapes, q / k / v generated on the device: one chunk over the full cache, and the recache forward
    (1, 4680, 12, [(0, 18720)]), (1, 18720, 12, [(0, 18720)]),
]
QNORM_CASES = [      # flash_attn_asm_qn_kernel: the gather through ll_flash_attn_qnorm (raw q of amplitude 2, keys of amplitude 4), every Lq
    # and start of the lists, every length from the kernel's two-tile floor on (attn_asm_min_keys lowered for those below 512)
    (1, 1, 1, [(0, 128)]), (1, 31, 1, [(0, 512)]), (1, 32, 3, [(63, 129)]), (2, 33, 1, [(64, 511)]), (1, 64, 1, [(65, 1023)]),
    (1, 127, 3, [(1, 1024)]), (1, 128, 1, [(37, 1025)]), (2, 129, 3, [(37, 513)]), (1, 255, 1, [(0, 129)]), (1, 256, 12, [(63, 512)]),
    (2, 257, 3, [(64, 128)]), (1, 328, 12, [(1, 1437)]),
]
ALL_SMALL_CASES = PIPE0_CASES + PIPE1_CASES + ASM_CASES + TWO_RANGE_CASES + PLAIN_ONE_RANGE_CASES + ADJACENT_CASES


# ---- plumbing of the edge suites that call the C entry points directly ------------------------------------------------------------------
def lib():
    from longlive_amd import _lib as L
    return L, L.load()


def run(fn, *args):
    """A C entry point with tensors as device pointers (None = NULL) and the current stream appended; a nonzero return raises."""
    from longlive_amd import ops as O
    L, l = lib()
    a = [t.data_ptr() if isinstance(t, torch.Tensor) else t for t in args]
    L.check(getattr(l, fn)(*a, O._stream()), fn)


def nan_bf16(*shape):
    return torch.full(shape, NAN16, dtype=torch.int16, device="cuda").view(torch.bfloat16)


def untouched_bf16(t):
    return bool((t.contiguous().view(torch.int16) == NAN16).all())
