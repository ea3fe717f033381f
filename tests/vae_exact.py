"""Data constructions of the VAE-decoder / umT5 edge suite and their fp64 host references (plain helpers, no tests; the conventions
of tests/bf16_exact.py).

Convolution: integer codes -4 .. 4 in the input, integer codes -4 .. 4 under one power of two per output channel in the weights, bias
and residual on the 2^-3 grid.  K <= 27 x 384 = 10368, so |any partial sum of code products| <= 16 K < 2^24: every fp32 sum is exact
in ANY order -- (tap, channel) of conv_cl_kernel and (kt, slice, kh, kw) of conv_halo_kernel alike -- and the output has one correct
bit pattern: the fp64 convolution + bias rounded to bf16 once, and with a residual bf16(res + that) (the kernel's two rounding
points).  The expected tensor is F.conv3d in fp64 on the padded / upsampled input, never a kernel's output.

Row softmax: SOFTMAX_BOUND_ULP below.  umT5 attention: the position and mask constructions of T5Case.
Everything a test compares against comes from here; mutations (tests/test_vae_edges_host.py) are applied to these references only."""
import math

import torch
import torch.nn.functional as F

from bf16_exact import NAN16, ulp_bf16  # noqa: F401  (re-exported: the sentinel pattern and the ulp of the attention bound)

bf = torch.bfloat16
K_MAX = 27 * 384

# Generic rows of ll_softmax_rows, in bf16 ulp of the fp64 softmax rounded once: torch's own fp32 softmax rounded to bf16 is at most
# 1 ulp away from it (measured in tests/test_vae_edges_host.py over every (N, ld, scale) of SOFTMAX_SHAPES with 256 rows up to
# N = 128, 60 at N = 1000 and 9 at N = 6240: 1 ulp on 3 of 32768 elements at N = 128, 0 everywhere else -- an fp32 value next to a
# bf16 rounding boundary), plus one ulp for the kernel's exp2-based evaluation (v_exp_f32 of x log2(e) - max log2(e): a relative
# 2^-22 or so on the fp32 value, which can cross the same boundaries).
SOFTMAX_REF_ULP = 1
SOFTMAX_BOUND_ULP = SOFTMAX_REF_ULP + 1
SOFTMAX_SHAPES = [(1, 8, 1.0), (7, 8, 0.3), (8, 8, 0.05), (96, 96, 0.3), (96, 128, 1.0), (128, 128, 0.102), (1000, 1000, 0.05),
                  (6233, 6240, 0.0510), (6240, 6240, 0.0510)]      # (N, ld, scale); 0.051 = 384^-0.5, the decoder's


def hash_bits(idx, seed):
    """The 32-bit integer hash of tests/bf16_exact.py."""
    x = (idx * 2654435761 + seed) & 0xFFFFFFFF
    x = x ^ (x >> 15)
    x = (x * 2246822519) & 0xFFFFFFFF
    x = x ^ (x >> 13)
    x = (x * 3266489917) & 0xFFFFFFFF
    return x ^ (x >> 16)


def _codes(shape, seed, lo=-4, hi=4):
    n = 1
    for s in shape:
        n *= s
    b = hash_bits(torch.arange(n, dtype=torch.int64), seed)
    return ((b >> 9) % (hi - lo + 1) + lo).double().view(*shape)


# ---- convolution ----------------------------------------------------------------------------------------------------------------------
class ConvData:
    """One convolution on exact data.
    frames [nh + T, H, W, Cin] (float64, bf16-exact): nh = 2 history frames when KT == 3 (non-zero and distinct from the new frames, or
    zeros with hist='zero'), then the T new frames.  w [Cout, Cin, KT, KH, KH] = codes 2^ew[co]; channel 0 of every tap carries the
    tap's own code and channel 1 the temporal tap's, channel 32 s + 2 the slice's code: no tap equals its mirror, no slice its neighbour.
    bias = codes -8 .. 8 on the 2^-3 grid (zero with zero_bias), res [T, Ho, Wo, Cout] = codes -40 .. 40 on it.
    impulse=(t, h, w): the new frames are zero but for that pixel; history zero.   zero_box=(h0, h1, w0, w1): the input of every frame
    is zero there (with zero_bias the output pixels whose whole stencil lies inside are zero in every channel).
    shift: everything the output is linear in (weights, bias, residual) is multiplied by 2^shift: the same bits, another exponent."""

    def __init__(self, T, H, W, Cin, Cout, KT, KH, up=False, seed=1, hist="nonzero", impulse=None, zero_box=None, zero_bias=False,
                 shift=0):
        K = KT * KH * KH * Cin
        assert K <= K_MAX and 16 * K < 2 ** 24           # |any partial sum of code products| <= 16 K: exact in fp32 in any order
        assert not up or (KT == 1 and KH == 3)
        self.T, self.H, self.W, self.Cin, self.Cout, self.KT, self.KH, self.up, self.K = T, H, W, Cin, Cout, KT, KH, bool(up), K
        self.Ho, self.Wo = (2 * H, 2 * W) if up else (H, W)
        self.M = T * self.Ho * self.Wo
        self.nh = nh = 2 if KT == 3 else 0
        self.Kpad = (K + 63) // 64 * 64
        fr = _codes((nh + T, H, W, Cin), seed)
        if nh:
            fr[:2] = _codes((2, H, W, Cin), seed + 101)
            fr[0, :, :, 0], fr[1, :, :, 0] = 3.0, -3.0                        # non-zero and told apart from each other
            if hist == "zero":
                fr[:2] = 0.0
        if impulse is not None:
            t, h, w = impulse
            px = ((torch.arange(Cin) * 5) % 9 - 4).double()
            px[px == 0] = 1.0
            fr.zero_()
            fr[nh + t, h, w] = px
        if zero_box is not None:
            h0, h1, w0, w1 = zero_box
            fr[:, h0:h1, w0:w1] = 0.0
        cw = _codes((Cout, Cin, KT, KH, KH), seed + 7)
        tap = torch.arange(KT * KH * KH).view(KT, KH, KH)
        cw[:, 0] = ((tap % 9) - 4).double()
        cw[:, 1] = (tap // 9 - 1).double() + (tap % 2).double() * (0 if KT == 3 else 1)
        for s in range(Cin // 32):
            cw[:, 32 * s + 2] = float(s % 9 - 4)
        ew = ((torch.arange(Cout) * 5) % 7 - 3).double()
        w = cw * torch.pow(2.0, ew + shift).view(-1, 1, 1, 1, 1)
        cb = _codes((Cout,), seed + 13, -8, 8)
        bias = torch.zeros(Cout, dtype=torch.float64) if zero_bias else cb * 2.0 ** (shift - 3)
        res = _codes((T, self.Ho, self.Wo, Cout), seed + 17, -40, 40) * 2.0 ** (shift - 3)
        if zero_box is not None:
            res[:, (h0 << up):(h1 << up), (w0 << up):(w1 << up)] = 0.0
        for t in (fr, w, bias, res):
            assert torch.equal(t.to(bf).double(), t)                          # bf16-exact operands
        if nh and hist != "zero" and impulse is None and zero_box is None:
            assert not torch.equal(fr[0], fr[1]) and all(not torch.equal(fr[i], fr[j]) for i in (0, 1) for j in range(2, 2 + T))
        if impulse is None:
            for a in range(KH):
                for b in range(KH):
                    if (a, b) != (KH - 1 - a, KH - 1 - b):
                        assert not torch.equal(w[..., a, b], w[..., KH - 1 - a, KH - 1 - b])
            assert all(not torch.equal(w[:, 32 * s:32 * s + 32], w[:, 32 * s + 32:32 * s + 64]) for s in range(Cin // 32 - 1))
        self.frames, self.w, self.bias, self.res, self.shift = fr, w, bias, res, shift
        self.acc = conv_host(fr, w, KT, KH, up)                                # [T, Ho, Wo, Cout] fp64, exact
        # acc, bias and res are multiples of g = 2^(shift - 3): acc + bias and res + bf16(acc + bias) are exact in fp32 below 2^24 g,
        # so each of the kernel's two fp32 sums rounded to bf16 is the fp64 sum rounded once
        g = 2.0 ** (shift - 3)
        assert (self.acc.abs().max() + bias.abs().max()) < 2 ** 24 * g
        raw = self.acc + bias
        assert torch.equal(raw.float().double(), raw)
        self.want = raw.float().to(bf)
        s2 = res + self.want.double()
        assert s2.abs().max() < 2 ** 24 * g and torch.equal(s2.float().double(), s2)
        self.want_res = s2.float().to(bf)

    def packed_w(self):
        """[Cout, Kpad] bf16 with k = ((kt KH + kh) KH + kw) Cin + ci, zero padded (ops.pack_conv_weight's layout)."""
        p = torch.zeros(self.Cout, self.Kpad, dtype=bf)
        p[:, :self.K] = self.w.permute(0, 2, 3, 4, 1).reshape(self.Cout, self.K).to(bf)
        return p


def conv_input(frames, KH, up, replicate_left=False, flip_row=None):
    """[1, Cin, F, Hp, Wp] fp64: the (upsampled) frames with their spatial zero padding.  The mutations of the host proof:
    replicate_left -- the left border column is the edge pixel instead of zero; flip_row -- upsampled row r reads source row
    (r >> 1) ^ 1 (the row above where that lies below the frame) instead of r >> 1."""
    x = frames.permute(3, 0, 1, 2)[None]
    if up:
        idx = torch.arange(2 * frames.shape[1]) >> 1
        if flip_row is not None:
            src = int(idx[flip_row]) ^ 1
            idx[flip_row] = src if src < frames.shape[1] else src - 2
        x = x[:, :, :, idx].repeat_interleave(2, dim=4)
    p = KH // 2
    x = F.pad(x, (p, p, p, p, 0, 0))
    if replicate_left and p:
        x[..., 0] = x[..., 1]
    return x


def conv_host(frames, w, KT, KH, up, **mut):
    """fp64 convolution, channels-last result [T, Ho, Wo, Cout]: frame t of the output reads frames t .. t + KT - 1 of `frames`."""
    y = F.conv3d(conv_input(frames, KH, up, **mut), w)
    return y[0].permute(1, 2, 3, 0).contiguous()


def conv_pixel_host(frames, w, KT, KH, up, t, h, x, shift_tap=None):
    """One output pixel [Cout] in fp64 from its taps; shift_tap=(kt, kh, kw): that tap reads the pixel one to the right of its own."""
    xin = conv_input(frames, KH, up)[0]                                        # [Cin, F, Hp, Wp]
    out = torch.zeros(w.shape[0], dtype=torch.float64)
    for kt in range(KT):
        for kh in range(KH):
            for kw in range(KH):
                d = 1 if shift_tap == (kt, kh, kw) else 0
                col = min(x + kw + d, xin.shape[3] - 1)
                out += w[:, :, kt, kh, kw] @ xin[:, t + kt, h + kh, col]
    return out


def rms_silu_host(raw, gamma, silu):
    """The reference's rounding-point chain on bf16 rows [P, C]: oracle.ref_vae.rms_norm (F.normalize x sqrt(C) x gamma in bf16), SiLU."""
    from oracle import ref_vae as RV
    C = raw.shape[-1]
    y = RV.rms_norm(raw.t()[None, :, None, :, None].contiguous(), gamma.view(C, 1, 1, 1))
    if silu:
        y = F.silu(y)
    return y[0, :, 0, :, 0].t().contiguous()


def rows_norm(raw):
    """fp64 L2 norm of bf16 rows [P, C]."""
    return raw.double().pow(2).sum(-1).sqrt()


# ---- row softmax ----------------------------------------------------------------------------------------------------------------------
def softmax_rows_data(rows, N, ld, seed):
    """s [rows, ld] bf16: values in [-8, 8] on a grid of 0.008 (rounded to bf16), in the padding columns too (they must not leak)."""
    b = hash_bits(torch.arange(rows * ld, dtype=torch.int64), seed)
    s = (((b >> 8) % 2001).double() / 1000.0 - 1.0) * 8.0
    return s.view(rows, ld).to(bf)


def softmax_host(s, N, scale):
    """fp64 softmax(scale s[:, :N]) rounded to bf16 once, zeros in the columns from N on."""
    out = torch.zeros_like(s)
    out[:, :N] = torch.softmax(s[:, :N].double() * float(torch.tensor(scale, dtype=torch.float32)), -1).to(bf)
    return out


def softmax_torch32(s, N, scale):
    out = torch.zeros_like(s)
    out[:, :N] = torch.softmax(s[:, :N].float() * scale, -1).to(bf)
    return out


# ---- umT5 attention -------------------------------------------------------------------------------------------------------------------
T5_BIG = 40.0                      # the one non-zero entry of a head's bias table: e^-40 = 2^-57.7 is what every other key weighs
T5_V_OUT = -100.0                  # every channel of a V row from seq_len on
T5_MARK = 64.0                     # marker on key seq_len - 1 (channel 63)
T5_BOUND_ULP = 2                   # P rounded to bf16 once, the output once (the reasoning of bf16_exact.ATTN_BOUND_ULP); the oracle's
#                                    own path (oracle.ref_t5.attention) measures <= 1.25 ulp on every geometry (test_vae_edges_host.py)
T5_OFFSETS = lambda L: [-(L - 1), -1, 0, 1, L - 1, None, -17, 16, 31, -32]      # None: an all-zero table (the mask construction)


class T5Case:
    """q = 0, so a score is the bias alone.  Head h's table holds T5_BIG at relative offset d_h = offsets[(h + rot) % len] and zeros
    elsewhere (None: zeros everywhere).  Query i of head h then returns V[i + d_h] where 0 <= i + d_h < seq_len (position construction:
    pins bias_tab[key - query + L - 1] per offset class and the mask edge), else -- no key, a masked key, or no offset -- the mean of V
    over exactly the first seq_len keys (mask construction).  V: non-zero integers -4 .. 4 per (key, head, channel), channel 63 zero but
    for T5_MARK on key seq_len - 1, every row from seq_len on T5_V_OUT."""

    def __init__(self, L, H, seq_len, rot=0, heads=None):
        self.L, self.H, self.n, self.rot = L, H, seq_len, rot
        self.heads = list(range(H)) if heads is None else heads              # the host module evaluates a slice of a 64-head case
        offs = T5_OFFSETS(L)
        self.d = [offs[(h + rot) % len(offs)] for h in range(H)]

    def table(self):
        """[H, 2L - 1] float64."""
        t = torch.zeros(self.H, 2 * self.L - 1, dtype=torch.float64)
        for h, d in enumerate(self.d):
            if d is not None:
                assert abs(d) <= self.L - 1
                t[h, d + self.L - 1] = T5_BIG
        return t

    def v(self):
        """[L, H, 64] float64."""
        L, H = self.L, self.H
        idx = (torch.arange(L).view(-1, 1, 1) * H + torch.arange(H).view(1, -1, 1)) * 64 + torch.arange(64).view(1, 1, -1)
        b = hash_bits(idx.to(torch.int64), 4242)
        v = ((b >> 5) % 4 + 1).double() * (((b >> 11) & 1).double() * 2 - 1)
        v[:, :, 63] = 0.0
        v[self.n - 1, :, 63] = T5_MARK
        v[self.n:] = T5_V_OUT
        return v

    def k(self):
        """[L, H, 64]: arbitrary bf16-exact integers (q = 0 makes them irrelevant; a kernel that did not take q from its argument shows)."""
        L, H = self.L, self.H
        b = hash_bits(torch.arange(L * H * 64, dtype=torch.int64), 99)
        return ((b >> 7) % 17 - 8).double().view(L, H, 64)

    def expected(self, seq_len=None, shift=0):
        """[L, H, 64] float64 from the construction; seq_len / shift: the MUTATIONS of the host proof (one key more or fewer admitted, the
        bias offset moved by one) -- the data stays that of the case."""
        n = self.n if seq_len is None else seq_len
        v = self.v()
        mean = v[:n].mean(0)
        out = mean.unsqueeze(0).repeat(self.L, 1, 1)
        for h, d in enumerate(self.d):
            if d is None:
                continue
            i = torch.arange(self.L)
            j = i + d - shift                                                  # the table read one entry further on
            ok = (j >= 0) & (j < n)
            out[i[ok], h] = v[j[ok], h]
        return out

    def bound(self, expected):
        """T5_BOUND_ULP ulp of the expected element; at expected zeros a floor: all other keys together, L e^-40 x the largest |V|
        (T5_V_OUT cannot enter: masked keys weigh exactly 0)."""
        return torch.where(expected != 0, T5_BOUND_ULP * ulp_bf16(expected), torch.full_like(expected, self.L * math.exp(-T5_BIG) * T5_MARK))

    def host(self, seq_len=None, shift=0):
        """fp64 evaluation of T5Attention's core on the case's tensors: softmax(bias, keys >= seq_len excluded) v; mutations as above."""
        n = self.n if seq_len is None else seq_len
        L = self.L
        tab, v = self.table(), self.v()
        tab = F.pad(tab, (1, 1))                                               # a shifted read past either end finds zero
        idx = torch.arange(L)[None, :] - torch.arange(L)[:, None] + L - 1 + shift + 1
        out = torch.zeros(L, self.H, 64, dtype=torch.float64)
        for h in self.heads:
            p = torch.softmax(tab[h][idx][:, :n], -1)
            out[:, h] = p @ v[:n, h]
        return out

    def oracle(self):
        """oracle.ref_t5.attention itself on the case (bf16): x = V, identity value / output projections, zero query / key projections."""
        from oracle import ref_t5 as RT
        hs = self.heads
        C = len(hs) * 64
        x = self.v()[:, hs].reshape(1, self.L, C).to(bf)
        eye, zero = torch.eye(C, dtype=bf), torch.zeros(C, C, dtype=bf)
        sd = {"q.weight": zero, "k.weight": zero, "v.weight": eye, "o.weight": eye}
        idx = torch.arange(self.L)[None, :] - torch.arange(self.L)[:, None] + self.L - 1
        pos = self.table()[hs][:, idx].to(bf)[None]                            # [1, h, Lq, Lk]
        mask = torch.zeros(1, self.L, dtype=torch.long)
        mask[:, :self.n] = 1
        y = RT.attention(x, sd, "", len(hs), mask, pos)
        out = torch.zeros(self.L, self.H, 64, dtype=torch.float64)
        out[:, hs] = y[0].double().view(self.L, len(hs), 64)
        return out


def t5_seq_lens(L):
    return sorted({n for n in (1, 15, 16, 17, 63, 64, 65, L - 1, L) if 1 <= n <= L})


# (L, H, seq_len, rot) of every attention case of tests/test_t5_edges_gpu.py: every L x every seq_len at H = 1 and 3 (rot walks the
# offset classes through the heads), 64 heads at the ends
T5_CASES = [(L, H, n, (i + H) % 10) for L in (64, 128, 256, 512) for H in (1, 3) for i, n in enumerate(t5_seq_lens(L))]
T5_CASES += [(L, 1, L, r) for L in (64, 128, 256, 512) for r in range(5) if (L, 1, L, r) not in T5_CASES]   # every required offset unmasked
T5_CASES += [(64, 64, 17, 0), (128, 64, 127, 3), (512, 64, 511, 5), (512, 64, 512, 0), (512, 64, 1, 7)]
