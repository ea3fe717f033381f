"""MXFP8 self-attention, host side: the V-block scale rule across a write boundary, the lazy-max bound on P, the restatement against
fp64 attention, the shadow-refresh ranges of block_forward as a property over whole cache histories, argument validation and the
plan string of the new entry points (the library loads without a GPU), and the switches that reach the mode."""
import math

import pytest
import torch

import mx_attn_ref as MA
import mx_ref
from longlive_amd import _lib
from longlive_amd.kv_cache import plan_update, shadow_refresh_ranges
from oracle import ref_ops as R

bf = torch.bfloat16


def test_v_block_rule_straddles_a_write_boundary():
    """Slots 4672..4703 form one V^ block whatever was written where: its scale follows the block maximum across the boundary at
    4680 (old tokens small, new ones large), and the 32 codes sit in fragment order."""
    S, H = 9400, 2
    g = torch.Generator().manual_seed(0)
    v = (1e-3 * torch.randn(1, S, H, 128, generator=g)).to(bf)
    v[:, 4680:] = (40 * torch.randn(1, S - 4680, H, 128, generator=g)).to(bf)
    vq, vs = MA.shadow_v(v)
    j, h, d = 4672 // 32, 1, 77
    col = v[0, 32 * j: 32 * j + 32, h, d]
    q, s = mx_ref.quantize(col.reshape(1, 32))
    qo, so = mx_ref.quantize(v[0, 4640:4672, h, d].reshape(1, 32))
    assert int(vs[0, h, j, d]) == int(s[0, 0]) > int(so[0, 0]) + 10         # the large new values set the exponent
    for p in range(32):
        assert vq[0, h, j, d, p].view(torch.uint8) == q[0, MA.frag_slot(p)].view(torch.uint8)
    assert int(vs[0, h, 4640 // 32, d]) == int(so[0, 0])                   # the old-only block before it keeps its small exponent
    # padding slots past S read as zero: the last block of a 9400-slot cache holds 24 real slots
    last = v[0, 9376:9400, h, d].float()
    qp, sp = mx_ref.quantize(torch.cat([last, torch.zeros(8)]).to(bf).reshape(1, 32))
    assert int(vs[0, h, 9376 // 32, d]) == int(sp[0, 0])


def test_fragment_order_is_a_permutation_of_each_half():
    assert sorted(MA.frag_slot(p) for p in range(32)) == list(range(32))
    assert sorted(MA.frag_slot(p) for p in range(16)) == [s for s in range(32) if (s >> 2) & 1 == 0]


def test_lazy_max_keeps_p_below_e4m3_saturation():
    """Under THR = 8 every P = exp2(c s - M) is <= 2^8 (up to fp32 rounding) < 448, so e4m3fn(P) never saturates or overflows; also
    along score streams that grow tile by tile just under the threshold."""
    g = torch.Generator().manual_seed(1)
    c = 1.0 / math.sqrt(128) * MA.LOG2E
    worst = 0.0
    for trial in range(200):
        drift = torch.rand(1, generator=g).item() * 12
        M = -math.inf
        for t in range(40):
            s = torch.randn(64, generator=g) * 8 + drift * t / c * 0.1 * (trial % 3)
            tm = float((s.max() * c).float())
            M = tm if tm - M > MA.THR else M
            p = torch.exp2(s.float() * c - M)
            worst = max(worst, p.max().item())
            pq = p.to(MA.FP8).float()
            assert torch.isfinite(pq).all() and pq.max() <= 256.0
    assert 2.0 ** 7 < worst <= 2.0 ** 8 * (1 + 1e-6), worst


@pytest.mark.parametrize("segs", [[(0, 100), (164, 300)], [(0, 300)], [(37, 250)]])
def test_restatement_vs_fp64_attention(segs):
    g = torch.Generator().manual_seed(2)
    B, H, Lq, S = 1, 3, 40, 300
    q = torch.randn(B, Lq, H, 128, generator=g).to(bf)
    k = torch.randn(B, S, H, 128, generator=g).to(bf)
    v = torch.randn(B, S, H, 128, generator=g).to(bf)
    got = MA.mx_attention_cache(q, k, v, segs, dtype=torch.float64)
    ks = torch.cat([k[:, a:b] for a, b in segs], 1)
    vs = torch.cat([v[:, a:b] for a, b in segs], 1)
    exact = R.attention_exact(q, ks, vs)
    r = ((got - exact).norm() / exact.norm()).item()
    assert 1e-3 < r < 8e-2, r                    # quantised (e4m3: ~2^-4 per element), but attention all the same
    # fp32 accumulation (the kernel's) is the fp64 restatement up to summation order
    got32 = MA.mx_attention_cache(q, k, v, segs, dtype=torch.float32).double()
    assert ((got32 - got).norm() / got.norm()).item() < 1e-5


def test_tiles_start_at_range_starts_rounded_down_to_32():
    assert MA.tiles([(0, 4680), (4680, 18720)])[0] == (0, 0, 18720)          # adjacent ranges merge
    t = MA.tiles([(0, 4680), (6240, 18720)])
    assert t[73] == (4672, 0, 4680) and t[74] == (6240 & ~31, 6240, 18720)
    assert len(t) == 74 + math.ceil((18720 - 6240 // 32 * 32) / 64)


# ---- shadow refresh ranges: a brute-force property over cache histories ---------------------------------------------------------
class _HostLayer:
    """One layer's bf16 cache on the host, written as the model writes it (through `.data`, which bumps no version counter, like
    the C ABI writes), and a shadow refreshed only over shadow_refresh_ranges, exactly as block_forward does."""

    def __init__(self, S, H=1):
        self.k = torch.zeros(1, S, H, 128, dtype=bf)
        self.v = torch.zeros(1, S, H, 128, dtype=bf)
        self.S = S
        self.key = None
        self.sh = None
        self.g = torch.Generator().manual_seed(S)

    def key_now(self):
        from longlive_amd.model import mx_shadow_key
        return mx_shadow_key(self.k, self.v)

    def refresh(self, lo, hi):
        a, b = lo // 32 * 32, min(self.S, (hi + 31) // 32 * 32)
        kq, ks = MA.shadow_k(self.k)
        vq, vs = MA.shadow_v(self.v)
        self.sh["kq"][:, a:b] = kq[:, a:b]; self.sh["ks"][:, a:b] = ks[:, a:b]
        ja, jb = a // 32, (hi + 31) // 32
        self.sh["vq"][:, :, ja:jb] = vq[:, :, ja:jb]; self.sh["vs"][:, :, ja:jb] = vs[:, :, ja:jb]

    def forward(self, current_start, n, G, E, sink, local, max_attn, recache=False):
        stale = self.sh is None or self.key != self.key_now()
        if self.sh is None:
            kq, ks = MA.shadow_k(self.k)
            vq, vs = MA.shadow_v(self.v)
            self.sh = dict(kq=torch.full_like(kq, 3.0), ks=torch.full_like(ks, 9), vq=torch.full_like(vq, 3.0), vs=torch.full_like(vs, 9))
        plan = plan_update(current_start, n, G, E, self.S, sink, local, max_attn, recache)
        if plan.roll is not None:
            dst, src, m = plan.roll
            self.k.data[:, dst:dst + m] = self.k.data[:, src:src + m].clone()
            self.v.data[:, dst:dst + m] = self.v.data[:, src:src + m].clone()
        w0, wl = plan.write_start, plan.write_len
        self.k.data[:, w0:w0 + wl] = torch.randn(1, wl, *self.k.shape[2:], generator=self.g).to(bf)
        self.v.data[:, w0:w0 + wl] = torch.randn(1, wl, *self.v.shape[2:], generator=self.g).to(bf)
        for lo, hi in shadow_refresh_ranges(plan, stale, self.S):
            self.refresh(lo, hi)
        self.key = self.key_now()
        # every slot this attention reads: its K^ row and its whole V^ block are the bits of the current bf16 cache
        kq, ks = MA.shadow_k(self.k)
        vq, vs = MA.shadow_v(self.v)
        for a, b in plan.segments:
            assert torch.equal(self.sh["kq"][:, a:b].view(torch.uint8), kq[:, a:b].view(torch.uint8)), (a, b)
            assert torch.equal(self.sh["ks"][:, a:b], ks[:, a:b]), (a, b)
            ja, jb = a // 32, (b + 31) // 32
            assert torch.equal(self.sh["vq"][:, :, ja:jb].view(torch.uint8), vq[:, :, ja:jb].view(torch.uint8)), (a, b)
            assert torch.equal(self.sh["vs"][:, :, ja:jb], vs[:, :, ja:jb]), (a, b)
        return plan


@pytest.mark.parametrize("global_sink", [True, False])
@pytest.mark.parametrize("fs", [13, 40])
def test_shadow_refresh_ranges_keep_every_read_slot_current(fs, global_sink):
    """Fill, roll (unaligned evictions), a recompute of the last block at another timestep, an interactive prompt switch (indices
    kept; with global_sink=False the cache is zeroed in place outside the model and recached with sink_recache_after_switch), and
    more frames after it."""
    sink, local, nfb = 1, 4, 2                                         # frames
    S = local * fs
    L = _HostLayer(S)
    G = E = 0

    def fwd(start_frame, recache=False, commit=True):
        nonlocal G, E
        plan = L.forward(start_frame * fs, nfb * fs if not recache else 3 * fs, G, E, sink * fs, local, S, recache)
        if commit:
            G, E = plan.G_new, plan.E_new

    for blk in range(5):                                               # fill, then rolls
        fwd(blk * nfb, commit=False)                                   # a denoising step (no commit)
        fwd(blk * nfb)                                                 # the context pass
    fwd(4 * nfb)                                                       # recompute of the last block (current_end <= G)
    if not global_sink:
        L.k.zero_(); L.v.zero_()                                       # outside the model: version counters move
    plan_start = 5 * nfb - 3
    plan = L.forward(plan_start * fs, 3 * fs, G, E, sink * fs, local, S, not global_sink)
    G, E = plan.G_new, plan.E_new
    for blk in range(5, 8):
        fwd(blk * nfb)
    L.k.copy_(torch.randn(L.k.shape).to(bf))                           # another outside write (copy_) between two forwards
    fwd(8 * nfb)


def test_refresh_ranges_merge_roll_and_insert():
    plan = plan_update(12 * 4680, 4680, 12 * 4680, 18720, 18720, 4680, 12, 18720)
    assert plan.roll == (4680, 9360, 9360)
    assert shadow_refresh_ranges(plan, False, 18720) == [(4680, 18720)]
    assert shadow_refresh_ranges(plan, True, 18720) == [(0, 18720)]
    fill = plan_update(4680, 4680, 4680, 4680, 18720, 4680, 12, 18720)
    assert shadow_refresh_ranges(fill, False, 18720) == [(4680, 9360)]


# ---- ABI ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("call,needle", [
    (lambda L: L.ll_flash_attn_mx(1, 1, 1, 1, 1, 1, 1, 64, 12, 64, 1536, 1536, 100, 128, 0, 50, 0, 0, 0.1, None), "head_dim=64"),
    (lambda L: L.ll_flash_attn_mx(1, 1, 1, 1, 1, 1, 1, 64, 12, 128, 1536, 1536, 100, 100, 0, 50, 0, 0, 0.1, None), "S32=100"),
    (lambda L: L.ll_flash_attn_mx(1, 1, 1, 1, 1, 1, 1, 64, 12, 128, 1536, 1536, 100, 128, 60, 50, 0, 0, 0.1, None), "first key range"),
    (lambda L: L.ll_flash_attn_mx(1, 1, 1, 1, 1, 1, 1, 64, 12, 128, 1536, 1536, 100, 128, 0, 0, 0, 0, 0.1, None), "first key range"),
    (lambda L: L.ll_flash_attn_mx(1, 1, 1, 1, 1, 1, 1, 64, 12, 128, 1536, 1536, 100, 128, 0, 50, 90, 20, 0.1, None), "second key range"),
    (lambda L: L.ll_flash_attn_mx(1, 0, 1, 1, 1, 1, 1, 64, 12, 128, 1536, 1536, 100, 128, 0, 50, 0, 0, 0.1, None), "shadow codes"),
    (lambda L: L.ll_flash_attn_mx(1, 1, 1, 1, 0, 1, 1, 64, 12, 128, 1536, 1536, 100, 128, 0, 50, 0, 0, 0.1, None), "shadow codes"),
    (lambda L: L.ll_flash_attn_mx(1, 1, 1, 1, 1, 1, 1, 64, 12, 128, 1000, 1536, 100, 128, 0, 50, 0, 0, 0.1, None), "row strides"),
    (lambda L: L.ll_kv_shadow_mx(1, 1, 1, 1, 1, 0, 1, 100, 128, 12, 128, 0, 10, None), "shadow codes"),
    (lambda L: L.ll_kv_shadow_mx(1, 1, 1, 1, 1, 1, 1, 100, 128, 12, 96, 0, 10, None), "head_dim=96"),
    (lambda L: L.ll_kv_shadow_mx(1, 1, 1, 1, 1, 1, 1, 100, 96, 12, 128, 0, 10, None), "S32=96"),
    (lambda L: L.ll_kv_shadow_mx(1, 1, 1, 1, 1, 1, 1, 100, 128, 12, 128, 50, 101, None), "slot range [50, 101)"),
])
def test_invalid_arguments_are_rejected_before_launch(call, needle):
    L = _lib.load()
    assert call(L) == -1
    assert needle in L.ll_last_error().decode()


def test_plan_string_names_the_kernel_and_grid():
    from longlive_amd import ops
    p = ops.flash_attn_mx_plan(4680, 12, 1, [(0, 4680), (4680, 18720)])
    assert p.startswith("flash_attn_mx_kernel") and "v_mfma_scale_f32_32x32x64_f8f6f4" in p
    assert "444 workgroups of 128 query rows" in p and "293 key tiles of 64 in 1 range" in p
    p2 = ops.flash_attn_mx_plan(4680, 12, 1, [(0, 4680), (6240, 18720)])
    assert "2 ranges" in p2


# ---- switches ----------------------------------------------------------------------------------------------------------------
def test_set_attn_quant_and_cli_key():
    from longlive_amd import cli, synth
    from longlive_amd.model import CausalWanModelHIP
    m = CausalWanModelHIP(synth.toy_config(), device="cpu")
    assert m.attn_quant is None
    assert m.set_attn_quant("mxfp8") is m and m.attn_quant == "mxfp8"
    m.set_quant("int8")
    assert (m.quant, m.attn_quant) == ("int8", "mxfp8")                # orthogonal
    m.set_attn_quant(None)
    assert (m.quant, m.attn_quant) == ("int8", None)
    with pytest.raises(ValueError):
        m.set_attn_quant("int8")
    assert cli.attn_quant_mode(None) is None and cli.attn_quant_mode("none") is None
    assert cli.attn_quant_mode(" MXFP8 ") == "mxfp8"
    with pytest.raises(ValueError):
        cli.attn_quant_mode("fp8")
