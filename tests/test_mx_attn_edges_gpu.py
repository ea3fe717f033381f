"""flash_attn_mx_kernel and kv_shadow_mx_kernel at their tile, range and stride edges, through the C ABI with explicit pointers and
strides (ops.flash_attn_mx always passes ldq = ldo = H * 128 and production shapes).

Attention runs the exact data of tests/mx_attn_exact.py, which tests/test_mx_attn_edges_host.py proves to have ONE bf16 bit pattern
(every sum exact in any order, no expected element near a rounding tie) and to move under every listed departure from the scheme:
the comparison is torch.equal.  q padding columns hold NaN, `out` is a NaN field with sentinel rows, the shadows are the HOST's bytes
(ll_kv_shadow_mx is pinned to the same bytes below).  The shadow refresh is compared byte for byte, inside and OUTSIDE the refreshed
blocks.  One random-data case per geometry class keeps the rel-L2 bound of tests/test_mx_attn_gpu.py."""
import pytest
import torch

import mx_attn_exact as X
import mx_attn_ref as MA
from bf16_exact import lib as _lib
from bf16_exact import nan_bf16 as _nan_bf16
from bf16_exact import run as _run
from bf16_exact import untouched_bf16 as _untouched_bf16
from util import bf, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
U8 = torch.uint8
KERNEL_BOUND = 3e-3          # tests/test_mx_attn_gpu.py's
NAN_CODE, NAN_SCALE = 0x7F, 0xFF      # e4m3fn NaN, E8M0 NaN


def _shadow(b):
    """The host's shadow bytes of a built case on the device: kq, ks, vq, vs (uint8)."""
    return [t.view(U8).to(DEV).contiguous() for t in (b.kq, b.ks, b.vq, b.vs)]


def _attn(b, shadow, Lq=None, pad_q=0, pad_o=0, scale=X.SCALE):
    """One ll_flash_attn_mx call on the first Lq rows of a built case; checks padding and sentinels; returns out [B, Lq, H, 128]."""
    c = b.case
    B, H, Lq = c.B, c.H, Lq or c.Lq
    C = H * 128
    qb = _nan_bf16(B * Lq, C + pad_q)
    qb[:, :C] = b.q[:, :Lq].reshape(B * Lq, C).to(DEV)
    out = _nan_bf16(B * Lq + 3, C + pad_o)
    _run("ll_flash_attn_mx", qb, *shadow, out, B, Lq, H, 128, C + pad_q, C + pad_o, c.S, c.S32, *c.seg_args(), scale)
    assert _untouched_bf16(out[B * Lq:]) and _untouched_bf16(out[:, C:]), f"{c} Lq {Lq} ldo {C + pad_o}: wrote outside [B * Lq, H * 128]"
    return out[:B * Lq, :C].reshape(B, Lq, H, 128).cpu()


def _assert_bits(got, want, what):
    if not torch.equal(got.view(torch.int16), want.view(torch.int16)):
        bad = (got.view(torch.int16) != want.view(torch.int16))
        i = [int(x) for x in bad.nonzero()[0]]
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ, first at {i}: got {got[tuple(i)].item()} want "
                             f"{want[tuple(i)].item()}")


def _plan(c, Lq=None):
    from longlive_amd import ops
    return ops.flash_attn_mx_plan(Lq or c.Lq, c.H, c.B, c.segs)


# ---- ll_flash_attn_mx ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in X.EXACT_CASES if c is not X.ROWS], ids=repr)
def test_exact_case(case):
    """Range start mod 64 x range length, ranges ending at S and past S32 (the staging clamp), two ranges of every kind, zero K slots
    and a zero V block, the lazy-max constructions, B = 2 with H = 3: the expected bits, and the plan's tile and range counts."""
    b = X.Built.get(case)
    nt, nr = case.plan_counts()
    assert f"{nt} key tiles of 64 in {nr} range" in _plan(case), _plan(case)
    _assert_bits(_attn(b, _shadow(b)), b.want, case)
    if case is X.BATCH:
        _assert_bits(_attn(b, _shadow(b), pad_q=136, pad_o=8), b.want, f"{case} wide")


@pytest.mark.parametrize("Lq", X.LQ)
def test_rows_and_strides(Lq):
    """Lq from 1 to 257 (a lone row, ragged waves, a ragged workgroup, a third workgroup of one row) x ldq, ldo = H * 128 + {0, 8, 136}
    and ldo = H * 128 + 4: rows on 8 bytes are all the 8-byte stores of the epilogue need (a lane writes 4 bf16 at column offsets that
    are multiples of 4), so the entry point's ldo % 4 == 0 stands."""
    b = X.Built.get(X.ROWS)
    sh = _shadow(b)
    wg = (Lq + 127) // 128 * X.ROWS.H
    assert f"{wg} workgroups of 128 query rows, 3 key tiles of 64 in 2 ranges" in _plan(X.ROWS, Lq)
    for pad_q, pad_o in ((0, 0), (8, 8), (136, 136), (0, 4), (8, 136), (136, 4)):
        _assert_bits(_attn(b, sh, Lq, pad_q, pad_o), b.want[:, :Lq], f"Lq {Lq} ldq +{pad_q} ldo +{pad_o}")


UNREFRESHED = [c for c in X.GEOMETRY + X.ENDS + X.TWO if set(c.staged_blocks()) - set(c.touched_blocks())][::3] + [X.BATCH]


@pytest.mark.parametrize("case", UNREFRESHED, ids=repr)
def test_blocks_no_refresh_derived(case):
    """ll_flash_attn_mx's precondition: every block a tile stages has been derived or zeroed.  (1) ops.kv_shadow_mx_alloc hands out
    zeros, and a fresh shadow refreshed over the key ranges ALONE gives the expected bits, although tiles stage blocks no refresh
    touched.  (2) What no tile stages is never read into the result, nor is the K^ row of a masked slot: NaN codes (0x7f) and NaN
    scale bytes (0xff) there leave the bits alone.  (A staged, underived V^ block holding such bytes makes the output NaN -- 0 x NaN in
    the MFMA -- which is why the allocation zero-fills; measured once, not asserted.)"""
    from longlive_amd import ops
    b = X.Built.get(case)
    k, v = b.k.to(DEV), b.v.to(DEV)
    sh = ops.kv_shadow_mx_alloc(k)
    assert not any(bool(sh[n].view(U8).any()) for n in ("kq", "ks", "vq", "vs"))
    for lo, hi in case.segs:
        ops.kv_shadow_mx(k, v, sh, lo, hi)
    got = ops.flash_attn_mx(b.q.to(DEV), sh, case.segs, scale=X.SCALE).cpu()
    _assert_bits(got, b.want, f"{case}: shadow refreshed over the ranges only")
    kq, ks, vq, vs = _shadow(b)
    inr = torch.zeros(case.S32, dtype=torch.bool)
    inr[case.inr] = True
    kq[:, ~inr] = NAN_CODE
    ks[:, ~inr] = NAN_SCALE
    staged = torch.zeros(case.S32 // 32, dtype=torch.bool)
    staged[case.staged_blocks()] = True
    vq[:, :, ~staged] = NAN_CODE
    vs[:, :, ~staged] = NAN_SCALE
    touched = torch.zeros_like(staged)
    touched[case.touched_blocks()] = True
    vq[:, :, staged & ~touched] = 0
    vs[:, :, staged & ~touched] = 0
    _assert_bits(_attn(b, [kq, ks, vq, vs]), b.want, f"{case}: NaN bytes in masked K^ rows and unstaged V^ blocks")


def test_refusals_launch_and_write_nothing():
    """Overlapping ranges (their shared keys would count twice), a scale that is not positive and finite (the tile maximum is taken
    before the multiplication by c), S32 not S rounded up, ranges past S, head_dim != 128, strides off their alignment or below
    H * 128: LL_ERR_INVALID_ARG with the reason in ll_last_error, and `out` keeps its NaN field."""
    L, lib = _lib()
    b = X.Built.get(X.TWO[0])
    c = b.case
    sh = _shadow(b)
    C = c.H * 128
    qb = torch.zeros(c.Lq, C + 8, dtype=bf, device=DEV)
    out = _nan_bf16(c.Lq + 3, C + 8)
    ok = dict(hd=128, ldq=C, ldo=C, S=c.S, S32=c.S32, segs=c.seg_args(), scale=X.SCALE)
    bad = [(dict(segs=(0, 50, 40, 30)), "overlap"), (dict(segs=(40, 30, 0, 41)), "overlap"), (dict(segs=(0, 50, 0, 50)), "overlap"),
           (dict(scale=0.0), "scale="), (dict(scale=-X.SCALE), "scale="), (dict(scale=float("nan")), "scale="),
           (dict(scale=float("inf")), "scale="), (dict(S32=c.S32 + 32), "S32="), (dict(S32=c.S), "S32="),
           (dict(segs=(0, c.S + 1, 0, 0)), "first key range"), (dict(segs=(0, 10, c.S - 5, 6)), "second key range"),
           (dict(hd=64), "head_dim=64"), (dict(ldq=C + 4), "row strides"), (dict(ldo=C + 2), "row strides"), (dict(ldq=C - 8), "row strides"),
           (dict(ldo=C - 4), "row strides")]
    for kw, needle in bad:
        a = dict(ok, **kw)
        with pytest.raises(RuntimeError, match=needle):
            _run("ll_flash_attn_mx", qb, *sh, out, 1, c.Lq, c.H, a["hd"], a["ldq"], a["ldo"], a["S"], a["S32"], *a["segs"], a["scale"])
    torch.cuda.synchronize()
    assert _untouched_bf16(out)
    # ll_flash_attn shares the overlap rule
    kv = torch.zeros(1, c.S, C, dtype=bf, device=DEV)
    with pytest.raises(RuntimeError, match="overlap"):
        _run("ll_flash_attn", qb, kv, kv, out, 1, c.Lq, c.H, C, C, C, c.S * C, 0, 50, 40, 30, X.SCALE)
    torch.cuda.synchronize()
    assert _untouched_bf16(out)


@pytest.mark.parametrize("name", list(X.RANDOM))
def test_random_data_per_geometry_class(name):
    """Ragged Lq, a clamped last tile, two ranges in one tile: random data against the restatement, rel-L2 below the project's bound."""
    B, Lq, H, S, segs = X.RANDOM[name]
    q, k, v = X.random_data(B, Lq, H, S)
    c = X.Case(name, B, Lq, H, S, segs)
    b = X.Built.__new__(X.Built)
    b.case, b.q = c, q
    b.kq, b.ks = MA.shadow_k(k)
    b.vq, b.vs = MA.shadow_v(v)
    got = _attn(b, _shadow(b), pad_q=8, pad_o=8, scale=1.0 / 128 ** 0.5).float()
    want = MA.mx_attention_cache(q, k, v, segs).to(bf).float()
    r = rel_l2(got, want)
    print(f"{name}: flash_attn_mx vs restatement relL2 {r:.2e}")
    assert torch.isfinite(got).all() and r < KERNEL_BOUND, r


# ---- ll_kv_shadow_mx -----------------------------------------------------------------------------------------------------------------
SENTINEL = 0xA5


def _cache_pair(B, S, H, seed):
    """Random bf16 k / v with, along V's slot axis in (batch 0, head 0), the blocks this kernel alone quantises: channel 0 an amax on
    the m > 0.875 step (0.875 x 2^3), channel 1 just above it, channel 2 all zero, channel 3 small values that become e4m3 subnormals
    (one of them a rounding tie), channel 4 bf16's smallest subnormal alone (the exponent clamps at -127), channel 5 bf16's largest."""
    g = torch.Generator().manual_seed(seed)
    k = torch.randn(B, S, H, 128, generator=g).to(bf)
    v = (0.5 * torch.randn(B, S, H, 128, generator=g)).to(bf)
    n = min(S, 32)
    i = torch.arange(n)
    v[0, :n, 0, 0] = (0.25 * ((i % 5).float() - 2)).to(bf); v[0, 0, 0, 0] = 7.0
    v[0, :n, 0, 1] = v[0, :n, 0, 0]; v[0, 0, 0, 1] = 7.03125
    v[0, :n, 0, 2] = 0.0
    v[0, :n, 0, 3] = (2.0 ** -16 * (i % 4).float()).to(bf); v[0, 0, 0, 3] = 1.0
    if n > 1:
        v[0, 1, 0, 3] = 3 * 2.0 ** -18
    v[0, :n, 0, 4] = 0.0; v[0, n - 1, 0, 4] = 2.0 ** -133
    v[0, :n, 0, 5] = v[0, :n, 0, 0]; v[0, 0, 0, 5] = -3.3895313892515355e38
    k[0, 0, 0, :32] = 0.0; k[0, 0, 0, 5] = 2.0 ** -133
    return k, v


def _host_shadow(k, v):
    kq, ks = MA.shadow_k(k)
    vq, vs = MA.shadow_v(v)
    return [t.view(U8) for t in (kq, ks, vq, vs)]


@pytest.mark.parametrize("S", [1, 31, 32, 33, 95, 100])
def test_shadow_refresh_writes_its_blocks_and_no_others(S):
    """B = 2, H = 3.  A sentinel-filled shadow after a full refresh carries the host's bytes everywhere (padding slots of the last
    block: zero codes under scale byte 127 in K^, zeros in V^'s blocks).  Then the cache changes EVERYWHERE and one range is refreshed:
    blocks lo / 32 .. ceil(hi / 32) - 1 of all four arrays carry the new bytes, every other byte the old ones; lo == hi changes
    nothing."""
    B, H = 2, 3
    S32 = (S + 31) // 32 * 32
    k1, v1 = _cache_pair(B, S, H, 3)
    k2, v2 = _cache_pair(B, S, H, 4)
    k2, v2 = -k2, -v2
    old, new = _host_shadow(k1, v1), _host_shadow(k2, v2)
    assert all(not torch.equal(a, b) for a, b in zip(old, new))
    assert old[3][0, 0, 0, 4] == 0 and old[1][0, 0, 0, 0] == 0                       # the exponent clamp is reached: byte 0 = 2^-127
    if S % 32:
        assert not old[0][:, S:].any() and bool((old[1][:, S:] == 127).all())
    names = ("K codes", "K scales", "V codes", "V scales")
    sh = [torch.full(t.shape, SENTINEL, dtype=U8, device=DEV) for t in old]
    k1d, v1d, k2d, v2d = (t.to(DEV) for t in (k1, v1, k2, v2))
    _run("ll_kv_shadow_mx", k1d, v1d, *sh, B, S, S32, H, 128, 0, S)
    for n, got, want in zip(names, sh, old):
        assert torch.equal(got.cpu(), want), f"S {S} full refresh: {n}"
    base = [t.clone() for t in sh]
    ranges = [r for r in ((0, 1), (31, 33), (32, 64), (S - 1, S), (0, S), (0, 0), (S, S), (min(S, 40), min(S, 40))) if r[1] <= S and r[0] >= 0]
    for lo, hi in dict.fromkeys(ranges):
        sh = [t.clone() for t in base]
        _run("ll_kv_shadow_mx", k2d, v2d, *sh, B, S, S32, H, 128, lo, hi)
        j0, j1 = (lo // 32, (hi + 31) // 32) if hi > lo else (0, 0)
        want = [t.clone() for t in old]
        want[0][:, 32 * j0:32 * j1] = new[0][:, 32 * j0:32 * j1]
        want[1][:, 32 * j0:32 * j1] = new[1][:, 32 * j0:32 * j1]
        want[2][:, :, j0:j1] = new[2][:, :, j0:j1]
        want[3][:, :, j0:j1] = new[3][:, :, j0:j1]
        for n, got, w in zip(names, sh, want):
            assert torch.equal(got.cpu(), w), f"S {S} refresh [{lo}, {hi}): {n}"


def test_shadow_refusals_write_nothing():
    B, S, H = 1, 40, 1
    k = torch.zeros(B, S, H, 128, dtype=bf, device=DEV)
    sh = [torch.full(s, SENTINEL, dtype=U8, device=DEV) for s in ((B, 64, H, 128), (B, 64, H, 4), (B, H, 2, 128, 32), (B, H, 2, 128))]
    for args, needle in (((B, S, 32, H, 128, 0, S), "S32=32"), ((B, S, 64, H, 64, 0, S), "head_dim=64"), ((B, S, 64, H, 128, 5, 41), "slot range"),
                         ((B, S, 64, H, 128, 9, 8), "slot range"), ((B, S, 64, H, 128, -1, 8), "slot range")):
        with pytest.raises(RuntimeError, match=needle):
            _run("ll_kv_shadow_mx", k, k, *sh, *args)
    torch.cuda.synchronize()
    assert all(bool((t == SENTINEL).all()) for t in sh)
