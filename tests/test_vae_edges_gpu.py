"""The VAE decoder's kernels (csrc/conv.hip) at their tile and border edges, through the C ABI with explicit pointers and strides
(ops.conv_cl always passes ldo = Cout and cannot place guard frames).

Convolutions run on the exact data of tests/vae_exact.py -- every fp32 sum is exact in any order, so the output has ONE correct bit
pattern, the fp64 F.conv3d result rounded once (twice with a residual) -- and are compared with torch.equal.  Every case
  * asserts from ll_conv_plan that it runs the kernel instance it was written for (conv_cl_kernel<NT, MODE> /
    conv_halo_kernel<NCB, UP, RMS>), so a moved threshold cannot migrate it silently;
  * puts the input between NaN guard frames -- directly before the first frame the contract allows to be read (the first history
    frame for KT = 3, x itself for KT = 1) and directly after the last one: an out-of-contract read reaches the output;
  * writes rows of ldo > Cout (ldo % 8 == 4 and == 0 alternate) into a field of NAN16 with sentinel rows after the last pixel, whose
    bits must be unchanged; res has the same ldo and in some cases IS out.
The fused RMS form and ll_rms_silu_cl keep the project's bound for that arithmetic (1 ulp, 98 % exact, against the reference's
rounding-point chain evaluated on the exact raw tensor); ll_softmax_rows is bit-exact on its exact rows and within
vae_exact.SOFTMAX_BOUND_ULP of the fp64 softmax rounded once elsewhere; the two layout kernels are bit-exact."""
import ctypes

import pytest
import torch

import vae_exact as E
from util import assert_bf16_close, bf, bf16_ulp_distance

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN16 = E.NAN16


# ---- plumbing -------------------------------------------------------------------------------------------------------------------------
def _lib():
    from longlive_amd import _lib as L
    return L, L.load()


def _run(fn, *args):
    from longlive_amd import ops as O
    L, lib = _lib()
    a = [t.data_ptr() if isinstance(t, torch.Tensor) else t for t in args]
    L.check(getattr(lib, fn)(*a, O._stream()), fn)


def _nan_bf16(*shape):
    return torch.full(shape, NAN16, dtype=torch.int16, device=DEV).view(bf)


def _untouched(t):
    return bool((t.contiguous().view(torch.int16) == NAN16).all())


def _plan(g, res=0, rms=0):
    L, lib = _lib()
    buf = ctypes.create_string_buffer(512)
    L.check(lib.ll_conv_plan(g[0], g[1], g[2], g[3], g[4], g[5], g[6], int(g[7]), int(res), int(rms), buf, 512), "ll_conv_plan")
    return buf.value.decode()


class _halo:
    """Tuning key conv_halo for the duration of a case; the shipped value (1) afterwards, whatever happens."""

    def __init__(self, v):
        self.v = v

    def __enter__(self):
        L, lib = _lib()
        L.check(lib.ll_set_tuning(b"conv_halo", self.v), "ll_set_tuning")

    def __exit__(self, *exc):
        _lib()[1].ll_set_tuning(b"conv_halo", 1)


def instance(case):
    """The kernel instance a case was written for, as ll_conv_plan's text starts (epilogue left open)."""
    (T, H, W, Cin, Cout, KT, KH, up), kind = case[0], case[1]
    if kind == "halo":
        return f"conv_halo_kernel<bias, NCB {1 if Cout <= 16 else 6}, UP {int(up)}, RMS 0>"
    nt = 1 if Cout <= 32 else 3 if (Cout % 96 == 0 and Cout % 128 != 0) else 4
    return f"conv_cl_kernel<bias, NT {nt}, MODE {0 if Cin < 64 else 2 if up else 1}>"


def _conv(d, res=False, pad=4, alias=False, rms=None, want_raw=True):
    """One launch on ConvData d.  Returns (out [M, Cout] or None, out_rms or None) after checking every sentinel.
    rms = (gamma, silu): ll_conv_cl_rms (ldo = Cout by its contract: pad is ignored)."""
    Cout, M = d.Cout, d.M
    ldo = Cout if rms is not None else Cout + pad
    G = 1
    buf = torch.full((G + d.nh + d.T + G, d.H, d.W, d.Cin), float("nan"), dtype=bf, device=DEV)
    buf[G:G + d.nh + d.T] = d.frames.to(bf).to(DEV)
    x = buf[G + d.nh]
    assert x.data_ptr() + d.T * d.H * d.W * d.Cin * 2 == buf[G + d.nh + d.T].data_ptr()      # the input ends exactly at its last frame
    zero = torch.zeros(32, dtype=bf, device=DEV)
    w, b = d.packed_w().to(DEV), d.bias.to(bf).to(DEV)
    out = _nan_bf16(M + 3, ldo)
    r = None
    if res:
        r = out if alias else _nan_bf16(M, ldo)
        r[:M, :Cout] = d.res.view(M, Cout).to(bf).to(DEV)
    tail = (d.T, d.H, d.W, d.Cin, Cout, d.Kpad, d.KT, d.KH, int(d.up), ldo)
    if rms is None:
        _run("ll_conv_cl", x, zero, w, b, r, out, *tail)
        out2 = None
    else:
        gamma, silu = rms
        out2 = _nan_bf16(M + 3, ldo)
        _run("ll_conv_cl_rms", x, zero, w, b, r, out if want_raw else None, gamma, out2, int(silu), *tail)
        assert _untouched(out2[M:]), "ll_conv_cl_rms wrote out_rms rows beyond the last pixel"
        if not want_raw:
            assert _untouched(out), "ll_conv_cl_rms wrote the raw tensor it was told not to"
    torch.cuda.synchronize()
    assert _untouched(out[M:]) and _untouched(out[:M, Cout:]), f"wrote outside [M, Cout] (ldo {ldo})"
    if res and not alias:
        assert _untouched(r[:, Cout:])
    assert bool(torch.isnan(buf[:G].float()).all()) and bool(torch.isnan(buf[-G:].float()).all())
    return (out[:M, :Cout] if want_raw else None), (out2[:M] if out2 is not None else None)


def _check(d, got, res, what):
    want = (d.want_res if res else d.want).view(d.M, d.Cout).to(DEV)
    if not torch.equal(got, want):
        bad = (got.view(torch.int16) != want.view(torch.int16)).any(-1).nonzero().flatten()
        px = [(int(m) // (d.Ho * d.Wo), int(m) % (d.Ho * d.Wo) // d.Wo, int(m) % d.Wo) for m in bad[:12]]
        ch = (got.view(torch.int16) != want.view(torch.int16)).any(0).nonzero().flatten()[:12].tolist()
        raise AssertionError(f"{what}: {len(bad)} of {d.M} pixels differ, first (t, h, w) {px}, channels {ch}")


# ---- the case lists -------------------------------------------------------------------------------------------------------------------
# (T, H, W): M = 1, 255, 256, 257 (H = 1), W = 1, 2 x 2, T = 4 with the 256-pixel seam inside a row of frame 2, T = 3 (frame 2 reads new
# frame 0), five m-tiles
GEOS = [(1, 1, 1), (1, 15, 17), (1, 16, 16), (1, 1, 257), (3, 7, 1), (2, 2, 2), (4, 9, 13), (3, 11, 12), (2, 20, 31)]
COUTS = [8, 16, 24, 32, 96, 192, 288, 40, 128, 136, 384, 768]       # NT 1 | NT 3 | NT 4 (40, 136: ragged last n-tile)
TAPS = [(3, 3), (3, 1), (1, 3), (1, 1)]


def _cl_cases():
    """(geometry, 'cl', residual, ldo pad, history, res aliases out)"""
    cases, i = [], 0

    def add(T, H, W, Cin, Cout, KT, KH, up=False):
        nonlocal i
        res = i % 2 == 1
        cases.append(((T, H, W, Cin, Cout, KT, KH, up), "cl", res, (4, 8, 12, 0)[i % 4], "zero" if i % 3 == 2 else "nonzero", res and i % 4 == 3))
        i += 1
    # MODE 0: every Cin < 64 x every tap shape, walking the geometries and the channel counts; then with upsample
    for Cin in (8, 16, 32, 56):
        for KT, KH in TAPS:
            add(*GEOS[i % len(GEOS)], Cin, COUTS[(i * 5) % len(COUTS)], KT, KH)
    for Cin, geo in ((8, (1, 1, 1)), (32, (2, 5, 7)), (56, (1, 8, 16)), (16, (1, 1, 9))):
        add(*geo, Cin, COUTS[i % 4], 1, 3, True)
    # MODE 1: Cin 64 (one tap per K-step), 72 (the tap boundary drifts through the K-steps; K = 1944, 648 not multiples of 64), 96
    # (K = 2592, 864: the last K-step straddles the live / padded boundary), 192, 384; every tap shape
    for Cin, KT, KH, geo, Cout in ((64, 3, 3, (2, 9, 15), 96), (72, 3, 3, (3, 7, 1), 40), (96, 3, 3, (4, 9, 13), 136), (72, 1, 3, (1, 15, 17), 24),
                                   (96, 1, 3, (1, 1, 257), 192), (64, 1, 1, (1, 16, 16), 8), (192, 1, 1, (2, 20, 31), 96), (192, 3, 3, (3, 11, 12), 32),
                                   (384, 3, 1, (3, 5, 6), 768), (384, 3, 3, (2, 9, 15), 384), (72, 3, 1, (4, 2, 2), 288), (384, 1, 3, (1, 1, 1), 128),
                                   (96, 3, 3, (2, 32, 32), 96), (192, 3, 3, (1, 16, 32), 192), (96, 3, 3, (1, 16, 32), 8)):     # the halo kernel's own
        add(*geo, Cin, Cout, KT, KH)
    # n-tilings: every Cout at Cin 64, 1x3x3, two m-tiles with a ragged second one
    for Cout in COUTS:
        add(2, 9, 15, 64, Cout, 1, 3)
    # MODE 2: odd and even H, W; 8 x 16 is the halo kernel's own shape
    for Cin, geo, Cout in ((64, (1, 3, 5), 96), (96, (2, 4, 6), 192), (384, (1, 5, 4), 40), (64, (1, 1, 1), 8), (96, (1, 8, 16), 96), (384, (2, 7, 16), 192)):
        add(*geo, Cin, Cout, 1, 3, True)
    return cases


def _halo_cases():
    cases, i = [], 0

    def add(T, H, W, Cin, Cout, KT=3, up=False):
        nonlocal i
        res = i % 2 == 0
        cases.append(((T, H, W, Cin, Cout, KT, 3, up), "halo", res, (4, 8, 0)[i % 3], "zero" if i % 4 == 3 else "nonzero", res and i % 4 == 2))
        i += 1
    for Cin, Cout in ((32, 96), (64, 192), (96, 384), (160, 96), (384, 96), (96, 8), (32, 16)):      # one tile exactly, all four borders
        add(1, 16, 32, Cin, Cout)
    add(2, 24, 32, 32, 96)           # partial bottom only (8 of 16 rows)
    add(1, 16, 52, 64, 96)           # partial right only (20 of 32 columns)
    add(3, 30, 52, 32, 192)          # both partial, three frames
    add(1, 30, 52, 96, 16)           # ... the head
    add(1, 48, 96, 32, 96)           # interior tiles
    add(2, 32, 64, 96, 96)
    for H, W, Cin, Cout in ((8, 16, 64, 96), (7, 16, 192, 96), (15, 26, 64, 192), (8, 16, 384, 96), (15, 26, 32, 96)):     # upsampled: source sizes
        add(2 if Cin == 64 else 1, H, W, Cin, Cout, KT=1, up=True)
    return cases


CL_CASES, HALO_CASES = _cl_cases(), _halo_cases()
# either side of `fits` (>= 70 % of the tile grid filled, even sizes): 16 x 44 = 68.75 % and 22 x 32 = 68.75 % stay on the implicit
# GEMM, 16 x 46 = 71.9 % and 24 x 32 = 75 % go to the halo kernel; odd sizes never do
THRESHOLD_CASES = [((1, 16, 44, 32, 96, 3, 3, False), "cl", False, 4, "nonzero", False), ((1, 16, 46, 32, 96, 3, 3, False), "halo", False, 4, "nonzero", False),
                   ((1, 22, 32, 32, 96, 3, 3, False), "cl", True, 8, "nonzero", False), ((1, 24, 32, 32, 96, 3, 3, False), "halo", True, 8, "nonzero", False),
                   ((1, 17, 32, 32, 96, 3, 3, False), "cl", False, 4, "zero", False), ((1, 11, 16, 64, 96, 1, 3, True), "cl", False, 8, "nonzero", False),
                   ((1, 12, 16, 64, 96, 1, 3, True), "halo", False, 8, "nonzero", False)]


def _id(c):
    g = c[0]
    return f"{g[0]}x{g[1]}x{g[2]}-{g[3]}to{g[4]}-k{g[5]}{g[6]}{'-up' if g[7] else ''}-{c[1]}{'-res' if c[2] else ''}{'-alias' if c[5] else ''}-pad{c[3]}-{c[4]}"


def _run_case(c, tuning):
    g, kind, res, pad, hist, alias = c
    d = E.ConvData(*g, seed=g[3] + g[4], hist=hist)
    with _halo(tuning):
        plan = _plan(g, res)
        assert plan.startswith(instance(c).replace("<bias", "<bias_res" if res else "<bias")), plan
        got, _ = _conv(d, res, pad, alias)
    _check(d, got, res, f"{_id(c)} [{plan}]")


@pytest.mark.parametrize("case", CL_CASES, ids=_id)
def test_implicit_gemm_conv_is_bit_exact(case):
    _run_case(case, 0)


@pytest.mark.parametrize("case", HALO_CASES + THRESHOLD_CASES, ids=_id)
def test_halo_conv_and_its_threshold_are_bit_exact(case):
    _run_case(case, 1)


# ---- impulses ---------------------------------------------------------------------------------------------------------------------------
def _impulse_positions(T, H, W, up, seams_m):
    hs = {0, H - 1} | {h for h in ((7, 8, 15, 16) if up else (15, 16)) if h < H}
    ws = {0, W - 1} | {w for w in ((15, 16) if up else (31, 32)) if w < W}
    pos = [(T - 1, h, w) for h in sorted(hs) for w in sorted(ws)]
    Ho, Wo = (2 * H, 2 * W) if up else (H, W)
    for m in seams_m:                                     # both sides of the 256-pixel m-tile seams of the implicit GEMM
        for mm in (m - 1, m):
            if 0 <= mm < T * Ho * Wo:
                pos.append((mm // (Ho * Wo), (mm % (Ho * Wo) // Wo) >> up, (mm % Wo) >> up))
    return list(dict.fromkeys(pos))


@pytest.mark.parametrize("geom,tuning", [((2, 30, 52, 32, 96, 3, 3, False), 1), ((2, 30, 52, 32, 96, 3, 3, False), 0), ((2, 30, 52, 32, 8, 3, 3, False), 1),
                                         ((1, 15, 26, 64, 96, 1, 3, True), 1), ((1, 15, 26, 64, 96, 1, 3, True), 0), ((2, 17, 33, 8, 16, 3, 1, False), 1),
                                         ((1, 9, 17, 8, 8, 1, 3, True), 1)], ids=str)
def test_impulse_response_is_the_weight_stencil(geom, tuning):
    """One non-zero input pixel at the image corners, both sides of every halo-tile seam and of the m-tile seams: the output is the
    weight stencil around it (the host reference; tests/test_vae_edges_host.py shows it is the stencil) and zero elsewhere, bit for bit."""
    T, H, W, Cin, Cout, KT, KH, up = geom
    Ho, Wo = (2 * H, 2 * W) if up else (H, W)
    with _halo(tuning):
        plan = _plan(geom)
        kind = "halo" if (tuning and Cin % 32 == 0 and KH == 3 and (KT == 3 or up) and (Cout % 96 == 0 or Cout <= 16)) else "cl"
        assert plan.startswith(instance((geom, kind))), plan
        for pos in _impulse_positions(T, H, W, up, range(256, min(T * Ho * Wo, 1025), 256)):
            d = E.ConvData(*geom, seed=9, impulse=pos, zero_bias=True, hist="zero")
            got, _ = _conv(d, pad=4)
            _check(d, got, False, f"impulse at {pos} [{plan}]")


# ---- the fused RMS epilogue and ll_rms_silu_cl ----------------------------------------------------------------------------------------------
def _assert_rms(got, raw, gamma, silu, what):
    want = E.rms_silu_host(raw.cpu(), gamma.cpu(), silu)
    assert_bf16_close(got, want, 1, 0.98, what)


def _shifts(d0):
    """Powers of two that put the rows' norms (a) above 2^60, the plain-division branch of `tame`, with every sum of squares still
    finite in fp32, and (b) below 2^-60 -- there max(n, 1e-12) applies: the kernel's lower `tame` limit is unreachable behind it."""
    n = E.rows_norm(d0.want_res.view(d0.M, d0.Cout))
    top = int(torch.ceil(torch.log2(n.max())))
    return 63 - top, -61 - top


@pytest.mark.parametrize("geom,res,silu,want_raw", [((1, 16, 32, 96, 96, 3, 3, False), False, True, True), ((2, 30, 52, 32, 96, 3, 3, False), True, True, True),
                                                    ((1, 8, 16, 64, 96, 1, 3, True), False, False, True), ((1, 15, 26, 192, 96, 1, 3, True), True, True, False)],
                         ids=str)
def test_conv_rms_raw_is_exact_and_rms_follows_the_reference_chain(geom, res, silu, want_raw):
    """ll_conv_cl_rms on exact data, at shift 0 and at the two power-of-two scalings of _shifts: the raw tensor is the exact expected
    one (once it is not written: out = NULL), out_rms is the reference's chain on that exact tensor within 1 ulp / 98 % exact (the
    bound of test_conv_cl_rms_is_conv_then_rms_silu).  A 6 x 8 box of zero input with zero bias and residual gives all-zero pixels
    (n = 0: max(n, 1e-12))."""
    up = geom[7]
    gamma = (1.0 + E._codes((96,), 3, -8, 8) * 2.0 ** -5).to(bf).to(DEV)
    box = dict(zero_box=(2, 8, 4, 12), zero_bias=True)
    d0 = E.ConvData(*geom, seed=11, **box)
    plan = _plan(geom, res, 1)
    assert plan.startswith(f"conv_halo_kernel<{'bias_res' if res else 'bias'}, NCB 6, UP {int(up)}, RMS 1>"), plan
    for shift in (0,) + _shifts(d0):
        d = d0 if shift == 0 else E.ConvData(*geom, seed=11, shift=shift, **box)
        want = (d.want_res if res else d.want).view(d.M, 96)
        n = E.rows_norm(want)
        assert int((n == 0).sum()) >= 4, "no all-zero pixel"
        if shift > 0:
            assert int((n > 2.0 ** 60).sum()) > d.M // 2 and n.max() < 2.0 ** 63.5
        if shift < 0:
            assert n.max() < 2.0 ** -60
        raw, out2 = _conv(d, res, rms=(gamma, silu), want_raw=want_raw)
        if want_raw:
            _check(d, raw, res, f"fused raw, shift {shift}")
        _assert_rms(out2, want, gamma, silu, f"fused rms {geom} shift {shift}")


@pytest.mark.parametrize("C", [8, 96, 128, 136, 256, 264, 512])
@pytest.mark.parametrize("pixels", [1, 5, 17, 35])
def test_rms_silu_rows_at_the_lane_group_edges(C, pixels):
    """ll_rms_silu_cl at the G = 16 / 32 / 64 boundaries (C = 128 | 136, 256 | 264), pixel counts that do not fill a block, rows of
    integer codes under 2^0, 2^e_big (n > 2^60: plain division) and 2^-70 (n < 1e-12: the clamp), zero rows; guard row after the output."""
    import math
    e_big = 61 - int(math.floor(math.log2(math.sqrt(C))))
    x = E._codes((pixels, C), C + pixels)
    sc = torch.tensor([0.0, float(e_big), -70.0, 3.0, 0.0])[torch.arange(pixels) % 5]
    x = x * torch.pow(2.0, sc.double()).view(-1, 1)
    x[torch.arange(pixels) % 5 == 4] = 0.0
    x = x.to(bf)
    n = E.rows_norm(x)
    assert n.max() < 2.0 ** 63.6 and (pixels < 2 or n.max() > 2.0 ** 60)
    gamma = (1.0 + E._codes((C,), 5, -8, 8) * 2.0 ** -5).to(bf)
    for silu in (True, False):
        out = _nan_bf16(pixels + 1, C)
        _run("ll_rms_silu_cl", x.to(DEV), gamma.to(DEV), out, pixels, C, int(silu))
        torch.cuda.synchronize()
        assert _untouched(out[pixels:])
        _assert_rms(out[:pixels], x, gamma, silu, f"rms_silu C={C} pixels={pixels} silu={silu}")


# ---- ll_softmax_rows ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,ld,scale", E.SOFTMAX_SHAPES)
@pytest.mark.parametrize("rows", [1, 7])
def test_softmax_rows_exact_rows_padding_and_bound(N, ld, scale, rows):
    """rows + 2 rows (3 and 9: not multiples of the 4 rows of a block).  Row 0: one column at +A, the others at -A with 2 A scale log2(e)
    > 10 + log2(N) binary orders, so all other weights together stay below half a bf16 ulp of 1: exactly 1.0 there.  Row 1, for a
    power-of-two N: constant, exactly 1 / N.  The other rows: SOFTMAX_BOUND_ULP from the fp64 softmax rounded once.  Columns from N on:
    +0 bits; the row after the last: untouched."""
    import math
    R = rows + 2
    s = E.softmax_rows_data(R, N, ld, N + rows)
    big = scale * 1.4426950408889634
    A = 2.0 ** math.ceil(math.log2((10 + math.log2(N)) / (2 * big)))
    lead = min(N - 1, 5)
    s[0, :N] = -A
    s[0, lead] = A
    pow2 = N & (N - 1) == 0
    if pow2:
        s[1, :N] = 1.5
    p = _nan_bf16(R + 1, ld)
    _run("ll_softmax_rows", s.to(DEV), p, R, N, ld, ctypes.c_float(scale))
    torch.cuda.synchronize()
    assert _untouched(p[R:])
    got = p[:R].cpu()
    assert bool((got[:, N:].contiguous().view(torch.int16) == 0).all()), "padding columns are not +0"
    assert got[0, lead].item() == 1.0 and int((got[0, :N].float() >= 2.0 ** -9).sum()) == 1
    if pow2:
        assert torch.equal(got[1, :N], torch.full((N,), 1.0 / N).to(bf)), "constant row of a power-of-two N is not 1 / N"
    want = E.softmax_host(s, N, scale)
    d = bf16_ulp_distance(got[2:, :N], want[2:, :N])
    print(f"softmax N={N} ld={ld} scale={scale}: max ulp {int(d.max())}, off {(d > 0).float().mean().item():.4f}")
    assert int(d.max()) <= E.SOFTMAX_BOUND_ULP


# ---- layout kernels -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,C,h,w", [(1, 16, 1, 1), (3, 16, 5, 7), (2, 8, 3, 11), (1, 24, 9, 13)])
def test_vae_unscale_cl_sizes_off_the_block(T, C, h, w):
    assert (T * C * h * w) % 256 != 0
    z = (E._codes((T, C, h, w), 3) * 0.37).to(bf)
    mean = (E._codes((C,), 5) * 0.11).to(bf)
    inv_std = (1.0 / (1.0 + E._codes((C,), 7).abs() * 0.3)).to(bf)
    want = (z / inv_std.view(1, -1, 1, 1) + mean.view(1, -1, 1, 1)).permute(0, 2, 3, 1).contiguous()
    out = _nan_bf16(T * h * w + 1, C)
    _run("ll_vae_unscale_cl", z.to(DEV), mean.to(DEV), inv_std.to(DEV), out, T, C, h, w)
    torch.cuda.synchronize()
    assert _untouched(out[T * h * w:])
    assert torch.equal(out[:T * h * w].cpu().view(T, h, w, C), want)


@pytest.mark.parametrize("T,H,W,ldc", [(1, 1, 1, 3), (2, 6, 7, 3), (1, 9, 29, 8), (3, 5, 17, 16)])
def test_cl_to_tchw_clamp_strides_and_the_clamp_edges(T, H, W, ldc):
    assert (T * H * W) % 256 != 0
    vals = torch.tensor([-1.0, 1.0, -1.0078125, 1.0078125, -0.99609375, 0.99609375, 0.0, -3.0, 5.0, 0.5])
    x = vals[(torch.arange(T * H * W * ldc) * 7) % len(vals)].view(T, H, W, ldc).to(bf)
    out = torch.full((T * 3 * H * W + 4,), float("nan"), dtype=torch.float32, device=DEV)
    _run("ll_cl_to_tchw_clamp", x.to(DEV), out, T, H, W, ldc)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[T * 3 * H * W:]).all())
    assert torch.equal(out[:T * 3 * H * W].cpu().view(T, 3, H, W), x[..., :3].float().clamp(-1, 1).permute(0, 3, 1, 2))
