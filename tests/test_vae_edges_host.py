"""The constructions of tests/test_vae_edges_gpu.py and tests/test_t5_edges_gpu.py (tests/vae_exact.py), proved on the host.

Convolution: the data is exact (the constructor asserts the bounds; here two fp32 accumulation orders -- the implicit GEMM's (tap,
channel) and the halo kernel's (kt, slice, kh, kw) -- reproduce the fp64 sums), an impulse gives the weight stencil and nothing else,
and each deliberate mutation of the fp64 reference -- a tap read from the neighbouring pixel at one seam pixel, the two history
frames swapped, zero padding replaced by edge replication at one border, upsample parity flipped on one row, one channel slice
skipped -- changes at least one bit of the expected tensor.  ll_conv_plan (host only) names the kernel instance each GPU case was
written for.

Row softmax: torch's fp32 softmax rounded to bf16 is within SOFTMAX_REF_ULP of the fp64 softmax rounded once.

umT5 attention: for every geometry the fp64 evaluation equals the construction's expected values, oracle.ref_t5.attention itself is
inside T5_BOUND_ULP (measured: at most 1.25 ulp), and one key more / fewer in the mask or a bias offset moved by one moves an element
by >= 8 x the bound wherever the construction has a row that can see it (smallest multiple measured over all cases: 64.6).  Mutations are applied to the host reference only."""
import ctypes

import pytest
import torch

import vae_exact as E
from util import bf16_ulp_distance

bf = E.bf

HOST_CONV = [   # (T, H, W, Cin, Cout, KT, KH, up): one of every tap shape and decode mode, small enough for seconds on the host
    (2, 5, 6, 8, 8, 3, 3, False), (2, 4, 5, 16, 24, 3, 1, False), (1, 6, 7, 56, 40, 1, 3, False), (2, 3, 3, 32, 16, 1, 1, False),
    (3, 6, 5, 72, 96, 3, 3, False), (1, 17, 33, 64, 96, 3, 3, False), (2, 4, 6, 96, 96, 1, 3, True), (1, 5, 3, 32, 8, 1, 3, True),
    (1, 16, 32, 160, 96, 3, 3, False),
]


def _bits(t):
    return t.contiguous().view(torch.int16)


@pytest.mark.parametrize("geom", HOST_CONV, ids=str)
def test_conv_data_is_exact_in_both_kernel_orders(geom):
    T, H, W, Cin, Cout, KT, KH, up = geom
    d = E.ConvData(*geom, seed=3)
    xin, w = E.conv_input(d.frames, KH, up).float(), d.w.float()
    # (tap, channel) order: one fp32 conv3d; (kt, slice, kh, kw): partial convolutions summed in fp32
    y = torch.nn.functional.conv3d(xin, w)[0].permute(1, 2, 3, 0)
    assert torch.equal(y.double(), d.acc)
    part = torch.zeros_like(y)
    sl = min(32, Cin)
    for kt in range(KT):
        for s in range(0, Cin, sl):
            for kh in range(KH):
                for kw in range(KH):
                    xs = xin[:, s:s + sl, kt:kt + T, kh:kh + d.Ho, kw:kw + d.Wo]
                    part += torch.einsum("cthw,oc->thwo", xs[0], w[:, s:s + sl, kt, kh, kw])
    assert torch.equal(part.double(), d.acc)
    assert torch.equal((y + d.bias.float()).to(bf), d.want)
    assert torch.equal((d.res.float() + d.want.float()).to(bf), d.want_res)
    assert d.want.float().abs().max() > 0 and not torch.equal(d.want, d.want_res)


@pytest.mark.parametrize("geom", HOST_CONV, ids=str)
def test_conv_mutations_change_the_expected_bits(geom):
    T, H, W, Cin, Cout, KT, KH, up = geom
    d = E.ConvData(*geom, seed=3)

    def want(acc):
        return (acc + d.bias).float().to(bf)

    # a tap read from the neighbouring pixel, at one pixel beside the first tile seam the image has (or its last pixel)
    t, h, x = T - 1, min(15, d.Ho - 1), min(31, d.Wo - 1)
    assert torch.equal(E.conv_pixel_host(d.frames, d.w, KT, KH, up, t, h, x), d.acc[t, h, x])
    if d.Wo > 1:
        x = min(x, d.Wo - 2)
        mut = E.conv_pixel_host(d.frames, d.w, KT, KH, up, t, h, x, shift_tap=(KT - 1, KH // 2, 0))
        assert not torch.equal(_bits(want(mut)), _bits(d.want[t, h, x]))
    if KT == 3:
        swapped = d.frames.clone()
        swapped[0], swapped[1] = d.frames[1], d.frames[0]
        assert not torch.equal(_bits(want(E.conv_host(swapped, d.w, KT, KH, up))), _bits(d.want))
    if KH == 3:
        assert not torch.equal(_bits(want(E.conv_host(d.frames, d.w, KT, KH, up, replicate_left=True))), _bits(d.want))
    if up and H > 1:
        for r in (1, d.Ho - 2):
            assert not torch.equal(_bits(want(E.conv_host(d.frames, d.w, KT, KH, up, flip_row=r))), _bits(d.want))
    for s in range(max(1, Cin // 32)):
        w2 = d.w.clone()
        w2[:, 32 * s:32 * s + 32, KT - 1] = 0.0
        assert not torch.equal(_bits(want(E.conv_host(d.frames, w2, KT, KH, up))), _bits(d.want))


@pytest.mark.parametrize("geom,pos", [((3, 17, 33, 16, 8, 3, 3, False), (0, 0, 0)), ((3, 17, 33, 16, 8, 3, 3, False), (1, 16, 32)),
                                      ((2, 17, 33, 64, 16, 3, 3, False), (1, 15, 31)), ((1, 9, 17, 32, 8, 1, 3, True), (0, 7, 15)),
                                      ((2, 6, 6, 8, 8, 3, 1, False), (0, 5, 0)), ((1, 6, 6, 8, 8, 1, 1, False), (0, 3, 3))], ids=str)
def test_impulse_gives_the_weight_stencil_and_nothing_else(geom, pos):
    T, H, W, Cin, Cout, KT, KH, up = geom
    d = E.ConvData(*geom, seed=5, impulse=pos, zero_bias=True, hist="zero")
    t, h, x = pos
    px = d.frames[d.nh + t, h, x]
    lit = (d.acc != 0).any(-1)
    if up:
        assert int(lit.sum()) <= 16 and lit[t, max(2 * h - 1, 0):2 * h + 3, max(2 * x - 1, 0):2 * x + 3].any()
        assert not lit[t, :max(2 * h - 1, 0)].any() and not lit[t, 2 * h + 3:].any()
        return
    p, seen = KH // 2, 0
    for kt in range(KT):
        for kh in range(KH):
            for kw in range(KH):
                to, ho, wo = t + KT - 1 - kt, h + p - kh, x + p - kw
                if 0 <= to < T and 0 <= ho < H and 0 <= wo < W:
                    assert torch.equal(d.acc[to, ho, wo], d.w[:, :, kt, kh, kw] @ px)
                    seen += 1
    assert int(lit.sum()) <= seen


def test_rms_reference_clamp_is_the_bf16_value():
    """F.normalize clamps the bf16 norm with eps = 1e-12 converted to the tensor's dtype; the kernels clamp with that bf16 value."""
    c = torch.zeros(1, dtype=bf).clamp_min(1e-12).float().item()
    assert c == torch.tensor(1e-12).to(bf).float().item()


def test_conv_plan_names_the_instance_of_every_gpu_case():
    """ll_conv_plan is host only: every GPU case's expected instance is checked here too, under the tuning the case runs with."""
    import test_vae_edges_gpu as G
    from longlive_amd import _lib as L
    lib = L.load()
    buf = ctypes.create_string_buffer(512)
    n = 0
    try:
        for halo_key, cases in ((0, G.CL_CASES), (1, G.HALO_CASES + G.THRESHOLD_CASES)):
            assert lib.ll_set_tuning(b"conv_halo", halo_key) == 0
            for c in cases:
                g = c[0]
                L.check(lib.ll_conv_plan(g[0], g[1], g[2], g[3], g[4], g[5], g[6], int(g[7]), 0, 0, buf, 512), "ll_conv_plan")
                assert buf.value.decode().startswith(G.instance(c)), (c, buf.value.decode())
                n += 1
    finally:
        lib.ll_set_tuning(b"conv_halo", 1)
    assert n == len(G.CL_CASES) + len(G.HALO_CASES) + len(G.THRESHOLD_CASES) >= 75
    # rejected like the launch itself; the fused form only where ll_conv_cl_rms_ok
    assert lib.ll_conv_plan(1, 16, 32, 12, 96, 3, 3, 0, 0, 0, buf, 512) == -1
    assert lib.ll_conv_plan(1, 16, 32, 96, 192, 3, 3, 0, 0, 1, buf, 512) == -1
    assert lib.ll_conv_plan(1, 16, 32, 96, 96, 3, 3, 0, 0, 0, None, 0) == -1
    L.check(lib.ll_conv_plan(2, 30, 52, 96, 96, 3, 3, 0, 1, 1, buf, 512), "ll_conv_plan")
    assert buf.value.decode().startswith("conv_halo_kernel<bias_res, NCB 6, UP 0, RMS 1> tile 16x32 pixels x 96 channels, 8 workgroups (2 frames x 2 x 2 tiles x 1 n-tiles)")


@pytest.mark.parametrize("N,ld,scale", E.SOFTMAX_SHAPES)
def test_softmax_reference_side_of_the_bound(N, ld, scale):
    s = E.softmax_rows_data(max(9, min(256, 60000 // N)), N, ld, N)
    d = bf16_ulp_distance(E.softmax_torch32(s, N, scale), E.softmax_host(s, N, scale))
    print(N, ld, scale, "max ulp", int(d.max()), "fraction off", (d > 0).float().mean().item())
    assert int(d.max()) <= E.SOFTMAX_REF_ULP
    assert (d > 0).float().mean().item() < 0.001


T5_MULTIPLE = 8


@pytest.mark.parametrize("L,H,n,rot", E.T5_CASES, ids=str)
def test_t5_constructions(L, H, n, rot):
    """Measured over all cases: the oracle's own path is at most 0.62 x the bound (1.25 ulp) from the construction; every visible mutation
    moves an element by >= 64.6 x the bound; invisible ones (seq_len = 1: every output is V[0]; a bias offset whose keys lie outside
    the mask on either side) move nothing at all.  Cases of 64 heads are evaluated on heads 0 .. 2 (heads are independent and the data
    of a head depends on its own index only)."""
    case = E.T5Case(L, H, n, rot, heads=list(range(min(H, 3))))
    hs = case.heads
    exp = case.expected()
    bound = case.bound(exp)
    host = case.host()
    nz = exp != 0
    err = (host - exp).abs()
    assert (err[:, hs] <= bound[:, hs]).all() and (err[:, hs][nz[:, hs]] <= (bound / 64)[:, hs][nz[:, hs]]).all()
    orc = case.oracle()
    oerr = ((orc - exp).abs() / bound)[:, hs]
    assert oerr.max() <= 1.0, oerr.max()
    print((L, H, n, rot), "oracle / bound", oerr.max().item())
    worst = {}
    for name, kw in (("more", dict(seq_len=n + 1)), ("fewer", dict(seq_len=n - 1)), ("shift+", dict(shift=1)), ("shift-", dict(shift=-1))):
        if (name == "more" and n == L) or (name == "fewer" and n == 1):
            continue
        moved = (((case.host(**kw) - exp).abs() / bound)[:, hs]).max().item()
        # the construction's own statement of the mutated result agrees with the fp64 evaluation of it
        mexp = case.expected(**kw)
        assert ((mexp - case.host(**kw)).abs()[:, hs] <= case.bound(mexp)[:, hs]).all()
        worst[name] = moved
        assert moved >= T5_MULTIPLE or moved < 1e-6, (name, moved)
    print("  mutations / bound", worst)
    assert any(m >= T5_MULTIPLE for m in worst.values())


def test_t5_every_offset_class_sees_a_shift_somewhere():
    """For every L and every required offset the unmasked case (seq_len = L, one head) sees the bias offset moved by one either way."""
    for L in (64, 128, 256, 512):
        for r, d in enumerate(E.T5_OFFSETS(L)[:5]):
            assert (L, 1, L, r) in E.T5_CASES and d in (-(L - 1), -1, 0, 1, L - 1)
            case = E.T5Case(L, 1, L, r)
            exp = case.expected()
            for shift in (1, -1):
                assert (((case.host(shift=shift) - exp).abs() / case.bound(exp)).max().item()) >= T5_MULTIPLE, (L, d, shift)
