"""The VAE encoder's kernels (csrc/conv.hip: ll_conv_cl_down, ll_conv_cl_tdown, ll_pixels_to_cl, ll_vae_scale_tchw) at their tile
and border edges, through the C ABI with explicit pointers, on the constructions of tests/vae_exact.py (tests/vae_enc_exact.py adds
the strided references).

Exact data: every fp32 sum is exact in any order, so the output has ONE correct bit pattern, the fp64 F.conv2d / F.conv3d result +
bias rounded once; compared with torch.equal.  Every case asserts from ll_conv_down_plan the kernel instance it was written for, puts
its input between NaN guard frames (for the temporal form the guard sits TWO frames before x: the one frame before x is the history
the contract allows), and writes rows of ldo > Cout into a field of NAN16 whose other bits must survive."""
import ctypes

import pytest
import torch

import vae_enc_exact as X
import vae_exact as E
from util import bf

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN16 = E.NAN16


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


def _plan(kind, T, H, W, Cin, Cout):
    L, lib = _lib()
    buf = ctypes.create_string_buffer(512)
    L.check(lib.ll_conv_down_plan(kind, T, H, W, Cin, Cout, buf, 512), "ll_conv_down_plan")
    return buf.value.decode()


def _instance(kind, Cin, Cout):
    nt = 1 if Cout <= 32 else 3 if (Cout % 96 == 0 and Cout % 128 != 0) else 4
    mode = (5 if Cin < 64 else 4) if kind else (6 if Cin < 64 else 3)
    return f"conv_cl_kernel<bias, NT {nt}, MODE {mode}>"


def _launch(d, pad):
    """One launch on DownData d; returns out [M, Cout] after checking the plan, the guards and every sentinel."""
    assert _plan(d.kind, d.T, d.H, d.W, d.Cin, d.Cout).startswith(_instance(d.kind, d.Cin, d.Cout)), _plan(d.kind, d.T, d.H, d.W, d.Cin, d.Cout)
    G = 1
    buf = torch.full((G + d.nh + d.T + G, d.H, d.W, d.Cin), float("nan"), dtype=bf, device=DEV)
    buf[G:G + d.nh + d.T] = d.frames.to(bf).to(DEV)
    x = buf[G + d.nh]
    zero = torch.zeros(32, dtype=bf, device=DEV)
    ldo = d.Cout + pad
    out = _nan_bf16(d.M + 3, ldo)
    _run("ll_conv_cl_tdown" if d.kind else "ll_conv_cl_down", x, zero, d.packed_w().to(DEV), d.bias.to(bf).to(DEV), out, d.T, d.H, d.W,
         d.Cin, d.Cout, d.Kpad, ldo)
    torch.cuda.synchronize()
    assert _untouched(out[d.M:]) and _untouched(out[:d.M, d.Cout:]), f"wrote outside [M, Cout] (ldo {ldo})"
    assert bool(torch.isnan(buf[:G].float()).all()) and bool(torch.isnan(buf[-G:].float()).all())
    return out[:d.M, :d.Cout]


def _check(d, got, what):
    want = d.want.view(d.M, d.Cout).to(DEV)
    if not torch.equal(got, want):       # a guard frame that was read shows as NaN here
        bad = (got.view(torch.int16) != want.view(torch.int16)).any(-1).nonzero().flatten()
        px = [(int(m) // (d.Ho * d.Wo), int(m) % (d.Ho * d.Wo) // d.Wo, int(m) % d.Wo) for m in bad[:12]]
        raise AssertionError(f"{what}: {len(bad)} of {d.M} pixels differ, first (t, h, w) {px}; got {got[bad[0]][:6].tolist()} want {want[bad[0]][:6].tolist()}")


# (T, H, W, Cin, Cout): every Cin of the issue (72: K = 648 is no multiple of 64), Cout 8 .. 384 over every n-tiling (NT 1: <= 32; NT 3:
# 96, 192; NT 4: the rest, 160 = a partial second n-tile), M = 1, odd / even sizes, 255 / 256 / 257 output pixels, T 1 .. 3
DOWN = [(1, 2, 2, 64, 8), (3, 3, 3, 72, 32), (2, 4, 5, 96, 96), (2, 5, 4, 192, 192), (1, 15, 26, 384, 384), (1, 16, 26, 96, 64),
        (3, 17, 33, 72, 128), (1, 30, 34, 96, 96), (1, 32, 32, 192, 40), (1, 2, 514, 96, 96), (2, 16, 26, 384, 96), (3, 3, 3, 64, 16),
        (1, 17, 33, 192, 384), (2, 15, 26, 96, 192), (1, 4, 5, 384, 8), (2, 30, 34, 64, 160),
        (2, 5, 5, 16, 96), (1, 4, 4, 32, 8)]                                     # Cin < 64: the per-lane decode (MODE 6)


@pytest.mark.parametrize("case", DOWN, ids=lambda c: "x".join(map(str, c)))
def test_conv_down_exact(case):
    T, H, W, Cin, Cout = case
    d = X.DownData(0, T, H, W, Cin, Cout, seed=3 + H + W)
    if (H, W) == (30, 34):
        assert d.Ho * d.Wo == 255
    if (H, W) == (2, 514):
        assert d.Ho * d.Wo == 257
    _check(d, _launch(d, 4 if Cout % 16 else 8), f"down {case}")


@pytest.mark.parametrize("H,W", [(4, 6), (5, 7)])
@pytest.mark.parametrize("where", ["last_row", "last_col", "corner", "origin"])
def test_conv_down_impulse_tells_the_asymmetric_pad(H, W, where):
    """A lone pixel: with the pad on the right / bottom and the stride origin at 0, input pixel (h, w) reaches output (h // 2 - (h odd
    or h == 2 Ho), ...) only through tap (h - 2 ho, w - 2 wo); a symmetric pad or an origin off by one moves it to another tap, whose
    channel-0 code differs by whole integers."""
    h, w = {"last_row": (H - 1, 2), "last_col": (2, W - 1), "corner": (H - 1, W - 1), "origin": (0, 0)}[where]
    d = X.DownData(0, 2, H, W, 96, 96, seed=11, impulse=(1, h, w))
    got = _launch(d, 4)
    _check(d, got, f"impulse {where} {H}x{W}")
    g = got.view(d.To, d.Ho, d.Wo, d.Cout).double().cpu()
    hit = {}
    for ho in range(d.Ho):
        for wo in range(d.Wo):
            kh, kw = h - 2 * ho, w - 2 * wo
            if 0 <= kh < 3 and 0 <= kw < 3:
                hit[(ho, wo)] = d.w[:, :, kh, kw] @ d.px
    assert hit and (where != "origin" or list(hit) == [(0, 0)])
    for ho in range(d.Ho):
        for wo in range(d.Wo):
            want = d.bias + hit.get((ho, wo), 0.0)
            assert torch.equal(g[1, ho, wo], want.float().to(bf).double()), (ho, wo)
    assert torch.equal(g[0], d.bias.float().to(bf).double().expand_as(g[0]))    # the other frame sees nothing
    sym = X.down_host(0, d.frames, d.w, pad=(1, 0, 1, 0))                      # the mutation this case exists for gives other integers
    assert not torch.equal(sym, d.acc)


# (T_in, H, W, Cin, Cout)
TDOWN = [(2, 3, 3, 192, 192), (4, 5, 4, 384, 384), (6, 9, 7, 192, 96), (8, 4, 5, 384, 8), (4, 2, 2, 192, 384), (2, 16, 17, 384, 64),
         (2, 16, 17, 32, 64), (8, 8, 8, 16, 32), (6, 3, 5, 56, 160)]          # Cin < 64: MODE 5; 16 x 17 = 272 pixels: two m-tiles


@pytest.mark.parametrize("case", TDOWN, ids=lambda c: "x".join(map(str, c)))
def test_conv_tdown_exact(case):
    T, H, W, Cin, Cout = case
    d = X.DownData(1, T, H, W, Cin, Cout, seed=5 + T + H)
    _check(d, _launch(d, 4 if Cout % 16 else 8), f"tdown {case}")


@pytest.mark.parametrize("Cin", [192, 32])
@pytest.mark.parametrize("f,taps", [(0, {0: 0}), (4, {1: 2, 2: 0}), (3, {1: 1}), (2, {1: 0, 0: 2}), (6, {2: 2})])
def test_conv_tdown_impulse_reaches_the_right_frames(Cin, f, taps):
    """frames index f = input frame f - 1 (f = 0: the history frame).  taps = {output frame j: temporal tap kt} it must reach, and
    nothing else: history -> out[0] through tap 0; frame 2j -> out[j] tap 1; an odd frame 2j - 1 = 2(j - 1) + 1 -> out[j] tap 0 and
    out[j - 1] tap 2 (f = 2, f = 4); the last frame T - 1 = 2j + 1 -> out[j] tap 2 only, there being no out[j + 1] (f = 6)."""
    d = X.DownData(1, 6, 3, 4, Cin, 96, seed=9, impulse=(f, 1, 2))
    got = _launch(d, 4)
    _check(d, got, f"tdown impulse frame {f - 1}")
    resp = got.view(d.To, d.H, d.W, d.Cout).double().cpu()
    for j in range(d.To):
        for h in range(d.H):
            for w in range(d.W):
                want = d.bias.clone()
                if (h, w) == (1, 2) and j in taps:
                    want = want + d.w[:, :, taps[j], 0, 0] @ d.px
                assert torch.equal(resp[j, h, w], want.float().to(bf).double()), (j, h, w)
    assert not torch.equal(X.down_host(1, torch.cat([d.frames, d.frames[-1:]]), d.w, origin=1), d.acc)


# ---- layout kernels -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, bf], ids=["f32", "bf16"])
@pytest.mark.parametrize("cdim", [0, 1], ids=["cthw", "tchw"])
@pytest.mark.parametrize("T,H,W,cpad", [(1, 3, 5, 8), (3, 8, 7, 32), (3, 3, 33, 16), (2, 17, 31, 8)])
def test_pixels_to_cl_bit_exact(dtype, cdim, T, H, W, cpad):
    """Values that do not fit bf16 (fp32 input is rounded once, to nearest even), both layouts, odd W, a strided view in time; the pad
    channels are zero and nothing is written past the last pixel."""
    n = 3 * (T + 2) * H * W
    v = (E.hash_bits(torch.arange(n, dtype=torch.int64), 77) % 200001).double() / 100000.0 - 1.0
    full = v.view(3, T + 2, H, W) if cdim == 0 else v.view(T + 2, 3, H, W)
    full = full.to(dtype).to(DEV)
    px = full.narrow(1 - cdim, 1, T)                                            # frames 1 .. T of a longer clip: strides, not a copy
    out = _nan_bf16(T * H * W + 2, cpad)
    _run("ll_pixels_to_cl", px, 1 if dtype == torch.float32 else 0, px.stride(cdim), px.stride(1 - cdim), out, T, H, W, cpad)
    torch.cuda.synchronize()
    assert _untouched(out[T * H * W:])
    got = out[:T * H * W].view(T, H, W, cpad).cpu()
    want = (px.cpu() if cdim == 1 else px.cpu().permute(1, 0, 2, 3)).to(bf).permute(0, 2, 3, 1)      # [T, H, W, 3]
    assert torch.equal(got[..., :3], want)
    assert bool((got[..., 3:].view(torch.int16) == 0).all())


def test_ops_pixels_to_cl_takes_views_and_both_layouts():
    from longlive_amd import ops as O
    x = torch.rand(2, 3, 5, 8, 9, device=DEV) * 2 - 1
    a = O.pixels_to_cl(x[1], 0, 8)
    b = O.pixels_to_cl(x[1].permute(1, 0, 2, 3), 1, 8)
    assert torch.equal(a, b) and torch.equal(a[..., :3], x[1].to(bf).permute(1, 2, 3, 0))


@pytest.mark.parametrize("T,h,w,ld", [(1, 1, 1, 16), (3, 8, 12, 16), (2, 7, 13, 24), (5, 60, 104, 16)])
def test_vae_scale_tchw_bit_exact(T, h, w, ld):
    from longlive_amd.vae import VAE_MEAN, VAE_STD
    mean = torch.tensor(VAE_MEAN).to(bf)
    inv_std = 1.0 / torch.tensor(VAE_STD).to(bf)                                 # utils/wan_wrapper.py:83-84 in bf16
    n = T * h * w * ld
    mu = ((E.hash_bits(torch.arange(n, dtype=torch.int64), 31) % 16001).double() / 1000.0 - 8.0).view(T, h, w, ld).to(bf)
    out = torch.full((T * 16 * h * w + 8,), float("nan"), dtype=torch.float32, device=DEV)
    _run("ll_vae_scale_tchw", mu.to(DEV), mean.to(DEV), inv_std.to(DEV), out, T, 16, h, w, ld)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[T * 16 * h * w:]).all())
    m = mu[..., :16].permute(0, 3, 1, 2)
    want = ((m - mean.view(1, 16, 1, 1)) * inv_std.view(1, 16, 1, 1)).float()    # vae.py:537-539 under bf16, then .float()
    assert want.dtype == torch.float32 and torch.equal(out[:T * 16 * h * w].view(T, 16, h, w).cpu(), want)
