"""Shared data constructions of the quantised-mode GPU tests (plain helpers, no tests): exact operands whose every fp32 sum is exact,
the bf16 epilogue tails on a bias output, hard quantiser inputs, and the unit softmax scale of the exact-data attention tests."""
import numpy as np
import torch

bf = torch.bfloat16


def exact_operands(M, N, K, seed):
    """Small-integer codes (exact in e4m3 and in int8) and power-of-two scales: every product and every fp32 sum is exact."""
    g = torch.Generator().manual_seed(seed)
    cx = torch.randint(-4, 5, (M, K), generator=g).float()
    cw = torch.randint(-4, 5, (N, K), generator=g).float()
    cw[:, 0] += torch.arange(N) % 3
    sx = torch.pow(2.0, torch.randint(-9, -3, (M,), generator=g).float())
    sw = torch.pow(2.0, torch.randint(-9, -3, (N,), generator=g).float())
    return cx, cw, sx, sw


def codes_and_scales(rows, K, seed, asym):
    """Small-integer code values (-2 .. 2, exact in E2M1 and E2M3) and a distinct power-of-two exponent per (row, K-block)."""
    g = torch.Generator().manual_seed(seed)
    c = torch.randint(-2, 3, (rows, K), generator=g).double()
    if asym:
        c[:, 0] = (torch.arange(rows) % 3).double()                     # W is not X's pattern transposed
    r, b = torch.arange(rows).view(rows, 1), torch.arange(K // 32).view(1, -1)
    ex = ((r * (5 if asym else 3) + b * (3 if asym else 5)) % 7) - 3
    return c, ex, c * torch.pow(2.0, ex.double()).repeat_interleave(32, 1)


def epi_tail(v, epi, res=None, e=None, mod=None, gate_idx=0, fs=1):
    """The epilogue tails (include/longlive_hip.h LL_EPI_*) on the bf16 bias output v."""
    if epi == 0:
        return v
    if epi == 1:
        return torch.nn.functional.gelu(v, approximate="tanh")
    if epi == 3:
        return (res.float() + v.float()).to(bf)
    B, F = e.shape[:2]
    gate = e[:, :, gate_idx] if mod is None else (mod[gate_idx].float() + e[:, :, gate_idx].float()).to(bf)
    gv = (v.view(B, F, fs, -1).float() * gate.float().unsqueeze(2)).to(bf).reshape(v.shape)
    return (res.float() + gv.float()).to(bf)


def epi_ref(acc, bias, epi, *tail, **kw):
    """The bf16 epilogues' rounding points on the fp64 accumulator (ll_gemm_bf16): the bias output, then its tail."""
    return epi_tail((acc.float() + bias.float()).to(bf), epi, *tail, **kw)


def within_1ulp(got, want):
    """Every element within 1 bf16 ulp of want, or within 2^-8 of want's RMS (elements near zero)."""
    from util import bf16_ulp_distance
    d = bf16_ulp_distance(got.cpu(), want)
    atol = want.float().pow(2).mean().sqrt().item() * 2 ** -8
    return bool(((d <= 1) | ((got.cpu().float() - want.float()).abs() <= atol)).all())


def hard_x_mx(rows, K, seed):
    """Gaussian rows with x100 outlier channels, a few all-zero blocks, and blocks of tiny values next to a large one (codes in the
    e4m3 subnormal range) or entirely tiny (bf16 subnormals, exponent clamped)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, K, generator=g)
    x[:, torch.randperm(K, generator=g)[:4]] *= 100
    x[::97, 32:64] = 0
    x[1::89, 64:96] *= 2.0 ** -14
    x[1::89, 64] = 300.0
    x[2::83, 96:128] = 2.0 ** -132 * torch.randint(-3, 4, (len(range(2, rows, 83)), 32), generator=g)
    return x.to(bf)


def hard_x_f8(rows, K, seed):
    """Gaussian rows with x100 outlier channels, all-zero rows, rows of values in the e4m3 subnormal range beside one large value,
    tiny rows, negative zeros."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, K, generator=g)
    x[:, torch.randperm(K, generator=g)[:4]] *= 100
    x[::97] = 0
    x[1::89] *= 2.0 ** -14
    x[1::89, 5] = 300.0
    x[2::83] *= 2.0 ** -40
    x[3::79, :64] = -0.0
    return x.to(bf)


def unit_c_scale():
    """A softmax scale with float32(scale * log2 e) == 1 exactly (the kernel's c), so integer scores give P = 2^integer."""
    s = np.float32(1.0 / 1.4426950408889634)
    for _ in range(8):
        if np.float32(s) * np.float32(1.4426950408889634) == np.float32(1.0):
            return float(s)
        s = np.nextafter(s, np.float32(1.0))
    raise AssertionError("no unit scale")
