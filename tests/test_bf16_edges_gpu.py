"""The bf16 GEMMs and attention kernels at their shape and stride edges, through the C ABI with explicit strides (the ops.* wrappers
always pass ldx = K, ldo = N, ldq = ldo = ldk = H * 128).

GEMMs run on exact data (tests/bf16_exact.py: every fp32 sum is exact in any order, so the bf16 output has ONE correct bit pattern)
and are compared with torch.equal against the fp64 host result and between kernel families -- the generated classic and persistent
kernels, split-K with both reduce kernels, the sum-of-squares form, the fused QKV form and each HIP tiling; only GELU keeps the
project's 2 ulp / 97 % bound against torch (its v_exp / v_rcp form is not bit-defined).  X padding columns hold NaN, `out` is a NaN
field the kernels may only write inside [M, N], workspaces carry guard words.

Attention runs the gather and uniform constructions of tests/bf16_exact.py, whose expected outputs are integers / exact means and
which tests/test_bf16_edges_host.py proves sensitive to one wrongly admitted or dropped key.  Tolerance: 2 bf16 ulp of the expected
element (the oracle's own bf16 path measures <= 0.51 ulp from the expected values on the host) with an absolute floor of
nkeys 2^-30 64 where the expected value is zero.

Every case asserts the kernel family it is about to run from the plan text; every test leaves the shipped tuning behind."""
import ctypes
import math
import re

import pytest
import torch
import torch.nn.functional as Fn

import bf16_exact as E
from bf16_exact import lib as _lib
from bf16_exact import nan_bf16 as _nan_bf16
from bf16_exact import run as _run
from bf16_exact import untouched_bf16 as _untouched_bf16
from quant_exact import epi_tail
from util import bf, bf16_ulp_distance

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN16 = E.NAN16
BIAS, GELU, GATE, RES = 0, 1, 2, 3
SHIPPED = {"gemm_asm": 35, "gemm_variant": 0, "gemm_variant_wide": 0, "gemm_group_m": 4, "gemm_lds_epi": 1, "attn_asm": 1,
           "attn_variant": 2, "attn_xcd": 1, "attn_asm_min_keys": 512, "attn_pp_min_keys": 1024}
SCALE = 1.0 / math.sqrt(128)


# ---- plumbing -------------------------------------------------------------------------------------------------------------------------
def _tune(**kv):
    L, lib = _lib()
    for k, v in kv.items():
        L.check(lib.ll_set_tuning(k.encode(), int(v)), "ll_set_tuning")


@pytest.fixture(autouse=True)
def _shipped_tuning():
    _tune(**SHIPPED)
    yield
    _tune(**SHIPPED)


def _text(fn, *args):
    L, lib = _lib()
    buf = ctypes.create_string_buffer(512)
    L.check(getattr(lib, fn)(*args, buf, 512), fn)
    return buf.value.decode()


def _plan_epi(M, N, K, epi, plain=1):
    return _text("ll_gemm_plan_epi", M, N, K, 0, epi, plain)


def _attn_plan(B, Lq, H, n0, n1=0, adjacent=0):
    return _text("ll_flash_attn_plan", Lq, H, B, n0, n1, adjacent)


def _assert_gelu_close(got, want, what):
    """tests/util.assert_bf16_close(got, want, 2, 0.97) of test_gemm_epilogues, evaluated on the device."""
    assert torch.isfinite(got.float()).all(), f"{what}: non-finite output"
    d = bf16_ulp_distance(got, want)
    atol = want.float().pow(2).mean().sqrt().item() * 2 ** -8
    bad = int(((d > 2) & ((got.float() - want.float()).abs() > atol)).sum())
    exact = (d == 0).float().mean().item()
    assert bad == 0, f"{what}: {bad} elements off by > 2 ulp and > {atol:.2e}"
    assert exact >= 0.97, f"{what}: only {exact:.4f} of elements bit-exact"


class Data:
    """A GemmData set with its device copies, a residual and the GELU reference of the bias output (torch tanh-GELU on the host; the
    sets with a GELU case are the O(1) form, see GemmData)."""
    _cache = {}

    def __init__(self, M, N, K, seed, unit=False, gelu=False):
        d = E.GemmData(M, N, K, seed, unit, o1=gelu)
        self.M, self.N, self.K, self.d = M, N, K, d
        self.x, self.w, self.b, self.want = d.x.to(DEV), d.w.to(DEV), d.bias.to(DEV), d.want.to(DEV)
        g = torch.Generator().manual_seed(seed + 5)
        self.res = (torch.randint(-40, 41, (M, N), generator=g).float() * 2.0 ** -3).to(bf).to(DEV)
        self.gelu = Fn.gelu(d.want, approximate="tanh").to(DEV) if gelu else None

    @classmethod
    def get(cls, M, N, K, unit=False, gelu=False):
        key = (M, N, K, unit, gelu)
        if key not in cls._cache:
            if len(cls._cache) > 2:
                cls._cache.clear()
            cls._cache[key] = cls(M, N, K, N + K, unit, gelu)
        return cls._cache[key]


def _gemm(D, M, epi=BIAS, ldx=None, ldo=None, alias=False, e=None, mod=None, gate_idx=0, rpb=0, fl=0, fn="ll_gemm_bf16", tail=None):
    """One call on the first M rows: X [M, ldx] with NaN beyond K, out [M + 3, ldo] a NaN field, res [M, ldo] (or out itself).  Checks
    the sentinels and returns out[:M, :N].  tail(res) = the entry point's arguments after ldo, where they are not ll_gemm_bf16's."""
    N, K = D.N, D.K
    ldx, ldo = ldx or K, ldo or N
    x = _nan_bf16(M, ldx)
    x[:, :K] = D.x[:M]
    out = _nan_bf16(M + 3, ldo)
    res = None
    if epi in (GATE, RES):
        res = out if alias else _nan_bf16(M, ldo)
        res[:M, :N] = D.res[:M]
    nmod = 0 if e is None else e.shape[-2]
    tail = tail(res) if tail is not None else (epi, res, e, mod, nmod, gate_idx, rpb, fl)
    _run(fn, x, D.w, D.b, out, M, N, K, ldx, ldo, *tail)
    assert _untouched_bf16(out[M:]) and _untouched_bf16(out[:M, N:]), f"{fn} {M}x{N}x{K} ldo={ldo}: wrote outside [M, N]"
    return out[:M, :N]


def _family(M, N, K, epi, mod=False):
    """The kernel family gemm_asm_width() / gemm_asm_launch() give a plain call under the shipped tuning: the statement this suite
    holds the plan text against, so that a dispatch change cannot move a case to another kernel unnoticed."""
    tail = {BIAS: "bias", GELU: "gelu", GATE: "gate_res", RES: "res"}[epi]
    if K < 256 or mod:
        return "gemm_kernel_v"
    if epi == GELU:
        return "gemm_asmp?_224_gelu" if N % 224 == 0 else "gemm_kernel_v"
    if epi == BIAS and N > 2048 and N % 192 == 0:
        return "gemm_asmp?_192_bias"
    if epi == BIAS and M <= 1024 and N >= 16384 and N % 256 == 0:
        return "gemm_asm_256_bias"
    if N % 128 == 0 and (N <= 2048 or M <= 1024):
        return f"gemm_asmp?_128_{tail}"
    return "gemm_kernel_v"


def _check_vs_host(D, M, epi, got, what):
    if epi == GELU:
        _assert_gelu_close(got, D.gelu[:M], what)
    else:
        want = epi_tail(D.want[:M], epi, D.res[:M])
        assert torch.equal(got, want), f"{what}: max |diff| {(got.float() - want.float()).abs().max().item()}"


# ---- A1. the shape / stride sweep over every family ----------------------------------------------------------------------------------------
M_EDGES = (1, 63, 64, 65, 255, 256, 257, 1024, 1025, 1100, 2100)      # 1100 / 2100: 5 and 9 m-tiles, not multiples of gemm_group_m = 4
SWEEP = [
    # 128-wide generated kernels (N <= 2048; 2176 = 17 x 128: M <= 1024 generated, above that HIP), every K of the list at N = 384
    (128, 256, (BIAS, RES)), (384, 64, (BIAS, RES)), (384, 128, (BIAS,)), (384, 192, (BIAS, RES)), (384, 256, (BIAS, RES)),
    (384, 320, (BIAS, RES)), (384, 1536, (BIAS, RES)), (384, 8960, (BIAS, RES)), (2048, 256, (BIAS, RES)), (2048, 320, (BIAS,)),
    (2176, 256, (BIAS, RES)), (2176, 320, (BIAS,)),
    # 192-wide (N > 2048, N % 192 == 0, bias); with a residual these widths leave the generated kernels above M = 1024 or N % 128 != 0
    (2112, 256, (BIAS, RES)), (2304, 320, (BIAS, RES)), (4608, 256, (BIAS,)), (2304, 1536, (BIAS,)), (2304, 8960, (BIAS,)),
    # 224-wide GELU
    (224, 256, (GELU, BIAS)), (224, 8960, (GELU,)), (448, 320, (GELU,)), (448, 1536, (GELU,)), (8960, 256, (GELU,)), (448, 128, (GELU,)),
    # HIP only: N % 128 != 0 (8: one partial 8-column tile, 136: one tile + 8, 200: N % 16 == 8, 1544: a partial tile behind 12 whole ones)
    (8, 64, (BIAS, RES, GELU)), (8, 320, (BIAS,)), (136, 192, (BIAS, RES)), (136, 256, (BIAS, GELU)), (200, 256, (BIAS, RES, GELU)),
    (200, 1536, (BIAS,)), (1544, 128, (BIAS, RES)), (1544, 320, (BIAS, GELU)), (1544, 8960, (BIAS,)),
]


def _strides(N, K):
    return [(K, N), (K + 8, N + 8), (K + 64, N)]


@pytest.mark.parametrize("N,K,epis", SWEEP, ids=lambda v: str(v).replace(" ", ""))
def test_gemm_sweep_bit_exact_in_every_family(N, K, epis):
    """Every M of M_EDGES x every stride set at this (N, K): the kernel the shipped tuning picks (its family asserted from the plan),
    the classic generated kernel where that was the persistent one, and the HIP kernels (gemm_asm 0) each equal the host bit for bit
    (GELU: the 2 ulp / 97 % bound against torch, generated forms among themselves bit for bit)."""
    D = Data.get(max(M_EDGES), N, K, gelu=GELU in epis)
    for M in M_EDGES:
        for epi in epis:
            want_fam = _family(M, N, K, epi)
            for ldx, ldo in _strides(N, K):
                what = f"{M}x{N}x{K} epi {epi} ldx {ldx} ldo {ldo}"
                plan = _plan_epi(M, N, K, epi)
                assert re.match(want_fam, plan), (what, plan)
                got = _gemm(D, M, epi, ldx, ldo)
                _check_vs_host(D, M, epi, got, f"{what} [{plan.split('<')[0]}]")
                if plan.startswith("gemm_asm"):
                    try:
                        if plan.startswith("gemm_asmp"):
                            _tune(gemm_asm=3)
                            assert re.match("gemm_asm_", _plan_epi(M, N, K, epi))
                            assert torch.equal(_gemm(D, M, epi, ldx, ldo), got), f"{what}: classic vs persistent"
                        _tune(gemm_asm=0)
                        hplan = _plan_epi(M, N, K, epi)
                        assert hplan.startswith("gemm_kernel_v"), hplan
                        hip = _gemm(D, M, epi, ldx, ldo)
                    finally:
                        _tune(gemm_asm=35)
                    _check_vs_host(D, M, epi, hip, f"{what} [{hplan.split('<')[0]}]")
                    if epi != GELU:
                        assert torch.equal(hip, got), f"{what}: HIP vs generated"


@pytest.mark.parametrize("K", [256, 320, 1536, 8960])
def test_gemm_256_wide_kernel_and_its_m_boundary(K):
    """N = 16384: M <= 1024 runs gemm_asm_256_bias (1, 257: a lone row and a ragged second m-tile; 1024: the last M it takes), 1025 the
    HIP kernels, at 4, 5, 24 and 140 K-steps (the unrolled main loop leaves through a different exit for each).  Bit for bit against
    the host, at contiguous and wide strides, and against the HIP kernels."""
    N = 16384
    D = Data.get(1025, N, K)
    for M in (1, 257, 1024, 1025):
        plan = _plan_epi(M, N, K, BIAS)
        assert plan.startswith("gemm_asm_256_bias" if M <= 1024 else "gemm_kernel_v"), plan
        for ldx, ldo in _strides(N, K):
            got = _gemm(D, M, BIAS, ldx, ldo)
            assert torch.equal(got, D.want[:M]), (M, K, ldx, ldo, plan)
            try:
                _tune(gemm_asm=0)
                assert _plan_epi(M, N, K, BIAS).startswith("gemm_kernel_v")
                assert torch.equal(_gemm(D, M, BIAS, ldx, ldo), got)
            finally:
                _tune(gemm_asm=35)


# ---- A2. the HIP tilings --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,bn", [(0, 128), (2, 128), (3, 256), (5, 192), (6, 224)])
@pytest.mark.parametrize("N", [1544, 5376])
def test_gemm_hip_tilings_bit_exact(variant, bn, N):
    """gemm_asm 0 with gemm_variant 0 / 2 / 3 / 5 / 6 at a ragged N (1544: no tile width divides it) and at 5376 (a multiple of 128,
    192, 224 and 256; >= 4096, so gemm_variant_wide is exercised there too): every tiling equals the host bit for bit, at wide strides,
    with and without LDS-staged epilogues, with gemm_group_m 4 and 1."""
    K = 320
    D = Data.get(1100, N, K, gelu=True)
    try:
        _tune(gemm_asm=0, gemm_variant=variant)
        for M in (1, 257, 1100):
            plan = _text("ll_gemm_plan", M, N, K, 0)
            name = {0: "gemm_kernel_v2", 2: "gemm_kernel_v2", 3: "gemm_kernel_v5", 5: "gemm_kernel_v5", 6: "gemm_kernel_v5"}[variant]
            assert plan.startswith(name) and f"tile 256x{bn}" in plan, plan
            assert _plan_epi(M, N, K, BIAS) == plan
            for lds_epi in (1, 0, 2) if N == 1544 else (1,):
                _tune(gemm_lds_epi=lds_epi)
                for ldx, ldo in _strides(N, K):
                    for epi in (BIAS, RES, GELU):
                        got = _gemm(D, M, epi, ldx, ldo, alias=(epi == RES and ldo > N))
                        _check_vs_host(D, M, epi, got, f"v{variant} {M}x{N}x{K} epi {epi} lds_epi {lds_epi} ldx {ldx} ldo {ldo}")
        _tune(gemm_lds_epi=1, gemm_group_m=1)          # the N-fastest tile walk (tile_of with gm <= 1) of the HIP kernels
        assert "N fastest" in _text("ll_gemm_plan", 1100, N, K, 0)
        for M in (257, 1100):
            for ldx, ldo in _strides(N, K):
                for epi in (BIAS, RES):
                    _check_vs_host(D, M, epi, _gemm(D, M, epi, ldx, ldo), f"v{variant} {M}x{N}x{K} epi {epi} group_m 1 ldx {ldx} ldo {ldo}")
        _tune(gemm_group_m=4)
        if N >= 4096 and variant >= 2:
            _tune(gemm_variant=0, gemm_variant_wide=variant, gemm_lds_epi=1)
            assert f"tile 256x{bn}" in _text("ll_gemm_plan", 1100, N, K, 0)
            assert torch.equal(_gemm(D, 1100, BIAS, K + 8, N + 8), D.want[:1100])
    finally:
        _tune(**SHIPPED)


@pytest.mark.parametrize("variant,bn", [(2, 128), (3, 256), (5, 192), (6, 224)])
@pytest.mark.parametrize("K", [64, 128])
def test_gemm_hip_tilings_at_one_and_two_k_steps(variant, bn, K):
    """gemm_asm 0 with gemm_variant 2 / 3 / 5 / 6 at K = 64 and 128: one and two K-steps, so the rings have no next stage (or exactly
    one) to issue.  M = 257, N = 200: a partial n-tile in every width, and in the second m-tile only row 256 is live, so most of its
    waves take the stage-and-sync path.  Bit for bit against the host, with and without LDS-staged epilogues, at contiguous and wide
    strides."""
    M, N = 257, 200
    D = Data.get(M, N, K, gelu=True)
    try:
        _tune(gemm_asm=0, gemm_variant=variant)
        plan = _text("ll_gemm_plan", M, N, K, 0)
        assert plan.startswith("gemm_kernel_v2" if variant == 2 else "gemm_kernel_v5") and f"tile 256x{bn}" in plan, plan
        for lds_epi in (1, 0):
            _tune(gemm_lds_epi=lds_epi)
            for ldx, ldo in _strides(N, K):
                for epi in (BIAS, RES, GELU):
                    got = _gemm(D, M, epi, ldx, ldo)
                    _check_vs_host(D, M, epi, got, f"v{variant} {M}x{N}x{K} epi {epi} lds_epi {lds_epi} ldx {ldx} ldo {ldo}")
    finally:
        _tune(**SHIPPED)


# ---- A3. gate-residual ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fs,F", [(4, 37), (7, 19)])
@pytest.mark.parametrize("N", [384, 200])
def test_gemm_gate_residual_small_frames(fs, F, N):
    """B = 2 with frame_len 4 / 7 (M = 296 / 266: frames straddle every wave tile and the m-tile boundary), gate_idx 4 of 6: mod = NULL
    runs gemm_asm_128_gate_res at N = 384 (HIP at N = 200), a mod vector the HIP kernels' per-row evaluation.  Bit for bit against the
    host tails, res in its own [M, ldo] buffer and aliasing out, at wide strides."""
    B, K = 2, 256
    M = B * F * fs
    D = Data.get(M, N, K)
    g = torch.Generator().manual_seed(fs)
    e = (torch.randint(-8, 9, (B, F, 6, N), generator=g).float() * 2.0 ** -2).to(bf).to(DEV)
    mod = (torch.randint(-8, 9, (6, N), generator=g).float() * 2.0 ** -3).to(bf).to(DEV)
    for md in (None, mod):
        plan = _plan_epi(M, N, K, GATE, 1 if md is None else 0)
        assert re.match(_family(M, N, K, GATE, md is not None), plan), plan
        want = epi_tail(D.want, GATE, D.res, e, md, 4, fs)
        for ldx, ldo in _strides(N, K):
            for alias in (False, True):
                got = _gemm(D, M, GATE, ldx, ldo, alias=alias, e=e, mod=md, gate_idx=4, rpb=F * fs, fl=fs)
                assert torch.equal(got, want), f"fs {fs} N {N} mod {md is not None} ldx {ldx} ldo {ldo} alias {alias} [{plan.split('<')[0]}]"
        if plan.startswith("gemm_asm"):
            try:
                _tune(gemm_asm=0)
                assert torch.equal(_gemm(D, M, GATE, K + 8, N + 8, e=e, mod=md, gate_idx=4, rpb=F * fs, fl=fs), want)
            finally:
                _tune(gemm_asm=35)


# ---- A4. persistent against classic -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,epi", [(4102, 2048, BIAS), (4102, 2048, RES), (4102, 2048, GATE), (2900, 4608, BIAS), (2100, 8960, GELU)])
@pytest.mark.parametrize("K,group_m", [(256, 4), (256, 1), (320, 4), (320, 1), (1536, 4), (8960, 4)])
def test_gemm_persistent_kernels_bit_exact(M, N, K, epi, group_m):
    """Each of the five persistent kernels with more tiles than CUs (the plan must say so: 17 x 16 = 272, 12 x 24 = 288, 9 x 40 = 360
    tiles) and a ragged last m-tile (6, 84, 52 rows), at K = 256, 320, 1536 and 8960 (4, 5, 24, 140 K-steps: each leaves the unrolled
    loop elsewhere and hands the next tile over from another slot), with gemm_group_m 4 and 1, at contiguous and wide strides: equal to
    the host and to the classic kernels bit for bit (GELU: classic bit for bit, torch within the bound)."""
    D = Data.get(M, N, K, gelu=epi == GELU)
    kw = {}
    want = D.gelu if epi == GELU else None if epi == GATE else epi_tail(D.want, epi, D.res)
    if epi == GATE:
        B, fs = 2, 7
        F = M // (B * fs)
        assert B * F * fs == M
        g = torch.Generator().manual_seed(9)
        e = (torch.randint(-8, 9, (B, F, 6, N), generator=g).float() * 2.0 ** -2).to(bf).to(DEV)
        kw = dict(e=e, gate_idx=5, rpb=F * fs, fl=fs)
        want = epi_tail(D.want, GATE, D.res, e, None, 5, fs)
    try:
        _tune(gemm_group_m=group_m)
        plan = _plan_epi(M, N, K, epi)
        m = re.match(r"gemm_asmp_\d+_\w+<bf16>.*, (\d+) persistent workgroups walk (\d+) tiles", plan)
        assert m and int(m.group(2)) > int(m.group(1)), plan
        for ldx, ldo in _strides(N, K):
            got = _gemm(D, M, epi, ldx, ldo, alias=(ldo > N), **kw)
            if epi == GELU:
                _assert_gelu_close(got, want, f"persistent gelu ldx {ldx} ldo {ldo}")
            else:
                assert torch.equal(got, want), (plan, ldx, ldo)
            try:
                _tune(gemm_asm=3)
                assert re.match(r"gemm_asm_\d+_", _plan_epi(M, N, K, epi))
                assert torch.equal(_gemm(D, M, epi, ldx, ldo, **kw), got), f"classic vs persistent ldx {ldx} ldo {ldo}"
            finally:
                _tune(gemm_asm=35)
    finally:
        _tune(**SHIPPED)


# ---- A5. split-K ----------------------------------------------------------------------------------------------------------------------------
def _workspace(S, M, N):
    n = S * M * N
    ws = torch.full((n + 64,), float("nan"), dtype=torch.float32, device=DEV)          # no initialisation needed: handed over as NaN
    ws[n:] = 12345.0                                                                  # guard words
    return ws, n


@pytest.mark.parametrize("N,K,S", [(1536, 1024, 2), (1536, 1088, 2), (1536, 1536, 3), (1536, 1856, 3), (1024, 2048, 4), (4096, 2048, 4),
                                   (4096, 2112, 4)])
def test_gemm_split_k_bit_exact(N, K, S):
    """ll_gemm_bf16_ksplit / ..._t5norm with 2, 3 and 4 K-ranges (K = 1088 / 1856 / 2112: 17 / 29 / 33 K-steps, the last range shorter
    than the others), M in {1, 77, 512, 1024}, ldx > K and ldo > N, a NaN-filled workspace with guard words: gemm_asm_128_partial +
    the reduce kernels equal the host bit for bit (the sums are exact in any order); t5norm (ldo = N; N <= 2048 and both column groups
    at N = 4096) equals ll_gemm_bf16 + ll_t5_rmsnorm."""
    L, lib = _lib()
    D = Data.get(1024, N, K)
    nw = (torch.randint(1, 9, (N,), generator=torch.Generator().manual_seed(K)).float() * 2.0 ** -2).to(bf).to(DEV)
    for M in (1, 77, 512, 1024):
        assert lib.ll_gemm_ksplit_plan(M, N, K) == S, (M, N, K, lib.ll_gemm_ksplit_plan(M, N, K))
        ws, n = _workspace(S, M, N)
        assert lib.ll_gemm_ksplit_workspace_bytes(M, N, K) == 4 * n
        for ldx, ldo in _strides(N, K):
            for epi in (BIAS, RES):
                ws[:n] = float("nan")
                got = _gemm(D, M, epi, ldx, ldo, alias=(ldo > N), fn="ll_gemm_bf16_ksplit", tail=lambda res: (epi, res, ws, 4 * n))
                want = epi_tail(D.want[:M], epi, D.res[:M])
                assert torch.equal(got, want), f"split-K {M}x{N}x{K} S {S} epi {epi} ldx {ldx} ldo {ldo}"
                assert bool((ws[n:] == 12345.0).all()) and bool(torch.isfinite(ws[:n]).all()), "workspace guard / coverage"
            if N <= 4096:
                ws[:n] = float("nan")
                h = _nan_bf16(M + 3, N)
                xn = _gemm(D, M, RES, ldx, N, fn="ll_gemm_bf16_ksplit_t5norm", tail=lambda res: (res, nw, 1e-6, h, ws, 4 * n))
                want = epi_tail(D.want[:M], RES, D.res[:M])
                assert torch.equal(xn, want), f"t5norm x_new {M}x{N}x{K} ldx {ldx}"
                hw = torch.empty(M, N, dtype=bf, device=DEV)
                _run("ll_t5_rmsnorm", want.contiguous(), nw, hw, M, N, 1e-6)
                assert torch.equal(h[:M], hw) and _untouched_bf16(h[M:]), f"t5norm h {M}x{N}x{K}"
                assert bool((ws[n:] == 12345.0).all())
    try:                      # the same calls with the generated kernels off are the plain HIP kernels: the same bits
        _tune(gemm_asm=0)
        assert lib.ll_gemm_ksplit_plan(77, N, K) == 0
        ws, n = _workspace(S, 77, N)
        got = _gemm(D, 77, RES, K + 8, N + 8, fn="ll_gemm_bf16_ksplit", tail=lambda res: (RES, res, ws, 4 * n))
        assert torch.equal(got, epi_tail(D.want[:77], RES, D.res[:77])) and bool(torch.isnan(ws[:n]).all())
    finally:
        _tune(gemm_asm=35)


# ---- A6. the sum-of-squares form ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", [(128, 256), (384, 256), (1536, 256), (2048, 256), (384, 320), (2048, 320), (384, 1536), (2048, 1536),
                                 (384, 8960), (2048, 8960)])
def test_gemm_ssq_planes_bit_exact(N, K):
    """ll_gemm_bf16_ssq with 1, 3, 12 and 16 planes at M in {1, 65, 300, 1100} on the unit-scale data set (integer outputs: every
    plane's sum of squares is exact in fp32 in any order): out and ssq [planes, M] equal the host bit for bit, ldo = N and N + 8, NaN
    guard after the planes, K from 4 to 140 K-steps; ldx != K is refused."""
    L, lib = _lib()
    Ms = (1, 65, 300, 1100) if K <= 320 else (1, 65, 300)      # fewer rows at long K: the data set's largest |output| stays below 362
    D = Data.get(max(Ms), N, K, unit=True)
    assert _plan_epi(max(Ms), N, K, BIAS).startswith("gemm_asm_128_bias")      # the sum-of-squares kernel is that kernel's sibling
    for M in Ms:
        assert lib.ll_gemm_ssq_planes(M, N, K) == N // 128
        want_ssq = D.d.ssq(M).to(DEV)
        for ldo in (N, N + 8):
            ssq = torch.full((N // 128 * M + 64,), float("nan"), dtype=torch.float32, device=DEV)
            x = D.x[:M].contiguous()
            out = _nan_bf16(M + 3, ldo)
            _run("ll_gemm_bf16_ssq", x, D.w, D.b, out, ssq, M, N, K, K, ldo)
            assert torch.equal(out[:M, :N], D.want[:M]) and _untouched_bf16(out[M:]) and _untouched_bf16(out[:M, N:]), (M, N, ldo)
            assert torch.equal(ssq[:N // 128 * M].view(N // 128, M), want_ssq), (M, N, ldo)
            assert bool(torch.isnan(ssq[N // 128 * M:]).all())
    with pytest.raises(RuntimeError, match="not covered"):
        _run("ll_gemm_bf16_ssq", _nan_bf16(8, K + 8), D.w, D.b, _nan_bf16(8, N), torch.zeros(N // 128 * 8, device=DEV), 8, N, K, K + 8, N)


# ---- A7. the fused QKV projection ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,L,C,ws,ro,wl,fam", [
    (1, 300, 384, 37, 100, 180, "gemm_asm_192_bias"),      # v_col0 = 768 = 4 x 192: generated; the window begins and ends inside m-tiles
    (1, 300, 384, 37, 100, 180, ("gemm_asm_192_bias", 320)), (1, 300, 384, 37, 100, 180, ("gemm_asm_192_bias", 1536)),
    (1, 300, 384, 37, 100, 180, ("gemm_asm_192_bias", 8960)),      # ... at 5, 24 and 140 K-steps
    (1, 300, 384, 0, 0, 300, "gemm_asm_192_bias"),         # every token inserted
    (1, 300, 384, 37, 300, 0, "gemm_asm_192_bias"),        # write_len 0: every V tile skipped
    (1, 300, 384, 5, 299, 1, "gemm_asm_192_bias"),         # the last token alone
    (1, 300, 256, 37, 100, 180, "gemm_kernel_v"),          # v_col0 = 512: not a tile boundary of the 192-wide kernel -> HIP
    (2, 150, 384, 37, 60, 90, None),                       # B = 2 (v_L != M): HIP (ll_gemm_plan_epi's QKV form describes one batch
                                                           # element only; the fallback's kernel is ll_gemm_plan's)
    (1, 2900, 1536, 11, 256, 2500, "gemm_asmp_192_bias"),  # 12 x 24 = 288 tiles: the persistent form, window on / inside tile boundaries
    (1, 2900, 1536, 11, 256, 2500, ("gemm_asmp_192_bias", 320)), (1, 2900, 1536, 11, 256, 2500, ("gemm_asmp_192_bias", 1536)),
    (1, 2900, 1536, 11, 256, 2500, ("gemm_asmp_192_bias", 8960)),
], ids=lambda v: str(v).replace(" ", ""))
def test_gemm_qkv_v_insert_bit_exact(B, L, C, ws, ro, wl, fam):
    """ll_gemm_bf16_qkv: the q | k thirds of out equal the host bit for bit, the V third goes to cache rows [ws, ws + wl) of each batch
    element for tokens [ro, ro + wl) and nowhere else (the cache is a NaN field), the v third of `out` is left unwritten as the header
    promises (both launchers skip it: gemm_asm_kernel.inl redirects or returns, epi_dest returns nullptr), at contiguous and wide strides;
    generated, persistent and HIP forms agree bit for bit."""
    fam, K = fam if isinstance(fam, tuple) else (fam, 256)
    M, N, S = B * L, 3 * C, L + 100
    D = Data.get(M, N, K)
    if fam is not None:
        plan = _plan_epi(M, N, K, BIAS, 2)
        assert plan.startswith(fam), plan
    else:
        assert _text("ll_gemm_plan", M, N, K, 0).startswith("gemm_kernel_v")

    def run(ldx, ldo):
        cache = _nan_bf16(B * S + 3, C)
        got = _gemm(D, M, BIAS, ldx, ldo, fn="ll_gemm_bf16_qkv", tail=lambda res: (cache, B, L, S, ws, ro, wl))
        return got, cache

    for ldx, ldo in _strides(N, K):
        got, cache = run(ldx, ldo)
        assert torch.equal(got[:, :2 * C], D.want[:, :2 * C]), (ldx, ldo)
        assert _untouched_bf16(got[:, 2 * C:]), "the v third of out was written"
        want_c = _nan_bf16(B * S + 3, C)
        for b in range(B):
            want_c[b * S + ws:b * S + ws + wl] = D.want[b * L + ro:b * L + ro + wl, 2 * C:]
        assert torch.equal(cache.view(torch.int16), want_c.view(torch.int16)), (ldx, ldo)
        for asm in (3, 0):
            try:
                _tune(gemm_asm=asm)
                g2, c2 = run(ldx, ldo)
            finally:
                _tune(gemm_asm=35)
            assert torch.equal(g2.view(torch.int16), got.view(torch.int16)) and torch.equal(c2.view(torch.int16), cache.view(torch.int16)), asm


# ---- C. ldo must keep rows on 16 bytes ---------------------------------------------------------------------------------------------------------
def test_gemm_entry_points_refuse_ldo_off_16_bytes():
    """Every store path writes 16-byte vectors at row * ldo + n (generated epilogues, LDS-staged HIP epilogues, split-K reduce), so the
    entry points require ldo % 8 == 0: ldo = N + 4 is refused before anything is launched."""
    M, N, K = 8, 128, 256
    D = Data.get(M, N, K)
    out = _nan_bf16(M, N + 4)
    ws = torch.zeros(4 * M * N, device=DEV)
    with pytest.raises(RuntimeError, match="multiple of 8"):
        _run("ll_gemm_bf16", D.x, D.w, D.b, out, M, N, K, K, N + 4, BIAS, None, None, None, 0, 0, 0, 0)
    with pytest.raises(RuntimeError, match="multiple of 8"):
        _run("ll_gemm_bf16_ksplit", D.x, D.w, D.b, out, M, N, K, K, N + 4, BIAS, None, ws, ws.numel() * 4)
    with pytest.raises(RuntimeError, match="multiple of 8"):
        _run("ll_gemm_bf16_ssq", D.x, D.w, D.b, out, ws, M, N, K, K, N + 4)
    with pytest.raises(RuntimeError, match="multiple of 8"):
        _run("ll_gemm_bf16_qkv", D.x, D.w, D.b, out, M, N, K, K, N + 4, out, 1, M, M, 0, 0, 0)
    # the int8 entry points share the check (check_epilogue), the fp8 ones have their own
    M, N = 8, 384
    out = _nan_bf16(M, N + 4)
    xq, wq = torch.zeros(M, K, dtype=torch.int8, device=DEV), torch.zeros(N, K, dtype=torch.int8, device=DEV)
    sx, sw, b = torch.ones(M, device=DEV), torch.ones(N, device=DEV), torch.zeros(N, dtype=bf, device=DEV)
    for fn in ("ll_gemm_w8a8", "ll_gemm_f8"):
        with pytest.raises(RuntimeError, match="multiple of 8"):
            _run(fn, xq, sx, wq, sw, b, out, M, N, K, N + 4, BIAS, None, None, None, 0, 0, 0, 0)
    for fn in ("ll_gemm_w8a8_qkv", "ll_gemm_f8_qkv"):
        with pytest.raises(RuntimeError, match="multiple of 8"):
            _run(fn, xq, sx, wq, sw, b, out, M, N, K, N + 4, out, 1, M, M, 0, 0, 0)
    assert _untouched_bf16(out)


# ---- B. attention ---------------------------------------------------------------------------------------------------------------------------
def _attn(case, phase, wide, qnorm=False, build=None):
    """One call of a case: q [B * Lq, ldq] (wide: the first third of a QKV buffer whose other columns hold NaN), k / v [B, Sk, ldk] with
    NaN padding columns (wide: a batch stride larger than Sk * ldk, the slack finite like every row outside the ranges), out a NaN
    field [B * Lq + 5, ldo].  Checks sentinels and the bound; returns nothing."""
    B, Lq, H, Sk = case.B, case.Lq, case.H, case.Sk
    C = H * 128
    q, k, v, exp = build if build is not None else case.build(phase, DEV)
    ldq, ldo, ldk, slack = (3 * C, C + 8, C + 8, 24) if wide else (C, C, C, 0)
    if qnorm:
        ldq = C
        ssq, _ = case.q_raw_and_ssq(q)
        ssq = ssq.to(DEV)
        nw = torch.ones(C, dtype=bf, device=DEV)
    qb = _nan_bf16(B * Lq, ldq)
    qb[:, :C] = q.view(B * Lq, C).to(bf)
    kbs = Sk * ldk + slack
    kb = torch.full((B, kbs), E.V_OUT, dtype=bf, device=DEV)
    vb = torch.full((B, kbs), E.V_OUT, dtype=bf, device=DEV)
    for buf, t in ((kb, k), (vb, v)):
        rows = buf[:, :Sk * ldk].view(B, Sk, ldk)
        rows[..., C:] = _nan_bf16(1)
        rows[..., :C] = t.view(B, Sk, C).to(bf)
    out = _nan_bf16(B * Lq + 5, ldo)
    (s0, n0), (s1, n1) = case.ranges[0], (case.ranges[1] if len(case.ranges) > 1 else (0, 0))
    if qnorm:
        _run("ll_flash_attn_qnorm", qb, ssq, nw, 1e-6, kb, vb, out, B, Lq, H, ldq, ldo, ldk, kbs, s0, n0, SCALE)
    else:
        _run("ll_flash_attn", qb, kb, vb, out, B, Lq, H, ldq, ldo, ldk, kbs, s0, n0, s1, n1, SCALE)
    assert _untouched_bf16(out[B * Lq:]) and _untouched_bf16(out[:, C:]), "attention wrote outside [B * Lq, H * 128]"
    got = out[:B * Lq, :C].double().view(B, Lq, H, 128)
    assert torch.isfinite(got).all()
    over = (got - exp).abs() / E.attn_bound(exp, case.nkeys)
    worst = over.max().item()
    if worst > 1:
        b, r, h, c = [int(i) for i in (over == over.max()).nonzero()[0]]
        uni, tg = case.row_plan(phase)
        raise AssertionError(f"B{B} Lq{Lq} H{H} {case.ranges} phase {phase} wide {wide}: {int((over > 1).sum())} elements outside the bound, worst "
                             f"{worst:.1f} x at batch {b} row {r} ({'uniform' if uni[r] else 'gather -> slot %d' % tg[r]}) head {h} channel {c}: "
                             f"got {got[b, r, h, c].item()} want {exp[b, r, h, c].item()}")


def _attn_case(geom, want_kernel, adjacent=0, **kw):
    """Both phases x both stride sets of one geometry under the current tuning, and attn_xcd 0 on the multi-tile multi-head ones."""
    B, Lq, H, ranges = geom
    case = E.AttnCase(B, Lq, H, ranges, **kw)
    n0, n1 = ranges[0][1], ranges[1][1] if len(ranges) > 1 else 0
    plan = _attn_plan(B, Lq, H, n0, n1, adjacent)
    assert plan.startswith(want_kernel), (geom, plan)
    for phase in (0, 1):
        for wide in (False, True):
            _attn(case, phase, wide)
    if H > 1 and Lq > 256:
        try:
            _tune(attn_xcd=0)
            assert "XCD" not in _attn_plan(B, Lq, H, n0, n1, adjacent)
            _attn(case, 1, True)
        finally:
            _tune(attn_xcd=1)


_ids = lambda g: f"B{g[0]}-Lq{g[1]}-H{g[2]}-{g[3]}".replace(" ", "")


@pytest.mark.parametrize("geom", E.PIPE0_CASES, ids=_ids)
def test_attn_pipe_one_barrier_kernel(geom):
    """flash_attn_pipe_kernel<8, 0>: one range below attn_pp_min_keys with the generated kernel off."""
    _tune(attn_asm=0)
    _attn_case(geom, "flash_attn_pipe_kernel<8, 0>")


@pytest.mark.parametrize("geom", E.PIPE1_CASES, ids=_ids)
def test_attn_pipe_ping_pong_kernel(geom):
    """flash_attn_pipe_kernel<8, 1>: >= 1024 keys with the generated kernel off."""
    _tune(attn_asm=0)
    _attn_case(geom, "flash_attn_pipe_kernel<8, 1>")


@pytest.mark.parametrize("geom", E.ASM_CASES, ids=_ids)
def test_attn_generated_kernel(geom):
    """flash_attn_asm_kernel with attn_asm_min_keys at its floor (two tiles = 128 keys: the special-cased first and last tile and
    nothing between), and under the shipped threshold where the range has 512 keys or more."""
    nkeys = geom[3][0][1]
    _tune(attn_asm_min_keys=128)
    _attn_case(geom, "flash_attn_asm_kernel")
    _tune(attn_asm_min_keys=512)
    if nkeys >= 512:
        _attn_case(geom, "flash_attn_asm_kernel")
    else:
        assert _attn_plan(geom[0], geom[1], geom[2], nkeys).startswith("flash_attn_pipe_kernel<8, 0>")


@pytest.mark.parametrize("geom", E.TWO_RANGE_CASES, ids=_ids)
def test_attn_two_range_kernel(geom):
    """flash_attn_kernel<4>: two non-adjacent ranges under the shipped tuning."""
    _attn_case(geom, "flash_attn_kernel<4>")


@pytest.mark.parametrize("geom", E.PLAIN_ONE_RANGE_CASES, ids=_ids)
def test_attn_plain_kernel_one_range(geom):
    """flash_attn_kernel<4> on one range (attn_variant 0)."""
    _tune(attn_variant=0)
    _attn_case(geom, "flash_attn_kernel<4>")


@pytest.mark.parametrize("geom", E.ADJACENT_CASES, ids=_ids)
def test_attn_adjacent_ranges_merge(geom):
    """Two adjacent ranges are one range (the plan names a single-range kernel): the seam falls inside a tile.  Generated kernel, both
    HIP pipelines' choice with it off, and the plain kernel."""
    _attn_case(geom, "flash_attn_asm_kernel", adjacent=1)
    _tune(attn_asm=0)
    _attn_case(geom, "flash_attn_pipe_kernel<8, 0>" if sum(n for _, n in geom[3]) < 1024 else "flash_attn_pipe_kernel<8, 1>", adjacent=1)
    _tune(attn_variant=0)
    _attn_case(geom, "flash_attn_kernel<4>", adjacent=1)


@pytest.mark.parametrize("geom", E.QNORM_CASES, ids=_ids)
def test_attn_generated_qnorm_kernel(geom):
    """flash_attn_asm_qn_kernel through ll_flash_attn_qnorm: raw q of amplitude 2 with its host-computed plane sums of squares and a unit
    norm weight normalises to the +-1 codes, keys carry amplitude 4: the same scores, the same expected outputs.  With attn_asm_min_keys
    at its floor (128 / 129 keys: the special-cased first and last tile with nothing between) and under the shipped threshold."""
    L, lib = _lib()
    B, Lq, H, ranges = geom
    nkeys = ranges[0][1]
    case = E.AttnCase(B, Lq, H, ranges, a_k=4.0)
    # (ll_flash_attn_plan names ll_flash_attn's kernel; the q-norm entry point has no plan call of its own: it runs
    #  flash_attn_asm_qn_kernel exactly where ll_flash_attn_qnorm_ok says 1, which is where the plan names the generated kernel)
    for min_keys in (128, 512):
        _tune(attn_asm_min_keys=min_keys)
        ok = lib.ll_flash_attn_qnorm_ok(H, nkeys)
        assert ok == (1 if nkeys >= min_keys else 0) and _attn_plan(B, Lq, H, nkeys).startswith("flash_attn_asm_kernel") == bool(ok)
        if not ok:
            continue
        for xcd in (1, 0):
            _tune(attn_xcd=xcd)
            for phase in (0, 1):
                for wide in (False, True):
                    _attn(case, phase, wide, qnorm=True)


@pytest.mark.parametrize("geom", E.PROD_CASES, ids=_ids)
def test_attn_production_shapes(geom):
    """Lq 4680 over the 18720-key cache and the recache shape Lq = Lk = 18720, 12 heads, q / k / v generated on the device: the
    generated kernel and the ping-pong HIP kernel."""
    B, Lq, H, ranges = geom
    case = E.AttnCase(B, Lq, H, ranges)
    built = case.build(1, DEV)
    assert _attn_plan(B, Lq, H, ranges[0][1]).startswith("flash_attn_asm_kernel")
    _attn(case, 1, False, build=built)
    _tune(attn_asm=0)
    assert _attn_plan(B, Lq, H, ranges[0][1]).startswith("flash_attn_pipe_kernel<8, 1>")
    _attn(case, 1, True, build=built)


def test_attn_refuses_overlapping_ranges():
    """Two ranges that share keys would count them twice: refused before anything is launched (ll_flash_attn_mx has the same rule);
    ranges that only touch, and a second range before the first, are accepted."""
    case = E.AttnCase(1, 33, 1, [(0, 64), (100, 28)])
    q, k, v, _ = case.build(0, DEV)
    q, k, v = (t.to(bf).contiguous() for t in (q, k, v))
    out = _nan_bf16(33 + 3, 128)
    for s0, n0, s1, n1 in ((0, 64, 63, 10), (40, 30, 0, 41), (0, 64, 0, 64), (10, 50, 20, 5)):
        with pytest.raises(RuntimeError, match="overlap"):
            _run("ll_flash_attn", q, k, v, out, 1, 33, 1, 128, 128, 128, case.Sk * 128, s0, n0, s1, n1, SCALE)
    torch.cuda.synchronize()
    assert _untouched_bf16(out)
    for s0, n0, s1, n1 in ((0, 64, 64, 10), (100, 28, 0, 64)):
        _run("ll_flash_attn", q, k, v, out, 1, 33, 1, 128, 128, 128, case.Sk * 128, s0, n0, s1, n1, SCALE)
    torch.cuda.synchronize()
    assert _untouched_bf16(out[33:]) and bool(torch.isfinite(out[:33].float()).all())
