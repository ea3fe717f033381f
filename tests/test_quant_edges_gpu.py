"""The quantised block linears, their quantisers and producers, and MX self-attention at the shape edges the C ABI accepts but the
model (dim 1536, N in {1536, 4608, 8960}, K in {1536, 8960}, ldo == N) never reaches: partial n- and m-tiles, N % 16 == 8, one to
five K-stages, M below one wave tile, tile counts below 8 or not a multiple of GROUP_M, ldo > N, MX-output GELU forms at partial
tiles, QKV V-inserts that start inside a tile, every DISPATCH_NCH instance of the producers, and attention over few heads, short and
ragged query blocks, padded S32 and key ranges that do not start on a 32-slot boundary.

Every GEMM runs on exact data (small integer codes under power-of-two scales: every fp32 sum is exact), so results are compared bit
for bit with the host (tests/mx_ref.py, mx6_ref.py, mx4_ref.py, fp8_ref.py, mx_attn_ref.py), and every buffer a kernel could spill
into carries NaN sentinels that must survive.  The four MX families see the same operand VALUES in their own encodings (e4m3, E2M3,
E2M1 under one scale per (row, 32-block)), so their bf16 outputs -- GELU included -- must be identical; f8 and w8a8 see the same
integers."""
import copy
import itertools
import math

import pytest
import torch
import torch.nn.functional as Fn

import fp8_ref
import mx4_ref
import mx6_ref
import mx_attn_ref as MA
import mx_ref
from longlive_amd import synth
from quant_exact import codes_and_scales, epi_tail, exact_operands, hard_x_f8, hard_x_mx, unit_c_scale
from util import assert_bf16_close, bf

pytestmark = pytest.mark.gpu
DEV = "cuda"
U8 = torch.uint8
FP8 = torch.float8_e4m3fn
NAN16 = 0x7FC1                     # a bf16 quiet-NaN bit pattern: padding and sentinel rows
GUARD8 = 0xFF                      # an e4m3 NaN code / not a valid E8M0 scale the kernels write here: guard bytes
GEMM_ASM_DEFAULT = 35              # gemm.hip g_gemm_asm: int8 calls stay on the HIP kernels (bit 4 clear)

# entry point, activation encoding, weight encoding, K granule
MX_FAMS = {"mx": ("ll_gemm_mx", "e4m3", "e4m3", 128), "mx6": ("ll_gemm_mx6", "e2m3", "e2m3", 256),
           "mx4w6": ("ll_gemm_mx4w6", "e2m3", "e2m1", 256), "mx4": ("ll_gemm_mx4", "e2m1", "e2m1", 256)}
RW_FAMS = {"f8": "ll_gemm_f8", "w8a8": "ll_gemm_w8a8"}
ALL_FAMS = ("f8", "w8a8", "mx", "mx6", "mx4w6", "mx4")


@pytest.fixture(scope="module")
def ops():
    from longlive_amd import ops as O
    return O


def hn(name, shape, scale=1.0):
    return (scale * synth.hash_normal(149, name, shape)).to(bf)


def _run(fn, *args):
    """A C entry point with tensors as device pointers (None = NULL) and the current stream appended; a nonzero return raises."""
    from longlive_amd import _lib, ops as O
    lib = _lib.load()
    a = [t.data_ptr() if isinstance(t, torch.Tensor) else t for t in args]
    _lib.check(getattr(lib, fn)(*a, O._stream()), fn)


def _nan_bf16(*shape):
    return torch.full(shape, NAN16, dtype=torch.int16, device=DEV).view(bf)


def _untouched_bf16(t):
    return bool((t.contiguous().view(torch.int16) == NAN16).all())


def _guarded_u8(n, guard=256):
    return torch.full((n + guard,), GUARD8, dtype=U8, device=DEV)


def _fams(K):
    return [f for f in ALL_FAMS if K % (MX_FAMS[f][3] if f in MX_FAMS else 128) == 0]


class Operands:
    """Exact operands of one M x N x K problem in every family's encoding: MX values c 2^e (c in -2..2, a distinct power of two per
    (row, 32-block), W asymmetric) and the rowwise families' small integers under power-of-two row / channel scales."""

    def __init__(self, M, N, K, seed):
        self.M, self.N, self.K = M, N, K
        xc, xe, xv = codes_and_scales(M, K, seed, False)
        wc, we, wv = codes_and_scales(N, K, seed + 1, True)
        self.acc_mx = xv @ wv.t()
        assert self.acc_mx.abs().max() < 2 ** 17          # multiples of 2^-6: exact in fp32
        kinds = ("e4m3",) + (("e2m3", "e2m1") if K % 256 == 0 else ())
        self.X = {k: self._enc(k, xc, xe, xv) for k in kinds}
        self.W = {k: self._enc(k, wc, we, wv) for k in kinds}
        cx, cw, sx, sw = exact_operands(M, N, K, seed + 2)
        self.acc_rw = (cx.double() @ cw.double().t()).float()
        assert self.acc_rw.abs().max() < 2 ** 24
        self.scale_rw = sx.unsqueeze(1) * sw.unsqueeze(0)
        sx, sw = sx.to(DEV), sw.to(DEV)
        self.X["f8"] = (cx.to(FP8).view(U8).to(DEV), sx)
        self.W["f8"] = (cw.to(FP8).view(U8).to(DEV), sw)
        self.X["w8a8"] = (cx.to(torch.int8).to(DEV), sx)
        self.W["w8a8"] = (cw.to(torch.int8).to(DEV), sw)

    @staticmethod
    def _enc(kind, c, e, v):
        if kind == "e4m3":                       # 2^7 c or 2^8 c under the MX rule's own scale: the same values
            q, s = mx_ref.quantize(v.to(bf))
            assert torch.equal(mx_ref.dequantize(q, s), v)
            return q.view(U8).to(DEV), s.to(DEV)
        ref = mx6_ref if kind == "e2m3" else mx4_ref
        return torch.from_numpy(ref.pack(ref.encode(c.numpy()))).to(DEV), (e + 127).to(U8).to(DEV)

    def rows(self, M):
        """The problem on the first M activation rows (a row's codes, scales and sums do not depend on the other rows)."""
        od = copy.copy(self)
        od.M = M
        od.X = {k: (q[:M], s[:M]) for k, (q, s) in self.X.items()}
        od.acc_mx, od.acc_rw, od.scale_rw = self.acc_mx[:M], self.acc_rw[:M], self.scale_rw[:M]
        return od

    def operands(self, fam):
        if fam in RW_FAMS:
            return self.X[fam], self.W[fam]
        _, xk, wk, _ = MX_FAMS[fam]
        return self.X[xk], self.W[wk]

    def want(self, fam, bias):
        """The bias form on the host: the exact sum (times the row / channel scales), + bias in fp32, rounded to bf16."""
        if fam in RW_FAMS:
            return (self.acc_rw * self.scale_rw + bias.float()).to(bf)
        return (self.acc_mx.float() + bias.float()).to(bf)


def _gemm(fam, od, bias, epi=0, out=None, ldo=None, res=None, e=None, mod=None, gate_idx=0, rpb=0, fl=0, qo=None, so=None):
    M, N, K = od.M, od.N, od.K
    (xq, sx), (wq, sw) = od.operands(fam)
    if out is None and qo is None:
        out = torch.empty(M, N, dtype=bf, device=DEV)
    nmod = 0 if e is None else e.shape[-2]
    tail = (M, N, K, ldo or N, epi, res, e, mod, nmod, gate_idx, rpb, fl)
    if fam in RW_FAMS:
        _run(RW_FAMS[fam], xq, sx, wq, sw, bias, out, *tail)
    else:
        _run(MX_FAMS[fam][0], xq, sx, wq, sw, bias, out, qo, so, *tail)
    return out


def _gelu_checks(gelus, v_ref, what):
    """Every family's GELU equals the first one's bit for bit, and is within 2 bf16 ulp of torch's tanh-GELU of the bias form."""
    names = list(gelus)
    for f in names[1:]:
        assert torch.equal(gelus[f].cpu(), gelus[names[0]].cpu()), f"{what}: gelu {f} vs {names[0]}"
    assert_bf16_close(gelus[names[0]].cpu(), Fn.gelu(v_ref, approximate="tanh"), 2, 0.0, f"{what}: gelu vs torch")


# ---- 1. shape sweep: every (M, N, K) of the edge lists ------------------------------------------------------------------------------
# N: 8 (one partial 8-column tile), 136 (one tile + 8), 200 (N % 16 == 8), 1544 and 4616 (a partial last tile behind many whole ones).
# K: 128 / 256 / 384 (one / two / three stages of the 128-k kernels), 256 / 512 / 768 (nk = 1 / 2 / 3 of the 256-k kernels' scale
# ring: 768 is the first use of slot 2 and of the kt + 2 prefetch), 1280 (an odd five 256-k stages).
# M: 1 / 15 / 63 (below one wave tile: the `live` guard), 64, 65, 257 and 1100 (2 and 5 m-tiles: not a multiple of GROUP_M = 4).
# M = 1 x N = 8 is one workgroup; most of the others are tile counts not a multiple of 8 (xcd_remap's remainder path).
N_EDGES = (8, 136, 200, 1544, 4616)
K_EDGES = (128, 256, 384, 512, 768, 1280)
M_EDGES = (1, 15, 63, 64, 65, 257, 1100)


@pytest.mark.parametrize("N,K", list(itertools.product(N_EDGES, K_EDGES)))
def test_gemm_shape_sweep_bias_and_gelu_bit_exact(N, K):
    """Every M of M_EDGES at this (N, K), on the first M rows of one operand set: the bias form of every family that accepts K equals
    the host bit for bit; GELU equals the sibling families' bit for bit (the MX families among themselves, f8 with w8a8) and torch's
    tanh-GELU within 2 ulp."""
    full = Operands(max(M_EDGES), N, K, N + K)
    bias = hn(f"b{N}", (N,), 0.1)
    bd = bias.to(DEV)
    for M in M_EDGES:
        od = full.rows(M)
        gel_mx, gel_rw = {}, {}
        for fam in _fams(K):
            v = _gemm(fam, od, bd).cpu()
            want = od.want(fam, bias)
            assert torch.equal(v, want), f"{fam} {M}x{N}x{K}: bias, max |diff| {(v.float() - want.float()).abs().max()}"
            (gel_rw if fam in RW_FAMS else gel_mx)[fam] = _gemm(fam, od, bd, epi=1)
        _gelu_checks(gel_mx, od.want("mx", bias), f"mx {M}x{N}x{K}")
        _gelu_checks(gel_rw, od.want("f8", bias), f"rowwise {M}x{N}x{K}")


@pytest.mark.parametrize("fs,F", [(4, 37), (7, 19)])
def test_residual_and_gate_residual_small_frames_ragged_tile(fs, F):
    """B = 2 with frame_len 4 / 7 (M = 296 / 266: a partial second m-tile, frames straddling every wave tile), N = 200, with and without
    mod: residual and gate-residual equal the host epilogue tails on the bias form bit for bit, in every family."""
    B, N, K = 2, 200, 256
    M = B * F * fs
    od = Operands(M, N, K, fs)
    bias = hn("gb", (N,), 0.1)
    res, e, mod = hn("gres", (M, N)), hn("ge", (B, F, 6, N), 0.5), hn("gmod", (6, N), 0.1)
    bd, rd, ed, md_ = bias.to(DEV), res.to(DEV), e.to(DEV), mod.to(DEV)
    for fam in ALL_FAMS:
        v = od.want(fam, bias)
        got = _gemm(fam, od, bd, epi=3, res=rd).cpu()
        assert torch.equal(got, epi_tail(v, 3, res)), f"{fam} fs={fs}: residual"
        for md in (mod, None):
            got = _gemm(fam, od, bd, epi=2, res=rd, e=ed, mod=None if md is None else md_, gate_idx=4, rpb=F * fs, fl=fs).cpu()
            assert torch.equal(got, epi_tail(v, 2, res, e, md, 4, fs)), f"{fam} fs={fs} mod={md is not None}: gate-residual"


TILINGS = {2: "gemm_kernel_v2<{}> tile 256x128", 3: "gemm_kernel_v5<{}> tile 256x256", 5: "gemm_kernel_v5<{}> tile 256x192",
           6: "gemm_kernel_v5<{}> tile 256x224"}


@pytest.mark.parametrize("N", [1544, 200])
def test_rowwise_tilings_at_ragged_n(ops, N):
    """Every big-M tiling of the f8 and int8 kernels (forced through gemm_variant; int8 pinned to the HIP kernels through gemm_asm) at a
    partial last n-tile and m-tile (M = 2100 = 8 x 256 + 52, 9 m-tiles): bias, GELU (f8 == w8a8), residual and gate-residual at B = 2,
    frame_len 7, bit for bit.  The plan strings name the instance that ran."""
    import ctypes
    lib = ops._lib.load()
    B, F, fs, K = 2, 150, 7, 256
    M = B * F * fs
    od = Operands(M, N, K, N)
    bias = hn(f"tb{N}", (N,), 0.1)
    res, e, mod = hn("tres", (M, N)), hn("te", (B, F, 6, N), 0.5), hn("tmod", (6, N), 0.1)
    bd, rd, ed, md_ = bias.to(DEV), res.to(DEV), e.to(DEV), mod.to(DEV)
    v = od.want("f8", bias)
    assert torch.equal(v, od.want("w8a8", bias))
    want_res, want_gate = epi_tail(v, 3, res), epi_tail(v, 2, res, e, mod, 1, fs)
    buf = ctypes.create_string_buffer(256)
    try:
        # bit 4 clear keeps int8 on the HIP kernels.  The default (35) has it clear today; it is set here so that a changed default or a
        # tuning override (LL_TUNING, LL_TUNING_TEST) cannot move these calls to the generated kernels.
        assert lib.ll_set_tuning(b"gemm_asm", GEMM_ASM_DEFAULT & ~16) == 0
        for variant, name in TILINGS.items():
            assert lib.ll_set_tuning(b"gemm_variant", variant) == 0
            assert ops.gemm_plan_f8(M, N, K).split(",")[0] == name.format("f8")
            for epi in (0, 1, 2, 3):
                plain = 0 if epi == 2 else 1                 # the gate-residual calls below pass a per-batch modulation vector
                ops._lib.check(lib.ll_gemm_plan_epi(M, N, K, 1, epi, plain, buf, 256))
                assert buf.value.decode().split(",")[0] == name.format("i8"), (variant, epi, buf.value)
            gel = {}
            for fam in RW_FAMS:
                got = _gemm(fam, od, bd).cpu()
                assert torch.equal(got, v), f"{fam} v{variant} N={N}: bias"
                gel[fam] = _gemm(fam, od, bd, epi=1)
                assert torch.equal(_gemm(fam, od, bd, epi=3, res=rd).cpu(), want_res), f"{fam} v{variant} N={N}: residual"
                got = _gemm(fam, od, bd, epi=2, res=rd, e=ed, mod=md_, gate_idx=1, rpb=F * fs, fl=fs).cpu()
                assert torch.equal(got, want_gate), f"{fam} v{variant} N={N}: gate-residual"
            _gelu_checks(gel, v, f"v{variant} N={N}")
    finally:
        lib.ll_set_tuning(b"gemm_variant", 0)
        lib.ll_set_tuning(b"gemm_asm", GEMM_ASM_DEFAULT)


def test_rowwise_tilings_at_one_k_step(ops):
    """The same four tilings at K = 128, one K-step: the rings have no next stage to issue.  M = 257, N = 200: a partial n-tile in
    every width, and only row 256 live in the second m-tile.  Bias and residual of f8 and w8a8, bit for bit against the host."""
    lib = ops._lib.load()
    M, N, K = 257, 200, 128
    od = Operands(M, N, K, 11)
    bias, res = hn("kb", (N,), 0.1), hn("kres", (M, N))
    bd, rd = bias.to(DEV), res.to(DEV)
    v = od.want("f8", bias)
    assert torch.equal(v, od.want("w8a8", bias))
    want_res = epi_tail(v, 3, res)
    try:
        assert lib.ll_set_tuning(b"gemm_asm", GEMM_ASM_DEFAULT & ~16) == 0      # int8 on the HIP kernels, as above
        for variant, name in TILINGS.items():
            assert lib.ll_set_tuning(b"gemm_variant", variant) == 0
            assert ops.gemm_plan_f8(M, N, K).split(",")[0] == name.format("f8")
            for fam in RW_FAMS:
                assert torch.equal(_gemm(fam, od, bd).cpu(), v), f"{fam} v{variant}: bias"
                assert torch.equal(_gemm(fam, od, bd, epi=3, res=rd).cpu(), want_res), f"{fam} v{variant}: residual"
    finally:
        lib.ll_set_tuning(b"gemm_variant", 0)
        lib.ll_set_tuning(b"gemm_asm", GEMM_ASM_DEFAULT)


# ---- 2. nothing is written outside the result -----------------------------------------------------------------------------------
@pytest.mark.parametrize("pad", [8, 64])
@pytest.mark.parametrize("fam", ALL_FAMS)
def test_row_stride_and_sentinel_rows_stay_untouched(fam, pad):
    """ldo = N + pad with NaN padding, and three NaN sentinel rows after M (M = 70: a partial wave tile): the N-column slice of the bias,
    GELU and residual forms is exact, and no padding or sentinel byte changes.  The residual is read at the same ldo (its NaN padding
    must not reach the result)."""
    M, N, K = 70, 200, 256
    od = Operands(M, N, K, 3 * pad)
    bias = hn("sb", (N,), 0.1)
    bd, ldo = bias.to(DEV), N + pad
    v = od.want(fam, bias)
    res = hn("sres", (M, N))
    rbuf = _nan_bf16(M, ldo)
    rbuf[:, :N] = res.to(DEV)
    for epi, want in ((0, v), (1, None), (3, epi_tail(v, 3, res))):
        out = _nan_bf16(M + 3, ldo)
        _gemm(fam, od, bd, epi=epi, out=out, ldo=ldo, res=rbuf if epi == 3 else None)
        got = out[:M, :N].cpu()
        if want is None:
            want = _gemm(fam, od, bd, epi=1).cpu()           # GELU: the ldo = N call's bits
        assert torch.equal(got, want), f"{fam} ldo={ldo} epi={epi}"
        assert _untouched_bf16(out[:M, N:]), f"{fam} ldo={ldo} epi={epi}: row padding written"
        assert _untouched_bf16(out[M:]), f"{fam} ldo={ldo} epi={epi}: sentinel rows written"


MX_OUT = {"mx": (mx_ref, lambda N: N), "mx6": (mx6_ref, lambda N: N // 4 * 3), "mx4w6": (mx6_ref, lambda N: N // 4 * 3),
          "mx4": (mx4_ref, lambda N: N // 2)}


@pytest.mark.parametrize("fam,N", [("mx", 160), ("mx", 4640), ("mx6", 256), ("mx4w6", 256), ("mx4", 256)])
def test_mx_output_gelu_forms_at_partial_tiles(fam, N):
    """The FFN1 forms that write MX codes + scales: ll_gemm_mx at N = 160 / 4640 (a partial last n-tile of 32 columns), the MXFP6 /
    MXFP4 outputs at N = 256, M = 70.  Bytes equal the family's host quantiser applied to the bf16 GELU form; the guard bytes after
    the code and scale buffers stay untouched."""
    M, K = 70, 256
    od = Operands(M, N, K, N)
    bd = hn(f"xb{N}", (N,), 0.1).to(DEV)
    ref, row_bytes = MX_OUT[fam]
    nq, ns = M * row_bytes(N), M * (N // 32)
    qbuf, sbuf = _guarded_u8(nq), _guarded_u8(ns)
    _gemm(fam, od, bd, epi=1, qo=qbuf, so=sbuf)
    g = _gemm(fam, od, bd, epi=1).cpu()
    rq, rs = ref.quantize(g)
    assert torch.equal(sbuf[:ns].cpu(), rs.reshape(-1)), f"{fam} N={N}: scales"
    assert torch.equal(qbuf[:nq].cpu(), rq.reshape(-1).view(U8)), f"{fam} N={N}: codes"
    assert (qbuf[nq:] == GUARD8).all() and (sbuf[ns:] == GUARD8).all(), f"{fam} N={N}: guard bytes written"


# ---- 3. QKV V-insert off the tile grid ----------------------------------------------------------------------------------------------
QKV_FN = {"f8": "ll_gemm_f8_qkv", "w8a8": "ll_gemm_w8a8_qkv", "mx": "ll_gemm_mx_qkv", "mx6": "ll_gemm_mx6_qkv",
          "mx4w6": "ll_gemm_mx4w6_qkv", "mx4": "ll_gemm_mx4_qkv"}


@pytest.mark.parametrize("C", [200, 264])
@pytest.mark.parametrize("fam", ALL_FAMS)
def test_qkv_v_insert_inside_a_tile(fam, C):
    """C = 200 / 264: the V third starts at column 400 / 528, inside an n-tile.  B = 2, L = 75, windows: empty, ending at the last
    cache slot with roped_offset 30, and the whole L at write_start 3.  q / k thirds equal the plain GEMM, the v third of out stays
    unwritten, the window holds the V third of the right tokens and every other slot keeps its sentinel."""
    B, L, K, S = 2, 75, 256, 90
    N, M = 3 * C, B * L
    od = Operands(M, N, K, C)
    bd = hn(f"qb{C}", (N,), 0.1).to(DEV)
    plain = _gemm(fam, od, bd).view(B, L, N).cpu()
    (xq, sx), (wq, sw) = od.operands(fam)
    for ws, ro, wl in ((0, 0, 0), (S - 40, 30, 40), (3, 0, L)):
        out = _nan_bf16(B, L, N)
        cache = torch.full((B, S, C), 7.0, dtype=bf, device=DEV)
        _run(QKV_FN[fam], xq, sx, wq, sw, bd, out, M, N, K, N, cache, B, L, S, ws, ro, wl)
        what = f"{fam} C={C} window ({ws}, {ro}, {wl})"
        assert torch.equal(out[..., : 2 * C].cpu(), plain[..., : 2 * C]), what + ": q / k"
        assert _untouched_bf16(out[..., 2 * C:]), what + ": v third of out written"
        cv = cache.cpu()
        assert torch.equal(cv[:, ws: ws + wl], plain[:, ro: ro + wl, 2 * C:]), what + ": window"
        assert (cv[:, :ws] == 7).all() and (cv[:, ws + wl:] == 7).all(), what + ": slots outside the window"


# ---- 4. quantisers and producers ------------------------------------------------------------------------------------------------------
QUANT = {"mx": ("ll_quantize_mx", mx_ref, (32, 736)), "mx6": ("ll_quantize_mx6", mx6_ref, (256, 768)),
         "mx4": ("ll_quantize_mx4", mx4_ref, (256, 768)), "f8": ("ll_quantize_rows_f8", fp8_ref, (8, 200))}


def _quant_input(fam, rows, K, seed):
    x = (hard_x_f8 if fam == "f8" else hard_x_mx)(rows, max(K, 128), seed)[:, :K].contiguous()
    if K >= 64:
        x[0, 32:64] = 0                                   # an all-zero block in the first row
    return x


@pytest.mark.parametrize("K_sel", [0, 1])
@pytest.mark.parametrize("rows", [1, 3, 257])
@pytest.mark.parametrize("fam", list(QUANT))
def test_quantizers_at_small_rows_and_k_with_row_stride(fam, rows, K_sel):
    """The minimum K and a non-production K, rows 1 / 3 / 257, read at ldx = K + 8 with NaN padding past K: codes and scales equal the
    host restatement (a padding value in any block maximum or row maximum would change a scale), guard bytes after both outputs stay."""
    fn, ref, Ks = QUANT[fam]
    K = Ks[K_sel]
    x = _quant_input(fam, rows, K, rows * 7 + K)
    rq, rs = ref.quantize(x)
    rq, rs = rq.reshape(rows, -1).view(U8), rs.reshape(-1)
    xb = _nan_bf16(rows, K + 8)
    xb[:, :K] = x.to(DEV)
    qbuf = _guarded_u8(rq.numel())
    sbuf = _guarded_u8(rs.numel() * rs.element_size())
    _run(fn, xb, qbuf, sbuf, rows, K, K + 8)
    nq, ns = rq.numel(), rs.numel() * rs.element_size()
    assert torch.equal(sbuf[:ns].cpu(), rs.view(U8).reshape(-1)), f"{fam} rows={rows} K={K}: scales"
    assert torch.equal(qbuf[:nq].cpu(), rq.reshape(-1)), f"{fam} rows={rows} K={K}: codes"
    assert (qbuf[nq:] == GUARD8).all() and (sbuf[ns:] == GUARD8).all(), f"{fam} rows={rows} K={K}: guard bytes written"


# DISPATCH_NCH: C -> (chunks of 512, last chunk whole): 256 (1, partial), 512 (1, whole), 768 (2, p), 1024 (2, w), 1280 (3, p),
# 1536 (3, w: the model's, tested in the families' own modules), 1792 (4, p), 2048 (4, w); plus the narrowest C each family accepts.
PRODUCER_C = (256, 512, 768, 1024, 1280, 1792, 2048)
PRODUCERS = [(f, C) for f in ("mx6", "mx4") for C in PRODUCER_C] + [("mx", C) for C in (32,) + PRODUCER_C] + \
            [(f, C) for f in ("f8", "q8") for C in (8,) + PRODUCER_C]


@pytest.mark.parametrize("fam,C", PRODUCERS)
def test_producers_every_dispatch_instance(ops, fam, C):
    """ln_modulate (with and without mod), its _tab_ form and layernorm_affine emitting each family's codes + scales, B = 2, F = 3,
    frame_len 7 (42 rows: not a multiple of the 4 rows per workgroup): the bytes equal the family's quantiser applied to the bf16
    producer.  q8 (int8 rows): the quantiser is quantize_rows and the _tab_ form is ln_modulate_tab(q8=True)."""
    B, F, fs = 2, 3, 7
    L = F * fs
    suffix = "_" + fam
    q = getattr(ops, {"f8": "quantize_rows_f8", "q8": "quantize_rows"}.get(fam, "quantize" + suffix))
    ln_tab = (lambda *a: ops.ln_modulate_tab(*a, q8=True)) if fam == "q8" else getattr(ops, "ln_modulate_tab" + suffix)
    x = (hard_x_f8 if fam in ("f8", "q8") else hard_x_mx)(B * L, max(C, 128), C)[:, :C].contiguous().view(B, L, C).to(DEV)
    e, mod = hn(f"pe{C}", (B, F, 6, C), 0.5).to(DEV), hn(f"pm{C}", (6, C), 0.1).to(DEV)

    def same(got, want, what):
        assert torch.equal(got[1].cpu().view(U8), want[1].cpu().view(U8)), f"{fam} C={C} {what}: scales"
        assert torch.equal(got[0].cpu().view(U8), want[0].cpu().view(U8)), f"{fam} C={C} {what}: codes"

    for md in (mod, None):
        same(getattr(ops, "ln_modulate" + suffix)(x, e, md, 3, 4, F, 1e-6), q(ops.ln_modulate(x, e, md, 3, 4, F, 1e-6)),
             f"ln_modulate mod={md is not None}")
    tab = ops.modulation_table_f32(e, mod.view(1, 6, C), 0b010010)[0]
    same(ln_tab(x, tab, 3, 4, F, 1e-6), q(ops.ln_modulate_tab(x, tab, 3, 4, F, 1e-6)), "ln_modulate_tab")
    w, b = hn(f"nw{C}", (C,), 0.2).to(DEV), hn(f"nb{C}", (C,), 0.1).to(DEV)
    same(getattr(ops, "layernorm_affine" + suffix)(x, w, b, 1e-6), q(ops.layernorm_affine(x, w, b, 1e-6)), "layernorm_affine")


# ---- 5. MX attention geometry the model never uses --------------------------------------------------------------------------------
ATTN = {
    "H1_Lq1": dict(B=1, H=1, Lq=1, S=70, segs=[(0, 30), (45, 70)]),
    "H3_Lq33": dict(B=1, H=3, Lq=33, S=230, segs=[(0, 40), (75, 230)]),
    "H3_Lq150_B2": dict(B=2, H=3, Lq=150, S=200, segs=[(10, 50), (83, 200)]),
}
D_HEAD = 128


def exact_attention_data(B, H, Lq, S, seed):
    """q: ONE nonzero channel per (row, head), +-2^-1 or +-2^0 on a random channel; k: sparse (8 %) -1 / 0 / 1 times 2^1 or 2^2 per
    (slot, head, 32-channel block); V: integers -3 .. 3 times 2^-1 .. 2^1 per (32-slot block, head, channel).  Every score is one
    integer product q_c k_c, so |s| <= 4, and every V^ value is a multiple of 2^-1 below 6 in magnitude."""
    g = torch.Generator().manual_seed(seed)
    ch = torch.randint(0, D_HEAD, (B, Lq, H, 1), generator=g)
    qv = (torch.randint(0, 2, (B, Lq, H, 1), generator=g) * 2 - 1) * 2.0 ** torch.randint(-1, 1, (B, Lq, H, 1), generator=g)
    q = torch.zeros(B, Lq, H, D_HEAD).scatter_(3, ch, qv.float())
    z = torch.randint(-1, 2, (B, S, H, D_HEAD), generator=g) * (torch.rand(B, S, H, D_HEAD, generator=g) < 0.08)
    k = (z.reshape(B, S, H, 4, 32) * 2.0 ** torch.randint(1, 3, (B, S, H, 4, 1), generator=g)).reshape(B, S, H, D_HEAD)
    w = torch.randint(-3, 4, (B, S, H, D_HEAD), generator=g).float()
    vf = 2.0 ** torch.randint(-1, 2, (B, (S + 31) // 32, 1, H, D_HEAD), generator=g)
    v = w * vf.repeat_interleave(32, 1)[:, :S].reshape(B, S, H, D_HEAD)
    return q.to(bf), k.to(bf), v.to(bf)


def exact_attention_bits(q, k, segs):
    """(significant bits the kernel's fp32 sums can need on this data, largest score spread).  For one query with valid scores in
    [lo, hi], the lazy max M is always some tile's maximum, so M lies in [lo, hi] and every P = 2^(s - M) in [2^(lo - hi), 2^(hi - lo)].
    V^ values are multiples of 2^-1 below 6 in magnitude, so over n keys every partial sum of O (and of l) is a multiple of
    2^(lo - hi - 1) below 6 n 2^(hi - lo): log2(12 n) + (hi - lo) bits."""
    s = torch.einsum("blhd,bshd->bhls", q.double(), k.double())
    assert torch.equal(s, s.round()), "non-integer scores: P = 2^(s - M) would not be exact"
    valid = torch.zeros(k.shape[1], dtype=torch.bool)
    for a, e in segs:
        valid[a:e] = True
    sv = s[..., valid]
    spread = int((sv.amax(-1) - sv.amin(-1)).max())
    return math.log2(12 * int(valid.sum())) + spread, spread


@pytest.mark.parametrize("case", list(ATTN))
def test_mx_attention_edges_with_exact_data(ops, case):
    """H = 1 / 3, Lq = 1 / 33 / 150 (150: two q-tiles of 128 rows, the last one partial), B = 2, S not a multiple of 32 (S32 padded),
    ranges whose first 32-aligned tile starts before them, q and out as slices of wider rows (ldq = H 128 + 64 with NaN padding,
    ldo = H 128 + 32).  exact_attention_bits proves every fp32 sum exact (asserted: < 24 bits, and a score spread <= 8 keeps every
    P^ = 2^(s - M) an exact e4m3 value); with the kernel's normalisation (O times the fp32 reciprocal of l) the output then equals the
    restatement bit for bit, whatever order the kernel sums in.  No byte past H 128 of an output row changes."""
    cfg = ATTN[case]
    B, H, Lq, S, segs = cfg["B"], cfg["H"], cfg["Lq"], cfg["S"], cfg["segs"]
    D, HD = D_HEAD, cfg["H"] * D_HEAD
    q, k, v = exact_attention_data(B, H, Lq, S, Lq + S)
    bits, spread = exact_attention_bits(q, k, segs)
    assert spread <= 8 and bits < 24, (bits, spread)
    scale = unit_c_scale()
    kd, vd = k.to(DEV), v.to(DEV)
    sh = ops.kv_shadow_mx_alloc(kd)
    ops.kv_shadow_mx(kd, vd, sh, 0, S)
    ldq, ldo = HD + 64, HD + 32
    qb = _nan_bf16(B * Lq, ldq)
    qb[:, :HD] = q.reshape(B * Lq, HD).to(DEV)
    ob = _nan_bf16(B * Lq, ldo)
    (s0, e0), (s1, e1) = segs
    _run("ll_flash_attn_mx", qb, sh["kq"], sh["ks"], sh["vq"], sh["vs"], ob, B, Lq, H, D, ldq, ldo, S, sh["kq"].shape[1],
         s0, e0 - s0, s1, e1 - s1, scale)
    want = MA.mx_attention_cache(q, k, v, segs, scale=scale, dtype=torch.float64, rcp=True).to(bf)
    got = ob[:, :HD].cpu().view(B, Lq, H, D)
    assert torch.equal(got, want), f"{case}: max |diff| {(got.float() - want.float()).abs().max()}"
    assert _untouched_bf16(ob[:, HD:]), f"{case}: bytes past H x 128 written"
