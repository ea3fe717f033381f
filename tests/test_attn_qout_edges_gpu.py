"""The code-emitting attention kernels at their row, range and stride edges, through the C ABI: flash_attn_asm_mx / mx6 / mx4_kernel
(ll_flash_attn_q) and the OUTF forms of flash_attn_mx_kernel (ll_flash_attn_mx_q).  Every comparison is byte for byte.

ll_flash_attn_q runs (a) the picked-row data of tests/attn_qout_exact.py, whose expected bytes are the HOST quantisers' of chosen V
rows (tests/test_attn_qout_edges_host.py holds the construction's conditions), and (b) random data, where the header's contract is
the reference: the bytes of ops.quantize_<fmt>(ops.flash_attn(...)) under the same tuning.  ll_flash_attn_mx_q runs the exact data
of tests/mx_attn_exact.py over the host's shadow bytes; the expected bytes are the host quantiser's of the expected bf16 bits.
Codes and scales go into sentinel-filled buffers with two spare rows before and after the rows and padded strides, and the WHOLE
buffers are compared: what lies outside the rows' own H heads keeps the sentinel.  Refused calls write nothing."""
import contextlib
import itertools
import math

import numpy as np
import pytest
import torch

import attn_qout_exact as Q
import mx_attn_exact as X
from quant_exact import unit_c_scale
from attn_qout_emu import BITS, QUANT
from util import bf

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = 0xA5                        # neither 0 nor 127
NAN16 = 0x7FC1                     # q / k / v padding: whatever is read from there poisons the row
QID = {"mx": 1, "mx6": 2, "mx4": 3}
SPARE = 2                          # sentinel rows before and after the rows
SCALE = 1.0 / math.sqrt(128)
INVALID = -1                       # LL_ERR_INVALID_ARG


@pytest.fixture(scope="module")
def ops():
    from longlive_amd import ops as O
    return O


def _L():
    from longlive_amd import _lib
    return _lib, _lib.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


@contextlib.contextmanager
def min_keys(n):
    _, lib = _L()
    assert lib.ll_set_tuning(b"attn_asm_min_keys", n) == 0
    try:
        yield
    finally:
        lib.ll_set_tuning(b"attn_asm_min_keys", 512)


def _fmt(ops, name):
    return {"mx": ops.MX, "mx6": ops.MX6, "mx4": ops.MX4}[name]


def _nan(*shape):
    return torch.full(shape, NAN16, dtype=torch.int16, device=DEV).view(bf)


def _padded_rows(t, ld):
    """[rows, C] bf16 -> [rows, ld] with NaN padding columns"""
    rows, C = t.shape
    if ld == C:
        return t.contiguous()
    out = _nan(rows, ld)
    out[:, :C] = t
    return out


def _out_buffers(rows, wc, ws, pad_c, pad_s):
    codes = torch.full((rows + 2 * SPARE, wc + pad_c), SENT, dtype=torch.uint8, device=DEV)
    scales = torch.full((rows + 2 * SPARE, ws + pad_s), SENT, dtype=torch.uint8, device=DEV)
    return codes, scales


def _assert_bytes(got, want, what):
    """got: the whole (codes, scales) buffers; want: the rows' own bytes [rows, wc] / [rows, ws] (numpy uint8)"""
    for name, g, w in zip(("scales", "codes"), got[::-1], want[::-1]):
        g = g.cpu().numpy()
        full = np.full(g.shape, SENT, dtype=np.uint8)
        full[SPARE:SPARE + w.shape[0], :w.shape[1]] = w
        if not np.array_equal(g, full):
            bad = np.argwhere(g != full)
            r, c = (int(x) for x in bad[0])
            where = "a spare row" if not SPARE <= r < SPARE + w.shape[0] else "stride padding" if c >= w.shape[1] else "the rows"
            raise AssertionError(f"{what}: {name}: {len(bad)} bytes differ, first in {where} at row {r - SPARE} byte {c}: got {g[r, c]:#x} want "
                                 f"{full[r, c]:#x}; rows that differ: {sorted({int(x) - SPARE for x in bad[:, 0]})[:12]}")


def _u8(t):
    return t.contiguous().view(torch.uint8).reshape(-1, t.shape[-1]).cpu().numpy()


# ---- ll_flash_attn_q ---------------------------------------------------------------------------------------------------------------------
class KV:
    """k / v [B, Sk, H, 128] laid out for the C ABI.  wide: rows of H * 128 + 8 elements and a batch stride 24 elements above Sk rows;
    off: the base pointers that many rows into their buffers; all of the padding is NaN."""

    def __init__(self, k, v, wide, off=0):
        B, Sk, H, _ = k.shape
        C = H * 128
        self.ldk, slack, self.off = (C + 8, 24, off) if wide else (C, 0, off)
        self.kbs = Sk * self.ldk + slack
        self.bufs = []
        for t in (k, v):
            buf = _nan(self.off * self.ldk + B * self.kbs)
            rows = buf[self.off * self.ldk:].view(B, self.kbs)[:, :Sk * self.ldk].view(B, Sk, self.ldk)
            rows[..., :C] = t.reshape(B, Sk, C)
            self.bufs.append(buf)
        self.kptr, self.vptr = (b.data_ptr() + 2 * self.off * self.ldk for b in self.bufs)


def _asm_q(fmt, q, kv, seg_args, pad_q=0, pad_c=16, pad_s=4, scale=SCALE, rc_want=0, fmt_id=None, H_arg=None, ldc=None, lds=None, ldq=None,
           bufs=None):
    """One ll_flash_attn_q call -> the whole sentinel-filled (codes, scales) buffers."""
    L, lib = _L()
    B, Lq, H, _ = q.shape
    C = H * 128
    wc, ws = H * 16 * BITS[fmt], H * 4
    qb = _padded_rows(q.reshape(B * Lq, C), C + pad_q)
    codes, scales = bufs or _out_buffers(B * Lq, wc, ws, pad_c, pad_s)
    ldc, lds = codes.shape[1] if ldc is None else ldc, scales.shape[1] if lds is None else lds
    rc = lib.ll_flash_attn_q(QID[fmt] if fmt_id is None else fmt_id, qb.data_ptr(), kv.kptr, kv.vptr, codes.data_ptr() + SPARE * codes.shape[1],
                             scales.data_ptr() + SPARE * scales.shape[1], B, Lq, H_arg or H, ldq or C + pad_q, ldc, lds, kv.ldk, kv.kbs, *seg_args,
                             scale, _stream())
    if rc_want == 0:
        L.check(rc, "ll_flash_attn_q")
    else:
        assert rc == rc_want, rc
    torch.cuda.synchronize()
    return codes, scales


def _plan_ok(ops, fmt, p):
    plan = ops.flash_attn_q_plan(_fmt(ops, fmt), p.Lq, p.H, p.B, p.segments())
    nwg = (p.Lq + 255) // 256 * p.H * p.B
    assert plan.startswith(f"flash_attn_asm_{fmt}_kernel") and f"{nwg} workgroups of 256 query rows" in plan, plan
    assert ops.flash_attn_q_ok(_fmt(ops, fmt), p.H, p.segments())


@pytest.fixture(scope="module")
def random_rows(ops):
    """case (b): the random q, k, v of a geometry and the bf16 kernel's rows under attn_asm_min_keys = 128, shared by the formats"""
    cache = {}

    def get(geom, scale=None):
        key = (Q.case_id(geom), scale)
        if key not in cache:
            p = Q.Picked.get(geom, "mx")
            q, k, v = Q.hash_qkv("qe" + Q.case_id(geom), p.B, p.Lq, p.H, p.Sk)
            with min_keys(128):
                rows = ops.flash_attn(q, k, v, p.segments(), scale=scale).view(p.B, p.Lq, p.H * 128)
            cache[key] = (q, k, v, rows)
        return cache[key]
    return get


ASM = [(g, f) for g in Q.QOUT_ASM_CASES for f in Q.FMTS] + [(g, "mx") for g in Q.QOUT_ASM_ODD]
_ids = lambda v: Q.case_id(v) if isinstance(v, tuple) else str(v)


@pytest.mark.parametrize("geom,fmt", ASM, ids=_ids)
def test_generated_kernel_picked_rows_are_the_host_bytes(ops, geom, fmt):
    """(a): every output row is a chosen V row; the bytes are the host quantiser's.  Lq 1 .. 328, range starts 0 / 1 / 37 / 63 / 64 / 65,
    128 .. 1437 keys, ragged last tiles, adjacent ranges with a ragged seam, H up to 12, B = 2."""
    p = Q.Picked.get(geom, fmt)
    q, k, v = p.tensors(DEV)
    with min_keys(128):
        _plan_ok(ops, fmt, p)
        got = _asm_q(fmt, q, KV(k, v, False), p.segs_args())
    _assert_bytes(got, (p.codes, p.scales), f"{p}")


@pytest.mark.parametrize("geom,fmt", ASM, ids=_ids)
def test_generated_kernel_random_rows_are_the_quantiser_of_the_bf16_twin(ops, random_rows, geom, fmt):
    """(b): the header's contract on random data, V with block maxima over nine binades and exact zeros."""
    p = Q.Picked.get(geom, "mx")
    q, k, v, rows = random_rows(geom)
    want = getattr(ops, "quantize_" + fmt)(rows)
    with min_keys(128):
        got = _asm_q(fmt, q, KV(k, v, False), p.segs_args())
    _assert_bytes(got, (_u8(want[0]), _u8(want[1])), f"{fmt} {Q.case_id(geom)} random")


STRIDE_GEOMS = [g for g in Q.QOUT_ASM_CASES if g[1] == 257 or g[0] == 2]


@pytest.mark.parametrize("geom", STRIDE_GEOMS, ids=_ids)
@pytest.mark.parametrize("fmt", Q.FMTS)
def test_generated_kernel_strides(geom, fmt):
    """ldq = H * 128 + {0, 8} (ll_flash_attn_q requires multiples of 8 elements), ldc = the row's bytes + {0, 16, 48}, lds = 4 H +
    {0, 4, 12}, k / v rows of H * 128 + {0, 8} elements (the wide ones under a batch stride above Sk rows), base pointers zero and
    three rows into their buffers: the same bytes in every combination."""
    p = Q.Picked.get(geom, fmt)
    assert geom in STRIDE_GEOMS and len(STRIDE_GEOMS) == 4
    q, k, v = p.tensors(DEV)
    with min_keys(128):
        for wide, off in ((False, 0), (False, 3), (True, 0), (True, 3)):
            kv = KV(k, v, wide, off)
            for pad_q in (0, 8):
                for pad_c in (0, 16, 48):
                    for pad_s in (0, 4, 12):
                        got = _asm_q(fmt, q, kv, p.segs_args(), pad_q, pad_c, pad_s)
                        _assert_bytes(got, (p.codes, p.scales), f"{p} ldq +{pad_q} ldc +{pad_c} lds +{pad_s} wide k/v {wide} base +{off} rows")


@pytest.mark.parametrize("fmt", Q.FMTS)
def test_generated_kernel_other_scales(ops, random_rows, fmt):
    """Half the usual scale, and the scale whose c = scale x log2 e is exactly 1."""
    geom = Q.QOUT_ASM_CASES[7]                         # B 2, Lq 129, H 4, 1025 keys from slot 1
    p = Q.Picked.get(geom, "mx")
    for scale in (SCALE * 0.5, unit_c_scale()):
        q, k, v, rows = random_rows(geom, scale)
        want = getattr(ops, "quantize_" + fmt)(rows)
        with min_keys(128):
            got = _asm_q(fmt, q, KV(k, v, False), p.segs_args(), scale=scale)
        _assert_bytes(got, (_u8(want[0]), _u8(want[1])), f"{fmt} scale {scale}")
    q, k, v, rows = random_rows(geom)
    assert not torch.equal(rows, random_rows(geom, SCALE * 0.5)[3])                  # the scale reaches the kernel


def test_generated_kernel_refusals_write_nothing():
    """LL_ERR_INVALID_ARG with the argument in the message, and both buffers keep the sentinel."""
    _, lib = _L()
    geom = Q.QOUT_ASM_CASES[1]                         # Lq 31, H 2, keys [1, 130)
    p = Q.Picked.get(geom, "mx")
    q, k, v = p.tensors(DEV)
    kv = KV(k, v, False)
    C = p.H * 128
    seg = p.segs_args()
    bad = []
    for fmt in Q.FMTS:
        wc, ws = p.H * 16 * BITS[fmt], p.H * 4
        bad += [(fmt, dict(ldc=wc + 8), "code row stride"), (fmt, dict(lds=ws + 2), "scale row stride"), (fmt, dict(ldc=wc - 16), "code row stride"),
                (fmt, dict(lds=ws - 4), "scale row stride"), (fmt, dict(ldq=C + 4), "ldq="), (fmt, dict(ldq=C - 8), "ldq="),
                (fmt, dict(seg=(1, 64, 66, 64)), "not covered"), (fmt, dict(seg=(1, 127, 0, 0)), "not covered"),
                (fmt, dict(seg=(1, 100, 50, 100)), "overlap")]
        if fmt != "mx":
            bad += [(fmt, dict(H_arg=1), "1 heads")]
    bad += [("mx", dict(fmt_id=0), "fmt=0"), ("mx", dict(fmt_id=4), "fmt=4")]
    with min_keys(128):
        for fmt, kw, needle in bad:
            kw = dict(kw)
            bufs = _out_buffers(p.B * p.Lq, p.H * 16 * BITS[fmt], p.H * 4, 16, 4)
            got = _asm_q(fmt, q, kv, kw.pop("seg", seg), rc_want=INVALID, bufs=bufs, **kw)
            msg = lib.ll_last_error().decode()
            assert needle in msg and "ll_flash_attn_q" in msg, (fmt, kw, msg)
            assert all(bool((t == SENT).all()) for t in got), (fmt, kw)
    # under the shipped threshold the 129-key range is below attn_asm_min_keys: declined, and ll_flash_attn_q_ok says so
    assert lib.ll_flash_attn_q_ok(1, p.H, *seg) == 0
    bufs = _out_buffers(p.B * p.Lq, C, p.H * 4, 16, 4)
    got = _asm_q("mx", q, kv, seg, rc_want=INVALID, bufs=bufs)
    assert "not covered" in lib.ll_last_error().decode() and all(bool((t == SENT).all()) for t in got)


# ---- ll_flash_attn_mx_q -----------------------------------------------------------------------------------------------------------------
def _shadow(b):
    """The host's shadow bytes of a built case on the device: kq, ks, vq, vs (uint8)."""
    return [t.view(torch.uint8).to(DEV).contiguous() for t in (b.kq, b.ks, b.vq, b.vs)]


def _mx_want(b, fmt, Lq=None):
    c = b.case
    Lq = Lq or c.Lq
    codes, scales = QUANT[fmt](b.want[:, :Lq].reshape(c.B * Lq, c.H * 128))
    return (np.ascontiguousarray(codes).reshape(c.B * Lq, -1).view(np.uint8), np.ascontiguousarray(scales).reshape(c.B * Lq, -1).view(np.uint8))


def _mx_q(fmt, b, shadow, Lq=None, pad_q=0, pad_c=16, pad_s=4, rc_want=0, bufs=None, **kw):
    """One ll_flash_attn_mx_q call on the first Lq rows of a built case -> the whole sentinel-filled (codes, scales) buffers."""
    L, lib = _L()
    c = b.case
    B, H, Lq = c.B, c.H, Lq or c.Lq
    C = H * 128
    qb = _padded_rows(b.q[:, :Lq].reshape(B * Lq, C).to(DEV), C + pad_q)
    codes, scales = bufs or _out_buffers(B * Lq, H * 16 * BITS[fmt], H * 4, pad_c, pad_s)
    a = dict(fmt_id=QID[fmt], H=H, hd=128, ldq=C + pad_q, ldc=codes.shape[1], lds=scales.shape[1], S=c.S, S32=c.S32, segs=c.seg_args(), scale=X.SCALE)
    a.update(kw)
    rc = lib.ll_flash_attn_mx_q(a["fmt_id"], qb.data_ptr(), *(t.data_ptr() for t in shadow), codes.data_ptr() + SPARE * codes.shape[1],
                                scales.data_ptr() + SPARE * scales.shape[1], B, Lq, a["H"], a["hd"], a["ldq"], a["ldc"], a["lds"], a["S"], a["S32"],
                                *a["segs"], a["scale"], _stream())
    if rc_want == 0:
        L.check(rc, "ll_flash_attn_mx_q")
    else:
        assert rc == rc_want, rc
    torch.cuda.synchronize()
    return codes, scales


def _mx_plan_ok(ops, c, Lq=None):
    nt, nr = c.plan_counts()
    Lq = Lq or c.Lq
    wg = (Lq + 127) // 128 * c.H * c.B
    plan = ops.flash_attn_mx_plan(Lq, c.H, c.B, c.segs)
    assert f"{wg} workgroups of 128 query rows, {nt} key tiles of 64 in {nr} range" in plan, plan


@pytest.mark.parametrize("case", X.EXACT_CASES, ids=repr)
def test_mx_attention_exact_case_8bit(ops, case):
    """Every exact-data case of the bf16 form (H = 1 or 3) with MXFP8 codes out."""
    b = X.Built.get(case)
    _mx_plan_ok(ops, case)
    _assert_bytes(_mx_q("mx", b, _shadow(b)), _mx_want(b, "mx"), f"{case} mx")


@pytest.mark.parametrize("case", X.QOUT_EVEN, ids=repr)
@pytest.mark.parametrize("fmt", Q.FMTS)
def test_mx_attention_even_heads(ops, case, fmt):
    """H = 2, 4, 12 in all three formats: 257 rows over two ranges, B = 2 with the ranges in reverse order, the staging clamp, sweeps
    from slots 31 and 33."""
    b = X.Built.get(case)
    _mx_plan_ok(ops, case)
    want = _mx_want(b, fmt)
    assert len(np.unique(want[1])) > 1
    _assert_bytes(_mx_q(fmt, b, _shadow(b)), want, f"{case} {fmt}")
    if case is X.QOUT_BATCH:
        _assert_bytes(_mx_q(fmt, b, _shadow(b), pad_q=136, pad_c=48, pad_s=12), want, f"{case} {fmt} wide")


@pytest.mark.parametrize("Lq", X.LQ)
@pytest.mark.parametrize("case,fmt", [(X.ROWS, "mx")] + [(X.QOUT_ROWS, f) for f in Q.FMTS], ids=lambda v: str(v))
def test_mx_attention_rows_and_strides(ops, case, fmt, Lq):
    """Lq from 1 to 257 x ldq = H * 128 + {0, 8, 136}, ldc = the row's bytes + {0, 16, 48}, lds = 4 H + {0, 4, 12}."""
    b = X.Built.get(case)
    sh = _shadow(b)
    _mx_plan_ok(ops, case, Lq)
    want = _mx_want(b, fmt, Lq)
    for pad_q, pad_c, pad_s in itertools.product((0, 8, 136), (0, 16, 48), (0, 4, 12)):
        _assert_bytes(_mx_q(fmt, b, sh, Lq, pad_q, pad_c, pad_s), want, f"{case} {fmt} Lq {Lq} ldq +{pad_q} ldc +{pad_c} lds +{pad_s}")


def test_mx_attention_refusals_write_nothing():
    """Every refusal of the bf16 form's suite, and the output form's own: strides off 16 / 4 bytes or below the row, fmt 0 and 4, odd H
    with a packed format."""
    _, lib = _L()
    b = X.Built.get(X.QOUT_EVEN[4])
    c = b.case
    sh = _shadow(b)
    C = c.H * 128
    ws = c.H * 4
    bad = []
    for fmt in Q.FMTS:
        wc = c.H * 16 * BITS[fmt]
        bad += [(fmt, dict(ldc=wc + 8), "code row stride"), (fmt, dict(lds=ws + 2), "scale row stride"), (fmt, dict(ldc=wc - 16), "code row stride"),
                (fmt, dict(lds=ws - 4), "scale row stride")]
        if fmt != "mx":
            bad += [(fmt, dict(H=1), "H=1 must be even")]
    bad += [("mx", dict(fmt_id=0), "fmt=0"), ("mx", dict(fmt_id=4), "fmt=4"),
            ("mx", dict(segs=(0, 50, 40, 30)), "overlap"), ("mx", dict(segs=(40, 30, 0, 41)), "overlap"), ("mx", dict(segs=(0, 50, 0, 50)), "overlap"),
            ("mx", dict(scale=0.0), "scale="), ("mx", dict(scale=-X.SCALE), "scale="), ("mx", dict(scale=float("nan")), "scale="),
            ("mx", dict(scale=float("inf")), "scale="), ("mx", dict(S32=c.S32 + 32), "S32="), ("mx", dict(S32=c.S), "S32="),
            ("mx", dict(segs=(0, c.S + 1, 0, 0)), "first key range"), ("mx", dict(segs=(0, 10, c.S - 5, 6)), "second key range"),
            ("mx", dict(hd=64), "head_dim=64"), ("mx", dict(ldq=C + 4), "ldq="), ("mx", dict(ldq=C - 8), "ldq=")]
    assert c.S % 32                                     # S32 = S is a refusal
    for fmt, kw, needle in bad:
        bufs = _out_buffers(c.B * c.Lq, c.H * 16 * BITS[fmt], ws, 16, 4)
        got = _mx_q(fmt, b, sh, rc_want=INVALID, bufs=bufs, **kw)
        msg = lib.ll_last_error().decode()
        assert needle in msg and "ll_flash_attn_mx_q" in msg, (fmt, kw, msg)
        assert all(bool((t == SENT).all()) for t in got), (fmt, kw)
