"""The harness of the quantised-output forms of the generated self-attention kernel on the CPU emulator (plain helpers, no tests):
the formats and their host quantisers, the packed-row layout of a head's codes, one workgroup of a kernel text run over bf16 bit
arrays, the bytes the host quantiser expects, the edge blocks of the scale rule and the code rounding, and the one-hot case that
forces them through attention rows.  Used by tests/test_attn_asm_qout_emu.py and the code-emitting attention suites."""
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "longlive_amd", "csrc", "gen"))

import attn_asm_gen as G          # noqa: E402
import gfx950_emu as E            # noqa: E402
import mx4_ref                    # noqa: E402
import mx6_ref                    # noqa: E402
import mx_ref                     # noqa: E402

FMTS = ["mx", "mx6", "mx4"]
SENT = 0xA5                       # neither 0 nor 127
D = 128
MAXV = {"mx": 448.0, "mx6": 7.5, "mx4": 6.0}               # largest code value
STEP = {"mx": 2.0 ** -9, "mx6": 0.125, "mx4": 0.5}         # smallest subnormal code value
BITS = {"mx": 8, "mx6": 6, "mx4": 4}
QUANT = {"mx": lambda x: tuple(t.view(torch.uint8).numpy() if t.dtype != torch.uint8 else t.numpy() for t in mx_ref.quantize(x)),
         "mx6": lambda x: tuple(t.numpy() for t in mx6_ref.quantize(x)),
         "mx4": lambda x: tuple(t.numpy() for t in mx4_ref.quantize(x))}


def bf16_bits(x):
    return E.bf16_round(np.asarray(x, dtype=np.float32)).astype(np.uint16)


def bf16_val(bits):
    return E.bf16_to_f32(np.asarray(bits, dtype=np.uint32))


def head_code_bytes(fmt, hh):
    """byte positions, inside a packed row, of head hh's 128 codes (blocks j = 4 (hh & 1) + db of super-block hh >> 1)"""
    if fmt == "mx":
        return np.arange(hh * 128, hh * 128 + 128)
    blk, sup = (24, 192) if fmt == "mx6" else (16, 128)
    return np.concatenate([(hh >> 1) * sup + 2 * blk * db + blk * (hh & 1) + np.arange(blk) for db in range(4)])


def run(text, mode, qb_, kb_, vb_, rows_valid, nkeys, nheads, head, kstart, fmt=None):
    """One workgroup over bf16 bit arrays q [rows_valid, nheads, 128], k / v [kstart + nkeys, nheads, 128].  Plain text: returns the
    head's bf16 bits [rows_valid, 128].  Quantised form: returns the WHOLE code [256, row bytes] and scale [256, nheads * 4] buffers,
    prefilled with the sentinel."""
    ldq = ldk = nheads * D
    mem = E.Memory()
    aq, ak, av = mem.alloc(qb_), mem.alloc(kb_), mem.alloc(vb_)
    if fmt is None:
        ao = mem.alloc(np.full((rows_valid, nheads, D), 0x7FC0, dtype=np.uint16))
        obase, ldo_b = ao + head * D * 2, nheads * D * 2
    else:
        ldo_b = nheads * D * BITS[fmt] // 8
        ao = mem.alloc(np.full((256, ldo_b), SENT, dtype=np.uint8))
        asc = mem.alloc(np.full((256, nheads * 4), SENT, dtype=np.uint8))
        obase = ao + int(head_code_bytes(fmt, head)[0])
    m = E.Machine(text, mem, 4, mode=mode)
    c = np.float32((1.0 / math.sqrt(D)) * 1.4426950408889634)
    nt = (nkeys + 63) // 64
    for wv in m.waves:
        s = wv.s

        def put64(i, val):
            s[i], s[i + 1] = val & 0xFFFFFFFF, val >> 32
        put64(G.S_Q, aq + head * D * 2)
        put64(G.S_O, obase)
        put64(G.S_K, ak + (kstart * ldk + head * D) * 2)
        put64(G.S_V, av + (kstart * ldk + head * D) * 2)
        s[G.S_LDQ], s[G.S_LDO], s[G.S_LDK] = ldq * 2, ldo_b, ldk * 2
        s[G.S_ROWS], s[G.S_NT], s[G.S_LASTV] = rows_valid, nt, nkeys - 64 * (nt - 1)
        s[G.S_C] = int(E.f2u(c))
        s[G.S_NREC] = (nkeys - 1) * ldk * 2 + D * 2
        if fmt is not None:
            put64(G.S_SC, asc + 4 * head)
            s[G.S_SCLD] = nheads * 4
        wv.v[G.V_TID] = 64 * wv.id + np.arange(64, dtype=np.uint32)
        wv.v[1:] = 0x7FC0BEEF                           # uninitialised registers are NaN poison
        wv.a[:] = 0x7FC0BEEF
    m.run()
    if fmt is None:
        return mem.get(ao).view(np.uint16).reshape(rows_valid, nheads, D)[:, head].copy()
    return mem.get(ao).reshape(256, ldo_b).copy(), mem.get(asc).reshape(256, nheads * 4).copy()


def expected(fmt, out_bits, nheads, head):
    """the sentinel-filled buffers with the host quantiser's bytes of the head's bf16 rows in the head's places"""
    rows = out_bits.shape[0]
    full = np.zeros((rows, nheads, D), dtype=np.uint16)
    full[:, head] = out_bits
    x = torch.from_numpy((full.reshape(rows, nheads * D).astype(np.uint32) << 16).view(np.float32).copy()).to(torch.bfloat16)
    codes, scales = QUANT[fmt](x)
    wc = np.full((256, nheads * D * BITS[fmt] // 8), SENT, dtype=np.uint8)
    ws = np.full((256, nheads * 4), SENT, dtype=np.uint8)
    cols = head_code_bytes(fmt, head)
    wc[:rows, cols] = codes.reshape(rows, -1)[:, cols]
    ws[:rows, 4 * head: 4 * head + 4] = scales.reshape(rows, -1)[:, 4 * head: 4 * head + 4]
    return wc, ws


def _next(x, k=1):
    """the bf16 value k ulps above (k < 0: below) a positive bf16 value"""
    return float(bf16_val(np.uint32(int(bf16_bits(x)) + k)))


def edge_blocks(fmt):
    """32-value blocks (float, all bf16-representable) and what each is there for"""
    mv, st = MAXV[fmt], STEP[fmt]
    sc = 2.0 ** -3
    tie_lo, tie_hi = (1.25, 1.75) if fmt == "mx4" else (1.0625, 1.1875)       # halfway between two normal codes: down to even, up to even
    fill = [tie_lo, tie_hi, -tie_lo, -tie_hi, 0.75 * st, 0.25 * st, 0.5 * st, 1.5 * st, -0.25 * st, -0.5 * st, -0.75 * st, 2.5 * st,
            0.0, 1.0, -2.0, 3.0]
    base = np.array(([mv] + fill + [-mv] + fill[::-1])[:32]) * sc
    blocks = {"zero": np.zeros(32), "amax_at_max": base.copy()}
    b = base.copy(); b[0] = _next(mv * sc, 1); blocks["amax_one_ulp_above"] = b
    b = base.copy(); b[0] = _next(mv * sc, -1); b[17] = -b[0]; blocks["amax_one_ulp_below"] = b
    t = np.zeros(32)
    t[:6] = [2.0 ** -130, -2.0 ** -133, 2.0 ** -132, 3 * 2.0 ** -133, -2.0 ** -131, 5 * 2.0 ** -133]
    blocks["clamp"] = t
    return blocks


def one_hot_case(fmt, seed=7, nheads=2, head=1, kstart=3):
    """256 queries of +-1 entries, 4 * 64 + 20 keys: query i's key sits at slot pos[i] and equals 20 q_i (its score beats every other
    by more than 2^-149 after the softmax, so every other probability is exactly 0, l = 1 and the output row is V[pos[i]]); the
    unassigned keys are zero.  Query 0 has TWO such keys in one tile (l = 2): its output is half the sum of their V rows, which turns
    the smallest negative bf16 subnormal into -0.0."""
    rng = np.random.default_rng(seed)
    rows, nkeys = 256, 4 * 64 + 20
    q = rng.choice([-1.0, 1.0], size=(rows, nheads, D)).astype(np.float32)
    pos = rng.permutation(nkeys)
    twin = int(pos[rows])                                 # an unassigned slot ...
    same_tile = [i for i in range(rows) if pos[i] // 64 == twin // 64]
    pos[[0, same_tile[0]]] = pos[[same_tile[0], 0]]       # ... in the tile of query 0's key
    k = np.zeros((kstart + nkeys, nheads, D), dtype=np.float32)
    v = (rng.standard_normal((kstart + nkeys, nheads, D)) * np.exp2(rng.integers(-8, 8, (kstart + nkeys, nheads, 4)).repeat(32, -1))).astype(np.float32)
    k[kstart + pos[:rows]] = 20.0 * q
    k[kstart + twin] = 20.0 * q[0]
    blocks = edge_blocks(fmt)
    names = list(blocks)
    for i in range(1, 1 + 2 * len(names)):                # every edge block at two block positions, in rows of two waves
        r = i if i <= len(names) else 150 + i
        for db in range(4):
            v[kstart + pos[r], head, 32 * db: 32 * db + 32] = blocks[names[(i + db) % len(names)]]
    row0 = np.zeros(D)
    row0[:4] = [-2.0 ** -133, 2.0 ** -120, -2.0 ** -125, 2.0 ** -133]
    row0[32:36] = [-2.0 ** -133, MAXV[fmt], 0.25 * STEP[fmt] * 2, -0.75 * STEP[fmt] * 2]
    v[kstart + pos[0], head] = row0
    v[kstart + twin, head] = 0.0
    return bf16_bits(q), bf16_bits(k), bf16_bits(v), rows, nkeys, pos
